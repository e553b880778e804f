// SPDX-License-Identifier: Apache-2.0
// Compressed cube maps sampled by direction at a level of detail per point (astcenc_amd_sample_cube_tensors_device): for every
// point of a grid of directions (dx, dy, dz) and a lambda of its own, the sample of one level (MIP_NEAREST) or the blend of two
// (MIP_LINEAR), each level sampled on the face the direction points at, a tap that leaves the face reading the neighbouring face
// as the "Cube edges" rule of the mip filter names it (include/astcenc_amd.h has the definition, tests/sample_cube_model.py
// spells it out in numpy).
//
// The work item, the level walk, the batches, the sums, the blend, the stores (lod_walk_tile) and the table writer
// (decode_lod_table_build; the launch is the lod call's DecodeLodLaunch, its z the cube) are decode_lod.h's; this header
// holds what differs: the record, the coordinate stage (validity, the face, sc / ma and tc / ma -- divided once per point: the
// quotients do not depend on the level) and the taps of a level, whose layer is the tap's own: SamplePoint::blk counts blocks
// from the stream's start, so one level pass decodes blocks of several faces and deduplicates them across faces.
//
// Included by kernel_decode_cube.hip and tests/harness/decode_cube_check.cpp only: not part of wave_decode.h's include graph.
//
// Layout: decode_lod.h's -- ImageSetTable, first[count], padding, DecodeCubeRecord[count], then the DecodeLodLevel records of
// grid 0's levels, of grid 1's ...
#pragma once
#include "decode_lod.h"
#include "mip_resample.h"

namespace astcd { inline namespace ASTC_VARIANT {

struct DecodeCubeRecord {
	const float* dirs;                // point (i, j): dirs[j * dir_row + 3 i], dx, dy, dz
	size_t   dir_row;                 // floats from row to row of points
	const float* lod;                 // point (i, j): lod[j * lod_row + i]; null: +0.0 everywhere
	size_t   lod_row;
	void*    out;                     // the grid's `out`
	size_t   row;                     // elements from output row to output row
	size_t   levels;                  // bytes from the table's start to the record of level 0
	uint32_t level_count;             // 1 .. 32
	uint32_t cube;                    // layers 6 cube .. 6 cube + 5, in every level
	uint32_t out_x, out_y;
	uint32_t filter, mip_filter;
	uint32_t tw_log2;                 // the tile is (1 << tw_log2) points across and 64 >> tw_log2 down
	uint32_t tiles_x;                 // tiles per row of tiles: ceil(out_x / tw)
	uint32_t x_step;                  // elements from column to column (1 planar, `channels` interleaved)
	float    lod_bias;
	TensorParams fmt;
};
static_assert(sizeof(DecodeCubeRecord) % 8 == 0, "records are read word by word and hold pointers");

inline size_t decode_cube_bytes(const DecodeLodLaunch* grids, uint32_t count) { return decode_lod_table_bytes<DecodeCubeRecord>(grids, count); }

/* The cube call's table (decode_lod_table_build; 2D footprints): its own are the triples and the cube; no address modes. */
inline uint32_t decode_cube_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                  const DecodeLodLaunch* grids, uint32_t count)
{
	return decode_lod_table_build<DecodeCubeRecord>(out, images, streams, format, sampler, grids, count, [](DecodeCubeRecord& r, const DecodeLodLaunch& g) -> DecodeCubeRecord&
	{
		r.dirs = g.d_coords;
		r.dir_row = g.coord_row_pitch;
		r.cube = g.z;
		return r;
	});
}

/* A point is valid when dx, dy and dz are finite, not all three are zero (of either sign) and lambda' is not a NaN. */
WV_FN bool cube_valid(float dx, float dy, float dz, float lambda)
{
	const float inf = __builtin_inff();
	const float a = __builtin_fabsf(dx), b = __builtin_fabsf(dy), c = __builtin_fabsf(dz);
	// (a NaN fails its comparison)
	return a < inf && b < inf && c < inf && (a != 0.0f || b != 0.0f || c != 0.0f) && lambda == lambda;
}

/* The face of a valid direction and its face coordinates before the division: the major axis is x when |dx| >= |dy| and
 * |dx| >= |dz|, else y when |dy| >= |dz|, else z; face = 2 axis + (the major component is negative); ma = |major|;
 * sc = d . S_f and tc = d . T_f, each one component with a sign (the GL table):
 *     +X (-dz, -dy)   -X (dz, -dy)   +Y (dx, dz)   -Y (dx, -dz)   +Z (dx, -dy)   -Z (-dx, -dy) */
struct CubeFace { uint32_t face; float sc, tc, ma; };

WV_FN CubeFace cube_face(float dx, float dy, float dz)
{
	const float a = __builtin_fabsf(dx), b = __builtin_fabsf(dy), c = __builtin_fabsf(dz);
	CubeFace r;
	if (a >= b && a >= c)
	{
		const bool neg = dx < 0.0f;
		r.face = neg ? 1u : 0u; r.ma = a;
		r.sc = neg ? dz : -dz; r.tc = -dy;
	}
	else if (b >= c)
	{
		const bool neg = dy < 0.0f;
		r.face = neg ? 3u : 2u; r.ma = b;
		r.sc = dx; r.tc = neg ? -dz : dz;
	}
	else
	{
		const bool neg = dz < 0.0f;
		r.face = neg ? 5u : 4u; r.ma = c;
		r.sc = neg ? -dx : dx; r.tc = -dy;
	}
	return r;
}

/* What a lane keeps of its direction: the face and p = sc / ma, q = tc / ma (one binary64 division each, |p|, |q| <= 1). */
struct CubeAt { double p, q; uint32_t face; };

/* The face coordinate of a level of s texels: x = p h + h with h = s * 0.5 (exact), one product and then one sum; in [0, s]. */
WV_FN double cube_coordinate(double p, uint32_t s)
{
	const double h = (double)s * 0.5;
	const double ph = p * h;
	return ph + h;
}

/* The taps of a cleared point at (x, y) of face `face` of cube `cube` of the level `img` (s x s texels, x and y in [0, s]):
 * weights, blocks, texels and the pending bits, every tap with the layer the "Cube edges" rule gives it (mip_cube_source).
 * NEAREST: the texel (min(floor(x), s - 1), min(floor(y), s - 1)).  BILINEAR: sample_axis on x and on y, indices in [-1, s]. */
__attribute__((always_inline)) WV_FN void cube_point_taps(SamplePoint& P, const DecodeImage& img, uint32_t cube, uint32_t filter, uint32_t face, double x, double y)
{
	const uint32_t s = img.dim_x, block_x = img.block_x, block_y = img.block_y;
	SampleAxis ax = sample_axis(filter, x), ay = sample_axis(filter, y);
	if (filter == 0u)
	{
		ax.i0 = ax.i0 < (int32_t)s - 1 ? ax.i0 : (int32_t)s - 1;
		ay.i0 = ay.i0 < (int32_t)s - 1 ? ay.i0 : (int32_t)s - 1;
	}
	P.nx = ax.n; P.ny = ay.n;
	P.wx[0] = ax.w0; P.wx[1] = ax.w1; P.wy[0] = ay.w0; P.wy[1] = ay.w1;
#if WV_DEVICE
	#pragma unroll
#endif
	for (int t = 0; t < SAMPLE_TAPS; t++)
	{
		// (a tap of weight zero is not there: its block is not read)
		if ((uint32_t)(t & 1) >= ax.n || (uint32_t)(t >> 1) >= ay.n) continue;
		const MipCubeTexel src = mip_cube_source(face, (long long)(ax.i0 + (t & 1)), (long long)(ay.i0 + (t >> 1)), s);
		const uint32_t bx = src.x / block_x, by = src.y / block_y;
		P.blk[t] = ((6u * cube + src.face) * img.blocks_y + by) * img.blocks_x + bx;
		P.txy[t] = (src.x - bx * block_x) | ((src.y - by * block_y) << 8);
		P.pending |= 1u << t;
	}
}

/* How the cube call's lanes read a point and form its taps in a level (lod_walk_tile's Points). */
struct CubePoints {
	typedef CubeAt At;
	typedef SamplePoint Point;
	WV_FN static At none() { const At a = { 0.0, 0.0, 0xFFFFFFFFu }; return a; }
	/* (an invalid direction comes back with the face 0xFFFFFFFF) */
	WV_FN static At read(const DecodeCubeRecord& rec, uint32_t i, uint32_t j)
	{
		// (three floats are not 8-byte aligned: three dwords)
		const float* d = rec.dirs + (size_t)j * rec.dir_row + 3u * (size_t)i;
		const float dx = d[0], dy = d[1], dz = d[2];
		At a = none();
		if (cube_valid(dx, dy, dz, 0.0f))
		{
			const CubeFace f = cube_face(dx, dy, dz);
			a.face = f.face;
			a.p = (double)f.sc / (double)f.ma;
			a.q = (double)f.tc / (double)f.ma;
		}
		return a;
	}
	WV_FN static bool valid(const At& a, float lambda) { return a.face != 0xFFFFFFFFu && lambda == lambda; }
	__attribute__((always_inline)) WV_FN static void taps(SamplePoint& P, const DecodeCubeRecord& rec, const DecodeLodLevel& lv, const At& a)
	{
		cube_point_taps(P, lv.img, rec.cube, rec.filter, a.face, cube_coordinate(a.p, lv.img.dim_x), cube_coordinate(a.q, lv.img.dim_x));
	}
};

/* Tile `local` of the grid of `rec` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's; level(l) as
 * in decode_lod_tile. */
template <uint32_t kType, uint32_t kLayout, class LevelOf>
WV_FN LodTileCount decode_cube_tile(const DecodeCubeRecord& rec, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	return lod_walk_tile<kType, kLayout, CubePoints>(rec, level, local, batch, tile);
}

} } // namespace astcd::ASTC_VARIANT
