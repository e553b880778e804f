// SPDX-License-Identifier: Apache-2.0
// Compressed volumes sampled at (u, v, w) at a level of detail per point (astcenc_amd_sample_volume_tensors_device): for every
// point of a grid of normalised triples and a lambda of its own, the sample of one level (MIP_NEAREST) or the blend of two
// (MIP_LINEAR), each level sampled with the nearest texel or the trilinear blend of eight under an address mode per axis
// (include/astcenc_amd.h has the definition, tests/sample_volume_model.py spells it out in numpy).
//
// The work item, the level walk, the blend, the stores (lod_walk_tile) and the table writer (decode_lod_table_build; the launch is
// the lod call's DecodeLodLaunch, its z unused) are decode_lod.h's; this header holds what differs: the
// record, the eight-tap point, its taps -- (block, tx | ty << 8 | tz << 16), the block counted through layers of block_z slices,
// one division per axis tap -- the batch loop over eight slots, which hands block_z and tz to decode_batch_texel, and the sums
// (x taps, then y taps, then z taps).  A level pass may list 64 * 8 = 512 distinct blocks, 16 full batches; with a 3D footprint
// the taps of a point that share a block are decoded once, which is why the eight taps go through one pass and not two slices.
// The four-tap routines of decode_sample.h are not touched: the routines here are overloads on the point's type, and the per-tap
// arrays are indexed by constants only (the select pattern of sample_batches), so the point stays in registers.
//
// Included by kernel_decode_volume.hip and tests/harness/decode_volume_check.cpp only: not part of wave_decode.h's include graph.
//
// Layout: decode_lod.h's -- ImageSetTable, first[count], padding, DecodeVolumeRecord[count], then the DecodeLodLevel records of
// grid 0's levels, of grid 1's ...
#pragma once
#include "decode_lod.h"

namespace astcd { inline namespace ASTC_VARIANT {

constexpr int VOLUME_TAPS = 8;                 // taps of a point, at most: slot = z tap * 4 + y tap * 2 + x tap
constexpr int VOLUME_TILE_BLOCKS = SAMPLE_POINTS * VOLUME_TAPS;   // distinct blocks a level pass can list

struct DecodeVolumeRecord {
	const float* coords;              // point (i, j): coords[j * coord_row + 3 i], u, v, w
	size_t   coord_row;               // floats from row to row of points
	const float* lod;                 // point (i, j): lod[j * lod_row + i]; null: +0.0 everywhere
	size_t   lod_row;
	void*    out;                     // the grid's `out`
	size_t   row;                     // elements from output row to output row
	size_t   levels;                  // bytes from the table's start to the record of level 0
	uint32_t level_count;             // 1 .. 32
	uint32_t out_x, out_y;
	uint32_t filter, address_x, address_y, address_z, mip_filter;
	uint32_t tw_log2;                 // the tile is (1 << tw_log2) points across and 64 >> tw_log2 down
	uint32_t tiles_x;                 // tiles per row of tiles: ceil(out_x / tw)
	uint32_t x_step;                  // elements from column to column (1 planar, `channels` interleaved)
	float    lod_bias;
	TensorParams fmt;
};
static_assert(sizeof(DecodeVolumeRecord) % 8 == 0, "records are read word by word and hold pointers");

inline size_t decode_volume_bytes(const DecodeLodLaunch* grids, uint32_t count) { return decode_lod_table_bytes<DecodeVolumeRecord>(grids, count); }

/* The volume call's table (decode_lod_table_build; any footprint): its own are the triples and three address modes. */
inline uint32_t decode_volume_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                    const DecodeLodLaunch* grids, uint32_t count)
{
	return decode_lod_table_build<DecodeVolumeRecord>(out, images, streams, format, sampler, grids, count, [&](DecodeVolumeRecord& r, const DecodeLodLaunch& g) -> DecodeVolumeRecord&
	{
		r.coords = g.d_coords;
		r.coord_row = g.coord_row_pitch;
		r.address_x = sampler.address_x; r.address_y = sampler.address_y; r.address_z = sampler.address_z;
		return r;
	});
}

/* A point is valid when u, v and w are finite and no larger than 2^14 in magnitude and lambda' is not a NaN. */
WV_FN bool volume_valid(float u, float v, float w, float lambda)
{
	// (a NaN fails every comparison)
	return lod_valid(u, v, lambda) && w >= -16384.0f && w <= 16384.0f;
}

/* What a lane keeps of its point in a level. */
struct VolumePoint {
	uint32_t blk[VOLUME_TAPS];        // the tap's block, counted from the stream's start
	uint32_t txyz[VOLUME_TAPS];       // its texel in the block: tx | ty << 8 | tz << 16
	float    v[VOLUME_TAPS][4];       // its texel, what the entry's data type would have stored, as binary32 (+0.0: a BORDER tap outside)
	double   wx[2], wy[2], wz[2];
	uint32_t nx, ny, nz;
	uint32_t pending;                 // bit per tap slot: not decoded yet
	uint32_t live;                    // the lane has a point / the point is valid: bits 0 / 1
};

#if WV_DEVICE
#define VOLUME_POINTS_PARAM VolumePoint& point_regs
#else
#define VOLUME_POINTS_PARAM VolumePoint* point_lanes
#endif

/* A point without taps: nothing pending, every texel +0.0. */
__attribute__((always_inline)) WV_FN void sample_point_clear(VolumePoint& P)
{
	P.pending = 0u;
	P.nx = 0u; P.ny = 0u; P.nz = 0u;
	P.wx[0] = 0.0; P.wx[1] = 0.0; P.wy[0] = 0.0; P.wy[1] = 0.0; P.wz[0] = 0.0; P.wz[1] = 0.0;
	for (int t = 0; t < VOLUME_TAPS; t++)
	{
		P.blk[t] = 0xFFFFFFFFu; P.txyz[t] = 0u;
		for (int c = 0; c < 4; c++) P.v[t][c] = 0.0f;
	}
}

/* The taps of one axis of S texels in blocks of `block`: the addressed index of tap a (0xFFFFFFFF: not there -- the second of an
 * axis with one, a BORDER tap outside), its block along the axis and its texel in the block.  One division per axis tap. */
struct VolumeAxisTaps { uint32_t k[2], b[2], t[2]; };

__attribute__((always_inline)) WV_FN VolumeAxisTaps volume_axis_taps(const SampleAxis& ax, uint32_t mode, uint32_t S, uint32_t block)
{
	VolumeAxisTaps r;
	for (int a = 0; a < 2; a++)
	{
		uint32_t k = 0u;
		r.k[a] = 0xFFFFFFFFu;
		if ((uint32_t)a < ax.n) r.k[a] = sample_address(mode, ax.i0 + a, S, k) ? k : 0xFFFFFFFFu;
		// (the quotient of a tap that is not there is not used)
		r.b[a] = r.k[a] / block;
		r.t[a] = r.k[a] - r.b[a] * block;
	}
	return r;
}

/* The taps of a cleared point at (x, y, z), binary64 in texel units of `img`, |x|, |y|, |z| <= 2^30: weights, blocks, texels and
 * the pending bits. */
__attribute__((always_inline)) WV_FN void volume_point_taps(VolumePoint& P, const DecodeImage& img, uint32_t filter, uint32_t address_x, uint32_t address_y,
                                                            uint32_t address_z, double x, double y, double z)
{
	const SampleAxis ax = sample_axis(filter, x), ay = sample_axis(filter, y), az = sample_axis(filter, z);
	P.nx = ax.n; P.ny = ay.n; P.nz = az.n;
	P.wx[0] = ax.w0; P.wx[1] = ax.w1; P.wy[0] = ay.w0; P.wy[1] = ay.w1; P.wz[0] = az.w0; P.wz[1] = az.w1;
	const VolumeAxisTaps tx = volume_axis_taps(ax, address_x, img.dim_x, img.block_x);
	const VolumeAxisTaps ty = volume_axis_taps(ay, address_y, img.dim_y, img.block_y);
	const VolumeAxisTaps tz = volume_axis_taps(az, address_z, img.dim_z, img.block_z);
#if WV_DEVICE
	#pragma unroll
#endif
	for (int t = 0; t < VOLUME_TAPS; t++)
	{
		const int a = t & 1, b = (t >> 1) & 1, c = t >> 2;
		if (tx.k[a] == 0xFFFFFFFFu || ty.k[b] == 0xFFFFFFFFu || tz.k[c] == 0xFFFFFFFFu) continue;
		P.blk[t] = (tz.b[c] * img.blocks_y + ty.b[b]) * img.blocks_x + tx.b[a];
		P.txyz[t] = tx.t[a] | (ty.t[b] << 8) | (tz.t[c] << 16);
		P.pending |= 1u << t;
	}
}

/* sample_batches over eight slots: batches of distinct blocks of `img` (stream `blocks`) until no tap of the wave's points is
 * pending (all 64 lanes call this); `done` counts on. */
__attribute__((always_inline)) WV_FN void sample_batches(const DecodeImage& img, const uint8_t* blocks, DecodeBatch& batch, SampleTile& tile, VOLUME_POINTS_PARAM,
                                                         SampleTileCount& done)
{
	const bool small_block = img.block_x * img.block_y * img.block_z < 31u;
	const uint32_t swz_sel = swizzle_selector(img.swz);
	const int block_z = (int)img.block_z;
#if !WV_DEVICE
	uint32_t listed_blocks = 0u;
#endif
	for (;;)
	{
		// 1. the smallest pending block indices, ascending: a wave minimum a slot
		uint32_t lower = 0u;
		int count = 0;
		for (; count < DECODE_BATCH; count++)
		{
			uint32_t m = 0xFFFFFFFFu;
			WV_FOR64(l, 64)
			{
				const VolumePoint& P = SAMPLE_POINT(l);
#if WV_DEVICE
				#pragma unroll
#endif
				for (int t = 0; t < VOLUME_TAPS; t++)
					if (((P.pending >> t) & 1u) != 0u && P.blk[t] >= lower && P.blk[t] < m) m = P.blk[t];
			}
			m = sample_all_umin(m);
			if (m == 0xFFFFFFFFu) break;
			WV_ONE tile.list[count] = m;
			lower = m + 1u;
		}
		if (count == 0) break;
		WV_SYNC();
#if !WV_DEVICE
		// (the points of a tile reference at most 512 blocks of a level: sixteen full batches)
		listed_blocks += (uint32_t)count;
		if (listed_blocks > (uint32_t)VOLUME_TILE_BLOCKS) __builtin_trap();
#endif
		// 2. the decoder's phases over the list
		const SampleBlocks listed = { tile.list };
		(void)decode_batch_blocks(img, blocks, listed, count, batch);
		// 3. the taps that landed in the batch: those whose block is below `lower`
		WV_FOR64(l, 64)
		{
			VolumePoint& P = SAMPLE_POINT(l);
			// (one copy of the texel body, the slot picked and the result put back with selects: decode_sample.h's pattern)
#if WV_DEVICE
			#pragma clang loop unroll(disable)
#endif
			for (uint32_t t = 0; t < (uint32_t)VOLUME_TAPS; t++)
			{
				const uint32_t b = t == 0u ? P.blk[0] : t == 1u ? P.blk[1] : t == 2u ? P.blk[2] : t == 3u ? P.blk[3] :
				                   t == 4u ? P.blk[4] : t == 5u ? P.blk[5] : t == 6u ? P.blk[6] : P.blk[7];
				const uint32_t txyz = t == 0u ? P.txyz[0] : t == 1u ? P.txyz[1] : t == 2u ? P.txyz[2] : t == 3u ? P.txyz[3] :
				                      t == 4u ? P.txyz[4] : t == 5u ? P.txyz[5] : t == 6u ? P.txyz[6] : P.txyz[7];
				if (((P.pending >> t) & 1u) == 0u || b >= lower) continue;
				// (the list is ascending: the largest slot whose block is not above the tap's)
				int k = 0;
				for (int step = DECODE_BATCH >> 1; step > 0; step >>= 1)
					if (k + step < count && tile.list[k + step] <= b) k += step;
#if !WV_DEVICE
				if (tile.list[k] != b) __builtin_trap();
#endif
				SampleSink sink;
				decode_batch_texel(img, batch, k, block_z, (int)(txyz & 0xFFu), (int)((txyz >> 8) & 0xFFu), (int)(txyz >> 16), small_block, swz_sel, (size_t)0, sink, l);
				for (int c = 0; c < 4; c++)
				{
					P.v[0][c] = t == 0u ? sink.s[c] : P.v[0][c];
					P.v[1][c] = t == 1u ? sink.s[c] : P.v[1][c];
					P.v[2][c] = t == 2u ? sink.s[c] : P.v[2][c];
					P.v[3][c] = t == 3u ? sink.s[c] : P.v[3][c];
					P.v[4][c] = t == 4u ? sink.s[c] : P.v[4][c];
					P.v[5][c] = t == 5u ? sink.s[c] : P.v[5][c];
					P.v[6][c] = t == 6u ? sink.s[c] : P.v[6][c];
					P.v[7][c] = t == 7u ? sink.s[c] : P.v[7][c];
				}
				P.pending &= ~(1u << t);
			}
		}
		WV_SYNC();          // the batch scratch and the list are reused by the next turn
		done.batches++;
		done.blocks += (uint32_t)count;
	}
}

/* The sums of a point whose taps are decoded, in the defined order -- rows, planes, then the z taps -- one rounding. */
__attribute__((always_inline)) WV_FN void sample_point_sums(const VolumePoint& P, float s[4])
{
	for (int c = 0; c < 4; c++)
	{
		double p[2] = { 0.0, 0.0 };
#if WV_DEVICE
		#pragma unroll
#endif
		for (int kz = 0; kz < 2; kz++)
		{
			if (kz == 1 && P.nz <= 1u) continue;
			double r0 = P.wx[0] * (double)P.v[4 * kz][c];
			if (P.nx > 1u) r0 = r0 + P.wx[1] * (double)P.v[4 * kz + 1][c];
			double q = P.wy[0] * r0;
			if (P.ny > 1u)
			{
				double r1 = P.wx[0] * (double)P.v[4 * kz + 2][c];
				if (P.nx > 1u) r1 = r1 + P.wx[1] * (double)P.v[4 * kz + 3][c];
				q = q + P.wy[1] * r1;
			}
			p[kz] = q;
		}
		double acc = P.wz[0] * p[0];
		if (P.nz > 1u) acc = acc + P.wz[1] * p[1];
		s[c] = (float)acc;
	}
}

/* How the volume call's lanes read a point and form its taps in a level (lod_walk_tile's Points): the triple (u, v, w), valid
 * within 2^14, sampled at (u W_l, v H_l, w D_l) under the record's address modes. */
struct VolumeUVW { float u, v, w; };

struct VolumePoints {
	typedef VolumeUVW At;
	typedef VolumePoint Point;
	WV_FN static At none() { const At a = { 0.0f, 0.0f, 0.0f }; return a; }
	WV_FN static At read(const DecodeVolumeRecord& rec, uint32_t i, uint32_t j)
	{
		// (three floats are not 8-byte aligned: three dwords)
		const float* p = rec.coords + (size_t)j * rec.coord_row + 3u * (size_t)i;
		const At a = { p[0], p[1], p[2] };
		return a;
	}
	WV_FN static bool valid(const At& a, float lambda) { return volume_valid(a.u, a.v, a.w, lambda); }
	__attribute__((always_inline)) WV_FN static void taps(VolumePoint& P, const DecodeVolumeRecord& rec, const DecodeLodLevel& lv, const At& a)
	{
		// (exact products: 24 bits by 17)
		volume_point_taps(P, lv.img, rec.filter, rec.address_x, rec.address_y, rec.address_z, (double)a.u * (double)lv.img.dim_x, (double)a.v * (double)lv.img.dim_y,
		                  (double)a.w * (double)lv.img.dim_z);
	}
};

/* Tile `local` of the grid of `rec` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's; level(l) as
 * in decode_lod_tile. */
template <uint32_t kType, uint32_t kLayout, class LevelOf>
WV_FN LodTileCount decode_volume_tile(const DecodeVolumeRecord& rec, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	return lod_walk_tile<kType, kLayout, VolumePoints>(rec, level, local, batch, tile);
}

} } // namespace astcd::ASTC_VARIANT
