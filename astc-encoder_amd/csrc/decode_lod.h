// SPDX-License-Identifier: Apache-2.0
// Compressed mip chains sampled at a level of detail per point (astcenc_amd_sample_lod_tensors_device): for every point of a grid
// of normalised (u, v) pairs and a lambda of its own, the sample of one level (MIP_NEAREST) or the blend of the samples of two
// neighbouring levels (MIP_LINEAR: trilinear filtering), each level sampled as astcenc_amd_sample_tensors_device samples an
// entry (include/astcenc_amd.h has the definition, tests/sample_lod_model.py spells it out in numpy).
//
// A work item is a tile of 64 points of one grid, the tiles of decode_sample.h; the lane is the point.  Every lane forms its one
// or two (level, weight) pairs; the wave then walks the distinct levels its lanes still need in ascending order -- a wave minimum
// a pass -- and a level pass is decode_sample.h's pipeline run with that level's image and stream for the lanes that have the
// level: the taps from (u W_l, v H_l), sample_batches, the sums rounded to binary32 into the lane's slot for that level (a lane
// has a level as its l0 or as its l1, never both).  After the last pass the lane blends (binary64, two products and a sum, one
// rounding) and stores through TensorStore::put.  A level of weight zero is not among a lane's levels: none of its blocks is read.
//
// The level walk (lod_walk_tile) takes how a lane reads its point and forms its taps in a level as a parameter: decode_cube.h runs
// it over directions and cube faces, decode_volume.h over triples and eight taps.  The table writer (decode_lod_table_build) is
// likewise one for the lod call, its gradient, the cube call and the volume call: it takes the record's type and a callable for the
// few fields that are a call's own.
//
// Included by kernel_decode_lod.hip, decode_cube.h, decode_volume.h, decode_lod_grad.h and tests/harness/decode_lod_check.cpp only.
//
// Layout: ImageSetTable (count = grids, total = tiles), first[count], padding, DecodeLodRecord[count], then the DecodeLodLevel
// records of grid 0's levels, of grid 1's ...; a grid's record holds the byte offset of its first level record from the table's start.
#pragma once
#include "decode_sample.h"

namespace astcd { inline namespace ASTC_VARIANT {

constexpr uint32_t LOD_MAX_LEVELS = 32;
constexpr uint32_t LOD_NO_LEVEL = 0xFFFFFFFFu;

struct DecodeLodRecord {
	const float* coords;              // point (i, j): coords[j * coord_row + 2 i], u then v
	size_t   coord_row;               // floats from row to row of points
	const float* lod;                 // point (i, j): lod[j * lod_row + i]; null: +0.0 everywhere
	size_t   lod_row;
	void*    out;                     // the grid's `out`
	size_t   row;                     // elements from output row to output row
	size_t   levels;                  // bytes from the table's start to the record of level 0
	uint32_t level_count;             // 1 .. 32
	uint32_t z;                       // the slice, in every level
	uint32_t out_x, out_y;
	uint32_t filter, address_x, address_y, mip_filter;
	uint32_t tw_log2;                 // the tile is (1 << tw_log2) points across and 64 >> tw_log2 down
	uint32_t tiles_x;                 // tiles per row of tiles: ceil(out_x / tw)
	uint32_t x_step;                  // elements from column to column (1 planar, `channels` interleaved)
	float    lod_bias;
	TensorParams fmt;
};
static_assert(sizeof(DecodeLodRecord) % 8 == 0, "records are read word by word and hold pointers");

struct DecodeLodLevel {
	DecodeImage img;                  // the level's image; `data` unused
	const uint8_t* blocks;
};
static_assert(sizeof(DecodeLodLevel) % 8 == 0, "records are read word by word and hold pointers");

/* The table writer of every call of this family (the lod call below, decode_lod_grad.h, decode_cube.h, decode_volume.h), which
 * differ in their records: Record is the call's, Grid its launch -- a DecodeLodLaunch, or the gradient's, which embeds one
 * (decode_lod_launch_of, backend.h). */
template <class Record = DecodeLodRecord>
inline size_t decode_lod_levels_offset(uint32_t count)
{
	return decode_table_bytes<Record>(count);
}

template <class Record, class Grid>
inline size_t decode_lod_table_bytes(const Grid* grids, uint32_t count)
{
	size_t levels = 0;
	for (uint32_t i = 0; i < count; i++) levels += decode_lod_launch_of(grids[i]).level_count;
	return decode_lod_levels_offset<Record>(count) + levels * sizeof(DecodeLodLevel);
}

/* Writes the table of `count` grids over the images `images` (prepared, `data` unused) and their streams: the frame, the level
 * records, first[] and the tile count; returns the tiles of all grids (the caller has made sure they fit 32 bits).
 * own(record, grid) fills what is the call's own -- the points and their pitch, the slice or the cube, the address modes -- and
 * returns the part of the record that holds the fields every call has under one name, which are filled here. */
template <class Record, class Grid, class Own>
inline uint32_t decode_lod_table_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                       const Grid* grids, uint32_t count, Own own)
{
	uint8_t* t = static_cast<uint8_t*>(out);
	uint32_t* first;
	Record* rec = decode_table_begin<Record>(out, decode_lod_table_bytes<Record>(grids, count), count, first);
	size_t level_at = decode_lod_levels_offset<Record>(count);
	uint32_t tiles = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeLodLaunch& g = decode_lod_launch_of(grids[i]);
		auto& r = own(rec[i], grids[i]);
		r.lod = g.d_lod;
		r.lod_row = g.lod_row_pitch;
		r.out = g.d_out;
		r.row = g.row_pitch;
		r.levels = level_at;
		r.level_count = g.level_count;
		r.out_x = g.out_x; r.out_y = g.out_y;
		r.filter = sampler.filter; r.mip_filter = sampler.mip_filter;
		r.tw_log2 = decode_sample_tw_log2(g.out_y);
		r.tiles_x = (g.out_x + (1u << r.tw_log2) - 1u) >> r.tw_log2;
		r.x_step = tensor_x_step(format);
		r.lod_bias = g.lod_bias;
		r.fmt = tensor_params(format, g.plane_pitch);
		for (uint32_t l = 0; l < g.level_count; l++)
		{
			DecodeLodLevel& lv = *reinterpret_cast<DecodeLodLevel*>(t + level_at);
			lv.img = images[g.first_entry + l];
			lv.img.data = nullptr;
			lv.blocks = streams[g.first_entry + l];
			level_at += sizeof(DecodeLodLevel);
		}
		first[i] = tiles;
		tiles += (uint32_t)decode_sample_tiles(g.out_x, g.out_y);
	}
	return decode_table_finish(out, count, tiles);
}

/* What is the lod call's own in a record (its gradient's records begin with one): pairs, the slice, two address modes. */
inline DecodeLodRecord& decode_lod_own(DecodeLodRecord& r, const DecodeLodSampler& sampler, const DecodeLodLaunch& g)
{
	r.coords = g.d_coords;
	r.coord_row = g.coord_row_pitch;
	r.z = g.z;
	r.address_x = sampler.address_x; r.address_y = sampler.address_y;
	return r;
}

inline size_t decode_lod_bytes(const DecodeLodLaunch* grids, uint32_t count) { return decode_lod_table_bytes<DecodeLodRecord>(grids, count); }

/* The lod call's table: 2D footprints. */
inline uint32_t decode_lod_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeLodSampler& sampler,
                                 const DecodeLodLaunch* grids, uint32_t count)
{
	return decode_lod_table_build<DecodeLodRecord>(out, images, streams, format, sampler, grids, count,
		[&](DecodeLodRecord& r, const DecodeLodLaunch& g) -> DecodeLodRecord& { return decode_lod_own(r, sampler, g); });
}

/* A point is valid when u and v are finite and no larger than 2^14 in magnitude and lambda' is not a NaN. */
WV_FN bool lod_valid(float u, float v, float lambda)
{
	// (a NaN fails every comparison)
	return u >= -16384.0f && u <= 16384.0f && v >= -16384.0f && v <= 16384.0f && lambda == lambda;
}

/* The levels of a valid point and the weight of the second: lambda' clamped to [0, level_count - 1]; MIP_NEAREST (0) has one
 * level, ceil(lambda_c + 0.5) - 1; MIP_LINEAR (1) has l0 = floor(lambda_c) and, unless g = lambda_c - l0 is zero, l0 + 1. */
struct LodLevels { uint32_t l0, l1; double g; };

WV_FN LodLevels lod_levels(uint32_t mip_filter, uint32_t level_count, float lambda)
{
	const float top = (float)(level_count - 1u);
	float lc = lambda > 0.0f ? lambda : 0.0f;
	lc = lc < top ? lc : top;
	LodLevels r;
	r.l1 = LOD_NO_LEVEL; r.g = 0.0;
	if (mip_filter == 0u)
	{
		r.l0 = (uint32_t)(__builtin_ceil((double)lc + 0.5) - 1.0);
		return r;
	}
	const float fl = __builtin_floorf(lc);
	r.l0 = (uint32_t)fl;
	r.g = (double)(lc - fl);          // exact
	if (r.g != 0.0) r.l1 = r.l0 + 1u;
	return r;
}

/* What a lane keeps of its point across the level passes; `at` is where the point lies, in the form its call samples a level
 * from (LodUV here, decode_cube.h has a direction's). */
struct LodUV { float u, v; };

template <class At>
struct LodPointOf {
	At       at;
	uint32_t l0, l1;                  // its levels; l1 = LOD_NO_LEVEL: one level
	double   g;                       // the weight of l1
	float    s0[4], s1[4];            // the samples of l0 and l1, binary32
	uint32_t live;                    // the lane has a point / the point is valid: bits 0 / 1
};

#if WV_DEVICE
#define LOD_POINTS_DECL LodPoint lod_regs
#define LOD_POINT(l) lod_regs
#else
#define LOD_POINTS_DECL LodPoint lod_lanes[SAMPLE_POINTS]
#define LOD_POINT(l) lod_lanes[l]
#endif

/* How the lod call's lanes read a point and form its taps in a level (lod_walk_tile's `how`): the pair (u, v), valid within
 * 2^14, sampled at (u W_l, v H_l) of slice z under the record's address modes. */
struct LodUVPoints {
	typedef LodUV At;
	typedef SamplePoint Point;
	WV_FN static At none() { const At a = { 0.0f, 0.0f }; return a; }
	WV_FN static At read(const DecodeLodRecord& rec, uint32_t i, uint32_t j)
	{
		// (coords is aligned to 8 bytes and the pitch is even: one 8-byte load)
		const float* uv = static_cast<const float*>(__builtin_assume_aligned(rec.coords + (size_t)j * rec.coord_row + 2u * (size_t)i, 8));
		const At a = { uv[0], uv[1] };
		return a;
	}
	WV_FN static bool valid(const At& a, float lambda) { return lod_valid(a.u, a.v, lambda); }
	__attribute__((always_inline)) WV_FN static void taps(SamplePoint& P, const DecodeLodRecord& rec, const DecodeLodLevel& lv, const At& a)
	{
		// (exact products: 24 bits by 17)
		sample_point_taps(P, lv.img, rec.z, rec.filter, rec.address_x, rec.address_y, (double)a.u * (double)lv.img.dim_x, (double)a.v * (double)lv.img.dim_y);
	}
};

/* What a tile did, for the harness: level passes, batches run, blocks decoded, the distinct levels as a mask, and whether a
 * point blended two levels / had g = 0 under MIP_LINEAR, and the most blocks one pass decoded. */
struct LodTileCount { uint32_t passes, batches, blocks, level_mask, blended, single, most; };

/* The level walk of a tile, shared with decode_cube.h and decode_volume.h: tile `local` of the grid of `rec` (all 64 lanes call
 * this; `local` is uniform); kType / kLayout are the record's.  level(l): the DecodeLodLevel of the grid's level l, l uniform -- the kernel reads it
 * with scalar loads.  Points: how a lane reads its point (read, valid, none) and forms its taps in a level (taps), and what it
 * keeps of the point in a level (Point: SamplePoint, or decode_volume.h's eight taps, whose sample_point_clear, sample_batches and
 * sample_point_sums are overloads on that type); Rec: its record, with the fields of DecodeLodRecord that are used here. */
template <uint32_t kType, uint32_t kLayout, class Points, class Rec, class LevelOf>
WV_FN LodTileCount lod_walk_tile(const Rec& rec, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	typedef LodPointOf<typename Points::At> LodPoint;
	typedef typename Points::Point Point;
	const uint32_t tw_log2 = rec.tw_log2, tw_mask = (1u << tw_log2) - 1u, th_log2 = 6u - tw_log2;
	const uint32_t tile_y = local / rec.tiles_x, tile_x = local - tile_y * rec.tiles_x;
	const uint32_t i0 = tile_x << tw_log2, j0 = tile_y << th_log2;
#if WV_DEVICE
	Point point_regs;
#else
	Point point_lanes[SAMPLE_POINTS];
#endif
	LOD_POINTS_DECL;
	LodTileCount did = { 0u, 0u, 0u, 0u, 0u, 0u, 0u };

	// ---- the levels of every point ----
	WV_FOR64(l, 64)
	{
		LodPoint& Q = LOD_POINT(l);
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		Q.live = i < rec.out_x && j < rec.out_y ? 1u : 0u;
		Q.at = Points::none();
		Q.l0 = LOD_NO_LEVEL; Q.l1 = LOD_NO_LEVEL; Q.g = 0.0;
		for (int c = 0; c < 4; c++) { Q.s0[c] = 0.0f; Q.s1[c] = 0.0f; }
		if (Q.live)
		{
			const typename Points::At at = Points::read(rec, i, j);
			const float lambda = (rec.lod ? rec.lod[(size_t)j * rec.lod_row + (size_t)i] : 0.0f) + rec.lod_bias;
			if (Points::valid(at, lambda))
			{
				const LodLevels lv = lod_levels(rec.mip_filter, rec.level_count, lambda);
				Q.live = 3u;
				Q.at = at;
				Q.l0 = lv.l0; Q.l1 = lv.l1; Q.g = lv.g;
#if !WV_DEVICE
				if (lv.l0 >= rec.level_count || (lv.l1 != LOD_NO_LEVEL && lv.l1 >= rec.level_count)) __builtin_trap();
				if (rec.mip_filter == 1u) { if (lv.l1 != LOD_NO_LEVEL) did.blended = 1u; else did.single = 1u; }
#endif
			}
		}
	}

	// ---- a pass per distinct level, ascending ----
	SampleTileCount done = { 0u, 0u };
	uint32_t lower = 0u;
	for (;;)
	{
		uint32_t m = LOD_NO_LEVEL;
		WV_FOR64(l, 64)
		{
			const LodPoint& Q = LOD_POINT(l);
			// (l1 is l0 + 1 or none, and none is the largest value)
			const uint32_t next = Q.l0 >= lower ? Q.l0 : Q.l1;
			if (next >= lower && next < m) m = next;
		}
		m = sample_all_umin(m);
		if (m == LOD_NO_LEVEL) break;
		const DecodeLodLevel lv = level(m);
		WV_FOR64(l, 64)
		{
			Point& P = SAMPLE_POINT(l);
			const LodPoint& Q = LOD_POINT(l);
			P.live = Q.live;
			sample_point_clear(P);
			if (Q.l0 == m || Q.l1 == m) Points::taps(P, rec, lv, Q.at);
		}
#if !WV_DEVICE
		const uint32_t blocks_before = done.blocks;
#endif
		sample_batches(lv.img, lv.blocks, batch, tile, SAMPLE_POINTS_ARG, done);
#if !WV_DEVICE
		if (done.blocks - blocks_before > did.most) did.most = done.blocks - blocks_before;
#endif
		WV_FOR64(l, 64)
		{
			const Point& P = SAMPLE_POINT(l);
			LodPoint& Q = LOD_POINT(l);
			if (Q.l0 != m && Q.l1 != m) continue;
			float s[4];
			sample_point_sums(P, s);
			for (int c = 0; c < 4; c++)
			{
				Q.s0[c] = Q.l0 == m ? s[c] : Q.s0[c];
				Q.s1[c] = Q.l0 == m ? Q.s1[c] : s[c];
			}
		}
		lower = m + 1u;
		did.passes++;
		did.level_mask |= 1u << m;
	}
	did.batches = done.batches; did.blocks = done.blocks;

	// ---- the blend, one rounding, the tensors call's arithmetic and stores ----
	TensorStore<kType, kLayout> store = { rec.fmt };
	DecodeImage dst = {};
	dst.data = rec.out;
	WV_FOR64(l, 64)
	{
		const LodPoint& Q = LOD_POINT(l);
		if (!(Q.live & 1u)) continue;
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		float s[4];
		// (an invalid point has kept its +0.0)
		for (int c = 0; c < 4; c++) s[c] = Q.s0[c];
		if (Q.l1 != LOD_NO_LEVEL)
		{
			const double w0 = 1.0 - Q.g;
			for (int c = 0; c < 4; c++)
			{
				const double p0 = w0 * (double)Q.s0[c], p1 = Q.g * (double)Q.s1[c];
				s[c] = (float)(p0 + p1);
			}
		}
		store.template put<false>(dst, (size_t)j * rec.row + (size_t)i * rec.x_step, s);
	}
	WV_SYNC();
	return did;
}

/* The lod call's tile. */
template <uint32_t kType, uint32_t kLayout, class LevelOf>
WV_FN LodTileCount decode_lod_tile(const DecodeLodRecord& rec, const LevelOf level, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	return lod_walk_tile<kType, kLayout, LodUVPoints>(rec, level, local, batch, tile);
}

} } // namespace astcd::ASTC_VARIANT
