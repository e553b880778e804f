// SPDX-License-Identifier: Apache-2.0
// Compressed images sampled at arbitrary coordinates into tensors (astcenc_amd_sample_tensors_device): for every point of a
// grid of (x, y) pairs the nearest texel or the bilinear blend of four, under an address mode per axis, scaled, shifted and
// stored as the tensors call stores (include/astcenc_amd.h has the definition, tests/sample_model.py spells it out in numpy).
//
// A work item is a tile of tw x th points of one grid, tw * th = 64, the lane is the point: th = min(8, out_y rounded up to a
// power of two), so one row of points is 64 x 1 and five or more rows are 8 x 8.  The points of a tile may lie anywhere in the
// image, in any order.  Every lane forms its taps -- up to four (block, texel x, texel y); a BORDER tap outside the image and a
// tap of weight zero are not among them -- and the wave then repeats until no tap is pending:
//   1. collect: the DECODE_BATCH smallest distinct pending block indices, one wave minimum a slot, into a list in LDS -- so a
//      block that many lanes need is decoded once per tile, and the list is ascending;
//   2. decode_batch_blocks over that list: headers, weights, colour values, endpoints (the decoder's own phases);
//   3. every lane evaluates its taps whose block is in the list (a binary search) with decode_batch_texel; the sink keeps the
//      four components, made what the entry's data type would have stored, in registers: TensorStore's rule.
// After the last batch the lane forms the sums in the defined order (binary64, x taps then y taps, a sum starting as its first
// product), rounds once to binary32 and stores through TensorStore::put.
//
// The taps of a point, the batch loop and the sums are routines of their own (sample_point_taps, sample_batches,
// sample_point_sums): decode_lod.h runs them once per mip level a tile's points need.
//
// Included by kernel_decode_sample.hip, decode_lod.h and the harnesses of tests/harness only: not part of wave_decode.h's
// include graph.
//
// Layout: ImageSetTable (count = grids, total = tiles), first[count], padding, DecodeSampleRecord[count].
#pragma once
#include "decode_tensors.h"

namespace astcd { inline namespace ASTC_VARIANT {

constexpr int SAMPLE_POINTS = 64;              // points of a tile: the lanes of the wave
constexpr int SAMPLE_TAPS = 4;                 // taps of a point, at most: slot = y tap * 2 + x tap
constexpr int SAMPLE_TILE_BLOCKS = SAMPLE_POINTS * SAMPLE_TAPS;   // distinct blocks a tile can reference

struct DecodeSampleRecord {
	DecodeImage img;                  // the entry's image; data = the grid's `out`
	const uint8_t* blocks;
	const float* coords;              // point (i, j): coords[j * coord_row + 2 i], x then y
	size_t   coord_row;               // floats from row to row of points
	size_t   row;                     // elements from output row to output row
	uint32_t z;                       // the slice
	uint32_t out_x, out_y;
	uint32_t filter, address_x, address_y;
	uint32_t tw_log2;                 // the tile is (1 << tw_log2) points across and 64 >> tw_log2 down
	uint32_t tiles_x;                 // tiles per row of tiles: ceil(out_x / tw)
	uint32_t x_step;                  // elements from column to column (1 planar, `channels` interleaved)
	uint32_t pad;
	TensorParams fmt;
};
static_assert(sizeof(DecodeSampleRecord) % 8 == 0, "records are read word by word and hold pointers");

/* The tile of a grid of out_y rows: th = min(8, out_y rounded up to a power of two), tw = 64 / th; returned as log2(tw). */
WV_FN uint32_t decode_sample_tw_log2(uint32_t out_y)
{
	return out_y <= 1u ? 6u : out_y <= 2u ? 5u : out_y <= 4u ? 4u : 3u;
}

inline unsigned long long decode_sample_tiles(uint32_t out_x, uint32_t out_y)
{
	const uint32_t l = decode_sample_tw_log2(out_y), tw = 1u << l, th = 64u >> l;
	return (unsigned long long)((out_x + tw - 1u) / tw) * ((out_y + th - 1u) / th);
}

inline size_t decode_sample_bytes(uint32_t count) { return decode_table_bytes<DecodeSampleRecord>(count); }

/* Writes the table of `count` grids over the images `images` (prepared, 2D footprints, `data` unused) and their streams;
 * returns the tiles of all grids (the caller has made sure they fit 32 bits). */
inline uint32_t decode_sample_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, const DecodeSampler& sampler,
                                    const DecodeSampleLaunch* grids, uint32_t count)
{
	uint32_t* first;
	DecodeSampleRecord* rec = decode_table_begin<DecodeSampleRecord>(out, decode_sample_bytes(count), count, first);
	uint32_t tiles = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeSampleLaunch& g = grids[i];
		DecodeSampleRecord& r = rec[i];
		r.img = images[g.entry];
		r.img.data = g.d_out;
		r.blocks = streams[g.entry];
		r.coords = g.d_coords;
		r.coord_row = g.coord_row_pitch;
		r.row = g.row_pitch;
		r.z = g.z;
		r.out_x = g.out_x; r.out_y = g.out_y;
		r.filter = sampler.filter; r.address_x = sampler.address_x; r.address_y = sampler.address_y;
		r.tw_log2 = decode_sample_tw_log2(g.out_y);
		r.tiles_x = (g.out_x + (1u << r.tw_log2) - 1u) >> r.tw_log2;
		r.x_step = tensor_x_step(format);
		r.fmt = tensor_params(format, g.plane_pitch);
		first[i] = tiles;
		tiles += (uint32_t)decode_sample_tiles(g.out_x, g.out_y);
	}
	return decode_table_finish(out, count, tiles);
}

/* A tap index under an address mode (0 CLAMP, 1 REPEAT, 2 MIRROR, 3 BORDER) along an axis of S texels; |i| <= 2^30 + 1.
 * False: a BORDER tap outside the image.  32-bit unsigned divisions only: a negative index is reflected about -1/2 first
 * (j = -i - 1), which MIRROR wants anyway and REPEAT undoes (i mod S = S - 1 - (j mod S)). */
WV_FN bool sample_address(uint32_t mode, int32_t i, uint32_t S, uint32_t& k)
{
	const bool neg = i < 0;
	const uint32_t j = neg ? (uint32_t)(-(i + 1)) : (uint32_t)i;
	if (mode == 0u)
	{
		k = neg ? 0u : j < S - 1u ? j : S - 1u;
		return true;
	}
	if (mode == 1u)
	{
		const uint32_t m = j % S;
		k = neg ? S - 1u - m : m;
		return true;
	}
	if (mode == 2u)
	{
		// (2 S does not fit 32 bits: then j < S and j mod 2S is j)
		const uint32_t q = S >= 0x80000000u ? j : j % (2u * S);
		k = q < S ? q : 2u * S - 1u - q;
		return true;
	}
	k = j;
	return !neg && j < S;
}

/* The taps of a coordinate along one axis: n of them (1 or 2), their indices before addressing and their binary64 weights. */
struct SampleAxis { int32_t i0; uint32_t n; double w0, w1; };

/* (the coordinate as binary64: the level coordinates of decode_lod.h are products that a binary32 does not hold) */
WV_FN SampleAxis sample_axis(uint32_t filter, double x)
{
	SampleAxis a;
	if (filter == 0u)
	{
		a.i0 = (int32_t)__builtin_floor(x);
		a.n = 1u; a.w0 = 1.0; a.w1 = 0.0;
		return a;
	}
	const double t = x - 0.5;
	const double fl = __builtin_floor(t);
	const double f = t - fl;
	a.i0 = (int32_t)fl;
	a.w0 = 1.0 - f; a.w1 = f;
	a.n = f == 0.0 ? 1u : 2u;
	return a;
}

WV_FN SampleAxis sample_axis(uint32_t filter, float x) { return sample_axis(filter, (double)x); }

/* A point is valid when both coordinates are finite and no larger than 2^30 in magnitude. */
WV_FN bool sample_valid(float x, float y)
{
	// (a NaN fails both comparisons)
	return x >= -1073741824.0f && x <= 1073741824.0f && y >= -1073741824.0f && y <= 1073741824.0f;
}

/* What a lane keeps of its point. */
struct SamplePoint {
	uint32_t blk[SAMPLE_TAPS];        // the tap's block, counted from the stream's start
	uint32_t txy[SAMPLE_TAPS];        // its texel in the block: tx | ty << 8
	float    v[SAMPLE_TAPS][4];       // its texel, what the entry's data type would have stored, as binary32 (+0.0: a BORDER tap outside)
	double   wx[2], wy[2];
	uint32_t nx, ny;
	uint32_t pending;                 // bit per tap slot: not decoded yet
	uint32_t live;                    // the lane has a point / the point is valid: bits 0 / 1
};

#if WV_DEVICE
#define SAMPLE_POINTS_DECL SamplePoint point_regs
#define SAMPLE_POINTS_PARAM SamplePoint& point_regs
#define SAMPLE_POINTS_ARG point_regs
#define SAMPLE_POINT(l) point_regs
#else
#define SAMPLE_POINTS_DECL SamplePoint point_lanes[SAMPLE_POINTS]
#define SAMPLE_POINTS_PARAM SamplePoint* point_lanes
#define SAMPLE_POINTS_ARG point_lanes
#define SAMPLE_POINT(l) point_lanes[l]
#endif

/* Per-wave scratch next to DecodeBatch (LDS): the blocks of the batch, ascending. */
struct alignas(16) SampleTile {
	uint32_t list[DECODE_BATCH];
};

/* The batch's blocks for decode_batch_blocks. */
struct SampleBlocks {
	const uint32_t* list;
	WV_FN size_t operator()(int k) const { return (size_t)list[k]; }
};

/* The sink: the texel in whichever form it leaves the decoder becomes s[0 .. 3], the regions call's texel as binary32
 * (decode_tensors.h: what TensorStore stores, kept). */
struct SampleSink {
	float s[4];
	WV_FN void pixel(const DecodeImage&, int, size_t, uint32_t px) { tensor_from_pixel(px, s); }
	WV_FN void halves(const DecodeImage&, int, size_t, uint64_t px) { tensor_from_halves(px, s); }
	WV_FN void texel(const DecodeImage& img, int, size_t, float r, float g, float b, float a)
	{
		if (img.data_type == 0)
		{
			tensor_from_pixel(pack_texel_u8(img, r, g, b, a), s);
			return;
		}
		float src[7];
		swizzle_sources(r, g, b, a, src);
		for (int c = 0; c < 4; c++) s[c] = tensor_from_source(img, src, c);
	}
	WV_FN void trip_end(int, int, int) {}
};

/* The minimum over the wave of per-lane partials (the usage of wv_all_imax). */
WV_FN uint32_t sample_all_umin(uint32_t v)
{
#if WV_DEVICE
	asm volatile("s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n s_nop 1\n"
	    "v_min_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n s_nop 1\n"
	    : "+v"(v));
	return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
#else
	return v;
#endif
}

/* What a tile did, for the harness (`blocks` mode, the batch checks): batches run and blocks decoded. */
struct SampleTileCount { uint32_t batches, blocks; };

/* A point without taps: nothing pending, every texel +0.0. */
__attribute__((always_inline)) WV_FN void sample_point_clear(SamplePoint& P)
{
	P.pending = 0u;
	P.nx = 0u; P.ny = 0u;
	P.wx[0] = 0.0; P.wx[1] = 0.0; P.wy[0] = 0.0; P.wy[1] = 0.0;
	for (int t = 0; t < SAMPLE_TAPS; t++)
	{
		P.blk[t] = 0xFFFFFFFFu; P.txy[t] = 0u;
		for (int c = 0; c < 4; c++) P.v[t][c] = 0.0f;
	}
}

/* The taps of a cleared point at (x, y), binary64 in texel units of slice z of `img`, |x|, |y| <= 2^30: weights, blocks, texels
 * and the pending bits. */
__attribute__((always_inline)) WV_FN void sample_point_taps(SamplePoint& P, const DecodeImage& img, uint32_t z, uint32_t filter, uint32_t address_x, uint32_t address_y,
                                                            double x, double y)
{
	const uint32_t block_x = img.block_x, block_y = img.block_y;
	const SampleAxis ax = sample_axis(filter, x), ay = sample_axis(filter, y);
	P.nx = ax.n; P.ny = ay.n;
	P.wx[0] = ax.w0; P.wx[1] = ax.w1; P.wy[0] = ay.w0; P.wy[1] = ay.w1;
	// (a tap that is not there -- the second of an axis with one, a BORDER tap outside -- has no index: an index is at most
	//  2^30 + 1.  The flag travels in the integer, not as a boolean across the address modes' branches.)
	uint32_t kx[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu }, ky[2] = { 0xFFFFFFFFu, 0xFFFFFFFFu };
	for (int a = 0; a < 2; a++)
	{
		uint32_t k = 0u;
		if ((uint32_t)a < ax.n) kx[a] = sample_address(address_x, ax.i0 + a, img.dim_x, k) ? k : 0xFFFFFFFFu;
		if ((uint32_t)a < ay.n) ky[a] = sample_address(address_y, ay.i0 + a, img.dim_y, k) ? k : 0xFFFFFFFFu;
	}
	// (one division per axis tap, not per tap; the quotient of a tap that is not there is not used)
	const uint32_t bx[2] = { kx[0] / block_x, kx[1] / block_x }, by[2] = { ky[0] / block_y, ky[1] / block_y };
#if WV_DEVICE
	#pragma unroll
#endif
	for (int t = 0; t < SAMPLE_TAPS; t++)
	{
		if (kx[t & 1] == 0xFFFFFFFFu || ky[t >> 1] == 0xFFFFFFFFu) continue;
		P.blk[t] = (z * img.blocks_y + by[t >> 1]) * img.blocks_x + bx[t & 1];
		P.txy[t] = (kx[t & 1] - bx[t & 1] * block_x) | ((ky[t >> 1] - by[t >> 1] * block_y) << 8);
		P.pending |= 1u << t;
	}
}

/* Batches of distinct blocks of `img` (stream `blocks`) until no tap of the wave's points is pending (all 64 lanes call this);
 * `done` counts on. */
__attribute__((always_inline)) WV_FN void sample_batches(const DecodeImage& img, const uint8_t* blocks, DecodeBatch& batch, SampleTile& tile, SAMPLE_POINTS_PARAM,
                                                         SampleTileCount& done)
{
	const bool small_block = img.block_x * img.block_y < 31u;
	const uint32_t swz_sel = swizzle_selector(img.swz);
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
				const SamplePoint& P = SAMPLE_POINT(l);
#if WV_DEVICE
				#pragma unroll
#endif
				for (int t = 0; t < SAMPLE_TAPS; t++)
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
		// (the points of a tile reference at most 256 blocks of an image: eight full batches)
		listed_blocks += (uint32_t)count;
		if (listed_blocks > (uint32_t)SAMPLE_TILE_BLOCKS) __builtin_trap();
#endif
		// 2. the decoder's phases over the list
		const SampleBlocks listed = { tile.list };
		(void)decode_batch_blocks(img, blocks, listed, count, batch);
		// 3. the taps that landed in the batch: those whose block is below `lower`
		WV_FOR64(l, 64)
		{
			SamplePoint& P = SAMPLE_POINT(l);
			// (one copy of the texel body: the slot is picked and the result put back with selects, so that on the device the
			//  point's arrays are indexed by constants only and stay in registers)
#if WV_DEVICE
			#pragma clang loop unroll(disable)
#endif
			for (uint32_t t = 0; t < (uint32_t)SAMPLE_TAPS; t++)
			{
				const uint32_t b = t == 0u ? P.blk[0] : t == 1u ? P.blk[1] : t == 2u ? P.blk[2] : P.blk[3];
				const uint32_t txy = t == 0u ? P.txy[0] : t == 1u ? P.txy[1] : t == 2u ? P.txy[2] : P.txy[3];
				if (((P.pending >> t) & 1u) == 0u || b >= lower) continue;
				// (the list is ascending: the largest slot whose block is not above the tap's)
				int k = 0;
				for (int step = DECODE_BATCH >> 1; step > 0; step >>= 1)
					if (k + step < count && tile.list[k + step] <= b) k += step;
#if !WV_DEVICE
				if (tile.list[k] != b) __builtin_trap();
#endif
				SampleSink sink;
				decode_batch_texel(img, batch, k, 1, (int)(txy & 0xFFu), (int)(txy >> 8), 0, small_block, swz_sel, (size_t)0, sink, l);
				for (int c = 0; c < 4; c++)
				{
					P.v[0][c] = t == 0u ? sink.s[c] : P.v[0][c];
					P.v[1][c] = t == 1u ? sink.s[c] : P.v[1][c];
					P.v[2][c] = t == 2u ? sink.s[c] : P.v[2][c];
					P.v[3][c] = t == 3u ? sink.s[c] : P.v[3][c];
				}
				P.pending &= ~(1u << t);
			}
		}
		WV_SYNC();          // the batch scratch and the list are reused by the next turn
		done.batches++;
		done.blocks += (uint32_t)count;
	}
}

/* The sums of a point whose taps are decoded, in the defined order, one rounding. */
__attribute__((always_inline)) WV_FN void sample_point_sums(const SamplePoint& P, float s[4])
{
	for (int c = 0; c < 4; c++)
	{
		double r0 = P.wx[0] * (double)P.v[0][c];
		if (P.nx > 1u) r0 = r0 + P.wx[1] * (double)P.v[1][c];
		double acc = P.wy[0] * r0;
		if (P.ny > 1u)
		{
			double r1 = P.wx[0] * (double)P.v[2][c];
			if (P.nx > 1u) r1 = r1 + P.wx[1] * (double)P.v[3][c];
			acc = acc + P.wy[1] * r1;
		}
		s[c] = (float)acc;
	}
}

/* Tile `local` of the grid of `rec` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's. */
template <uint32_t kType, uint32_t kLayout>
WV_FN SampleTileCount decode_sample_tile(const DecodeSampleRecord& rec, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	const uint32_t tw_log2 = rec.tw_log2, tw_mask = (1u << tw_log2) - 1u, th_log2 = 6u - tw_log2;
	const uint32_t tile_y = local / rec.tiles_x, tile_x = local - tile_y * rec.tiles_x;
	const uint32_t i0 = tile_x << tw_log2, j0 = tile_y << th_log2;
	SAMPLE_POINTS_DECL;

	// ---- the taps of every point ----
	WV_FOR64(l, 64)
	{
		SamplePoint& P = SAMPLE_POINT(l);
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		P.live = i < rec.out_x && j < rec.out_y ? 1u : 0u;
		sample_point_clear(P);
		if (P.live)
		{
			// (coords is aligned to 8 bytes and the pitch is even: one 8-byte load)
			const float* xy = static_cast<const float*>(__builtin_assume_aligned(rec.coords + (size_t)j * rec.coord_row + 2u * (size_t)i, 8));
			const float x = xy[0], y = xy[1];
			if (sample_valid(x, y))
			{
				P.live = 3u;
				sample_point_taps(P, rec.img, rec.z, rec.filter, rec.address_x, rec.address_y, (double)x, (double)y);
			}
		}
	}

	// ---- batches of distinct blocks until no tap is pending ----
	SampleTileCount done = { 0u, 0u };
	sample_batches(rec.img, rec.blocks, batch, tile, SAMPLE_POINTS_ARG, done);

	// ---- the sums in the defined order, one rounding, the tensors call's arithmetic and stores ----
	TensorStore<kType, kLayout> store = { rec.fmt };
	WV_FOR64(l, 64)
	{
		const SamplePoint& P = SAMPLE_POINT(l);
		if (!(P.live & 1u)) continue;
		const uint32_t i = i0 + ((uint32_t)l & tw_mask), j = j0 + ((uint32_t)l >> tw_log2);
		float s[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
		if (P.live & 2u) sample_point_sums(P, s);
		store.template put<false>(rec.img, (size_t)j * rec.row + (size_t)i * rec.x_step, s);
	}
	WV_SYNC();
	return done;
}

} } // namespace astcd::ASTC_VARIANT
