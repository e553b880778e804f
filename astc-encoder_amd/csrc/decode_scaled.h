// SPDX-License-Identifier: Apache-2.0
// Scaled windows of compressed images decoded into tensors (astcenc_amd_decompress_scaled_tensors_device): a window of S_x x S_y
// texels becomes D_x x D_y tensor elements per channel through a bilinear or a box filter whose taps are exact rationals formed
// from (S, D, position) by integer arithmetic (include/astcenc_amd.h has the definition, tests/scaled_model.py spells it out in
// numpy).  No tap tables: the table holds one record per region.
//
// A work item is a tile of one region's output: up to SCALED_COLS output columns (lane = column) by up to SCALED_BAND output
// rows.  The wave walks the block rows the tile's y taps reach, top to bottom; a block row's covered blocks are decoded in runs
// (decode_row_batch, unchanged) through two policies: ScaledStage writes a texel into an LDS staging tile in the entry's data
// type, ScaledWindow is a DecodeWindow clipped to the rectangle the tile needs whose `at` is the index in that tile.  After each
// run every lane continues its column's tap sum of every staged source row (x pass); with the block row's last run -- the host
// sizes the tiles so that it is the only one wherever it can, decode_scaled_tiling -- the sum is complete and is added, weighted,
// to the output rows whose y taps hold the source row (y pass: the band's sums live in registers); after the last block row
// the sums are divided, converted and stored through TensorStore::put -- the two roundings, the NaNs and the stores of the
// tensors call.
//
// All sums are binary64, taps in increasing order, a sum starting as its first product: the sequence of operations of a sum
// does not depend on where run or block-row boundaries fall.  U8 entries take the same path: their sums are integers below
// 2^42, exact in binary64, so the sum is the integer N of the definition.
//
// Included by kernel_decode_scaled.hip and tests/harness/decode_scaled_check.cpp only: not part of wave_decode.h's include graph.
//
// Layout: ImageSetTable (count = regions, total = tiles), first[count], padding, DecodeScaledRecord[count].
#pragma once
#include "decode_tensors.h"

namespace astcd { inline namespace ASTC_VARIANT {

constexpr int SCALED_COLS = 64;                // output columns of a tile
constexpr int SCALED_BAND = 8;                 // output rows of a tile, at most
constexpr int SCALED_ROWS = 12;                // texel rows of a block row, at most (2D footprints)
constexpr int SCALED_STAGE_BYTES = 6144;       // the staging tile: 1536 U8, 768 F16 or 384 F32 texels
constexpr int SCALED_CARRY = 8;                // output columns of a tile whose source columns may span several decoded runs

/* The taps of one output position along one axis.  BILINEAR: source indices lo, hi (clamped to the window, lo <= hi) with
 * weights w0 > 0 and w1 >= 0.  BOX: source indices lo .. hi, the weights from scaled_box_weight. */
struct ScaledTaps { uint32_t lo, hi, w0, w1; };

WV_FN ScaledTaps scaled_taps(uint32_t filter, uint32_t S, uint32_t D, uint32_t j)
{
	ScaledTaps t;
	if (filter == 0)
	{
		// n = (2j + 1) S - D >= -D > -2D: its floor quotient by 2D is -1 when negative
		const uint64_t m = (2ull * j + 1ull) * S, d2 = 2ull * D;
		if (m < D)
		{
			t.lo = 0; t.hi = 0;
			t.w1 = (uint32_t)(m + D);                      // f = n + 2D
			t.w0 = (uint32_t)(d2 - t.w1);
			return t;
		}
		const uint64_t n = m - D, i0 = n / d2;
		t.w1 = (uint32_t)(n - i0 * d2);
		t.w0 = (uint32_t)d2 - t.w1;
		t.lo = i0 < S - 1u ? (uint32_t)i0 : S - 1u;
		t.hi = i0 + 1u < S - 1u ? (uint32_t)i0 + 1u : S - 1u;
		return t;
	}
	const uint64_t a = (uint64_t)j * S, b = a + S;
	t.lo = (uint32_t)(a / D); t.hi = (uint32_t)((b - 1u) / D);
	t.w0 = 0; t.w1 = 0;
	return t;
}

WV_FN uint32_t scaled_box_weight(uint32_t S, uint32_t D, uint32_t j, uint32_t k)
{
	const uint64_t a = (uint64_t)j * S, b = a + S, lo = (uint64_t)k * D, hi = lo + D;
	return (uint32_t)((b < hi ? b : hi) - (a > lo ? a : lo));
}

struct DecodeScaledRecord {
	DecodeImage img;                  // the entry's image; data = the region's `out`
	const uint8_t* blocks;
	uint32_t x, y, z;                 // the window's origin; z: the slice
	uint32_t size_x, size_y;          // S per axis
	uint32_t out_x, out_y;            // D per axis
	uint32_t filter, flags;           // astcenc_amd_window_filter, ASTCENC_AMD_TENSOR_FLIP_*
	uint32_t x_step;                  // elements from column to column (1 planar, `channels` interleaved)
	uint32_t cols;                    // output columns per tile (the last strip may be narrower), see decode_scaled_tiling
	uint32_t strips;                  // tiles per band of output rows: ceil(out_x / cols)
	uint32_t band;                    // output rows per tile (the last band may be shorter)
	uint32_t run_blocks;              // blocks per decoded run: what the staging tile holds of this entry's data type, at most DECODE_BATCH
	size_t   row;                     // elements from output row to output row
	TensorParams fmt;
};
static_assert(sizeof(DecodeScaledRecord) % 8 == 0, "records are read word by word and hold pointers");

/* DecodeWindow clipped to the rectangle a tile needs of one run; a texel's place is its index in the staging tile, whose
 * texel (0, 0) is texel (x0, y0) of the image: the first texel of the run's first block.  w.row_texels: the tile's pitch. */
struct ScaledWindow {
	DecodeWindow w;
	uint32_t x0, y0;
	static constexpr bool whole = false;
	WV_FN int cols_begin(uint32_t xr, int row_len) const { return w.cols_begin(xr, row_len); }
	WV_FN int cols_end(uint32_t xr, int row_len) const { return w.cols_end(xr, row_len); }
	WV_FN int rows_begin(uint32_t yr, int rows) const { return w.rows_begin(yr, rows); }
	WV_FN int rows_end(uint32_t yr, int rows) const { return w.rows_end(yr, rows); }
	WV_FN bool has(uint32_t xi, uint32_t yi, uint32_t zi) const { return w.has(xi, yi, zi); }
	WV_FN size_t at(const DecodeImage&, uint32_t xi, uint32_t yi, uint32_t) const { return (size_t)(yi - y0) * w.row_texels + (size_t)(xi - x0); }
	WV_FN size_t row_step(const DecodeImage&) const { return w.row_texels; }
};

/* The sink: the texel as the regions call stores it for the entry's data type (store_texel_at's three routes), at texel index
 * `at` of the staging tile -- 4, 8 or 16 bytes a texel. */
struct ScaledStage {
	uint8_t* stage;
	WV_FN void pixel(const DecodeImage&, int, size_t at, uint32_t px) const { __builtin_memcpy(stage + at * 4, &px, 4); }
	WV_FN void halves(const DecodeImage&, int, size_t at, uint64_t px) const { __builtin_memcpy(stage + at * 8, &px, 8); }
	WV_FN void texel(const DecodeImage& img, int lane, size_t at, float r, float g, float b, float a) const
	{
		if (img.data_type == 0)
		{
			pixel(img, lane, at, pack_texel_u8(img, r, g, b, a));
			return;
		}
		float src[7];
		swizzle_sources(r, g, b, a, src);
		if (img.data_type == 1)
		{
			uint16_t h4[4];
			for (int k = 0; k < 4; k++) h4[k] = float_to_half(src[img.swz[k]]);
			__builtin_memcpy(stage + at * 8, h4, 8);
		}
		else
		{
			float f4[4];
			for (int k = 0; k < 4; k++) f4[k] = src[img.swz[k]];
			__builtin_memcpy(stage + at * 16, f4, 16);
		}
	}
	WV_FN void trip_end(int, int, int) const {}
};

/* Per-wave scratch next to DecodeBatch (LDS). */
struct alignas(16) ScaledTile {
	uint8_t    stage[SCALED_STAGE_BYTES];
	double     carry[SCALED_ROWS][4][SCALED_CARRY];  // a source row's tap sum so far, per output column and component, from run to run (narrow tiles only)
	ScaledTaps xt[SCALED_COLS];                      // the taps of the tile's columns ...
	ScaledTaps yt[SCALED_BAND];                      // ... and rows
};

/* Texel `at` of the staging tile, its four components widened to binary64 (exact for all three data types). */
WV_FN void scaled_staged(const uint8_t* stage, uint32_t data_type, size_t at, double v[4])
{
	if (data_type == 0)
	{
		uint32_t px;
		__builtin_memcpy(&px, stage + at * 4, 4);
		for (int c = 0; c < 4; c++) v[c] = (double)((px >> (8 * c)) & 0xFFu);
	}
	else if (data_type == 1)
	{
		uint16_t h[4];
		__builtin_memcpy(h, stage + at * 8, 8);
		for (int c = 0; c < 4; c++) v[c] = (double)tensor_widen_half(h[c]);
	}
	else
	{
		float f[4];
		__builtin_memcpy(f, stage + at * 16, 16);
		for (int c = 0; c < 4; c++) v[c] = (double)f[c];
	}
}

/* The tiles of a region: strips of `cols` output columns across, bands of `band` output rows down.  run_blocks: the blocks the
 * staging tile holds of the entry's data type, at most DECODE_BATCH.
 *
 * `cols` is the widest strip, up to SCALED_COLS, whose source columns one run holds for certain: a block row is then decoded
 * once and no sum is carried from run to run.  The argument, with c the columns of a strip that starts at output column p:
 *   - L consecutive texels touch at most ceil((L - 1) / block_x) + 1 blocks wherever they start, so a run of n blocks holds
 *     them if L <= hold = (n - 1) block_x + 1;
 *   - BILINEAR: the first column's first tap is at least i0(p) (clamping only moves it inwards), the last column's second tap
 *     at most i0(p + c - 1) + 1, and i0(q) = floor(((2q + 1) S - D) / 2D) grows by at most (c - 1) S / D + 1 over c - 1 columns:
 *     L <= (c - 1) S / D + 3;
 *   - BOX: first index floor(p S / D), last floor(((p + c) S - 1) / D): L <= c S / D + 2;
 *   - so L <= c S / D + 3 for both, and c = floor((hold - 3) D / S) gives L <= hold.
 * Where that leaves fewer than SCALED_CARRY columns (a window reduced so strongly that a few output columns reach more texels
 * than a run has) the strip is SCALED_CARRY columns and the sums are carried.  tests/harness/decode_scaled_check.cpp sweeps
 * sizes, footprints and data types and checks every tile wider than SCALED_CARRY against run_blocks (`sweep`). */
inline void decode_scaled_tiling(uint32_t size_x, uint32_t out_x, uint32_t out_y, uint32_t data_type, uint32_t block_x, uint32_t block_y,
                                 uint32_t& run_blocks, uint32_t& cols, uint32_t& strips, uint32_t& band, uint32_t& bands)
{
	const uint32_t texel = data_type == 0 ? 4u : data_type == 1 ? 8u : 16u;
	const uint32_t fit = (uint32_t)SCALED_STAGE_BYTES / texel / (block_x * block_y);
	run_blocks = fit < (uint32_t)DECODE_BATCH ? fit : (uint32_t)DECODE_BATCH;
	const uint32_t hold = (run_blocks - 1u) * block_x + 1u;
	const uint64_t c = hold > 3u ? (uint64_t)(hold - 3u) * out_x / size_x : 0u;
	cols = c >= (uint64_t)SCALED_COLS ? (uint32_t)SCALED_COLS : c >= (uint64_t)SCALED_CARRY ? (uint32_t)c : (uint32_t)SCALED_CARRY;
	strips = (out_x + cols - 1u) / cols;
	band = out_y < (uint32_t)SCALED_BAND ? out_y : (uint32_t)SCALED_BAND;
	bands = (out_y + band - 1u) / band;
}

inline unsigned long long decode_scaled_tiles(uint32_t size_x, uint32_t out_x, uint32_t out_y, uint32_t data_type, uint32_t block_x, uint32_t block_y)
{
	uint32_t run_blocks, cols, strips, band, bands;
	decode_scaled_tiling(size_x, out_x, out_y, data_type, block_x, block_y, run_blocks, cols, strips, band, bands);
	return (unsigned long long)strips * bands;
}

inline size_t decode_scaled_bytes(uint32_t count) { return decode_table_bytes<DecodeScaledRecord>(count); }

/* Writes the table of `count` regions over the images `images` (prepared, 2D footprints, `data` unused) and their streams;
 * returns the tiles of all regions (the caller has made sure they fit 32 bits). */
inline uint32_t decode_scaled_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeTensorFormat& format, uint32_t filter,
                                    const DecodeScaledLaunch* regions, uint32_t count)
{
	uint32_t* first;
	DecodeScaledRecord* rec = decode_table_begin<DecodeScaledRecord>(out, decode_scaled_bytes(count), count, first);
	uint32_t tiles = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeScaledLaunch& g = regions[i];
		DecodeScaledRecord& r = rec[i];
		r.img = images[g.entry];
		r.img.data = g.d_out;
		r.blocks = streams[g.entry];
		r.x = g.x; r.y = g.y; r.z = g.z;
		r.size_x = g.size_x; r.size_y = g.size_y;
		r.out_x = g.out_x; r.out_y = g.out_y;
		r.filter = filter; r.flags = g.flags;
		r.x_step = tensor_x_step(format);
		r.row = g.row_pitch;
		r.fmt = tensor_params(format, g.plane_pitch);
		uint32_t bands;
		decode_scaled_tiling(g.size_x, g.out_x, g.out_y, r.img.data_type, r.img.block_x, r.img.block_y, r.run_blocks, r.cols, r.strips, r.band, bands);
		first[i] = tiles;
		tiles += r.strips * bands;
	}
	return decode_table_finish(out, count, tiles);
}

/* The output columns [c0, c0 + nc) and rows [r0, r0 + nr) of tile `local` of a region, and the window-relative source
 * rectangle [sx0, sx1] x [sy0, sy1] (inclusive) its taps reach.  Taps grow with the position, so the ends are those of the
 * tile's first and last column / row. */
struct ScaledTileRect { uint32_t c0, nc, r0, nr, sx0, sx1, sy0, sy1; };

WV_FN ScaledTileRect decode_scaled_rect(const DecodeScaledRecord& rec, uint32_t local)
{
	ScaledTileRect q;
	const uint32_t band = local / rec.strips;
	q.c0 = (local - band * rec.strips) * rec.cols;
	q.nc = rec.out_x - q.c0 < rec.cols ? rec.out_x - q.c0 : rec.cols;
	q.r0 = band * rec.band;
	q.nr = rec.out_y - q.r0 < rec.band ? rec.out_y - q.r0 : rec.band;
	q.sx0 = scaled_taps(rec.filter, rec.size_x, rec.out_x, q.c0).lo;
	q.sx1 = scaled_taps(rec.filter, rec.size_x, rec.out_x, q.c0 + q.nc - 1u).hi;
	q.sy0 = scaled_taps(rec.filter, rec.size_y, rec.out_y, q.r0).lo;
	q.sy1 = scaled_taps(rec.filter, rec.size_y, rec.out_y, q.r0 + q.nr - 1u).hi;
	return q;
}

/* The blocks tile `local` decodes -- every block its source rectangle touches, once: what decode_scaled_tile returns -- and,
 * in `widest`, the blocks of its widest block row (host code: the harness checks the tiling's promise with it, and
 * tools/time_decode_scaled.py counts blocks decoded per block covered with it). */
inline uint32_t decode_scaled_tile_blocks(const DecodeScaledRecord& rec, uint32_t local, uint32_t* widest = nullptr)
{
	const ScaledTileRect q = decode_scaled_rect(rec, local);
	const uint32_t across = (rec.x + q.sx1) / rec.img.block_x - (rec.x + q.sx0) / rec.img.block_x + 1u;
	const uint32_t down = (rec.y + q.sy1) / rec.img.block_y - (rec.y + q.sy0) / rec.img.block_y + 1u;
	if (widest) *widest = across;
	return across * down;
}

/* The band sums of a lane: registers on the device (every index is a constant of an unrolled loop); the sequential build,
 * whose lanes take turns, keeps a set per lane. */
#if WV_DEVICE
#define SCALED_ACC_DECL double acc_regs[SCALED_BAND][4]
#define SCALED_ACC(l, jj, c) acc_regs[jj][c]
#else
#define SCALED_ACC_DECL double acc_lanes[SCALED_COLS][SCALED_BAND][4]
#define SCALED_ACC(l, jj, c) acc_lanes[l][jj][c]
#endif

/* Tile `local` of the region of `rec` (all 64 lanes call this; `local` is uniform); kType / kLayout are the record's.  Returns
 * the blocks it decoded (uniform; the harness sums them). */
template <uint32_t kType, uint32_t kLayout>
WV_FN uint32_t decode_scaled_tile(const DecodeScaledRecord& rec, uint32_t local, DecodeBatch& batch, ScaledTile& tile)
{
	const ScaledTileRect q = decode_scaled_rect(rec, local);
	const uint32_t filter = rec.filter, Sx = rec.size_x, Dx = rec.out_x, Sy = rec.size_y, Dy = rec.out_y;
	const uint32_t block_x = rec.img.block_x, block_y = rec.img.block_y, data_type = rec.img.data_type;
	WV_FOR64(l, 64)
	{
		if ((uint32_t)l < q.nc) tile.xt[l] = scaled_taps(filter, Sx, Dx, q.c0 + (uint32_t)l);
		if ((uint32_t)l < q.nr) tile.yt[l] = scaled_taps(filter, Sy, Dy, q.r0 + (uint32_t)l);
	}
	WV_SYNC();

	// the image's texels the tile needs, and the blocks that hold them
	const uint32_t ax0 = rec.x + q.sx0, ax1 = rec.x + q.sx1, ay0 = rec.y + q.sy0, ay1 = rec.y + q.sy1;
	const uint32_t bxa = ax0 / block_x, bxb = ax1 / block_x, bya = ay0 / block_y, byb = ay1 / block_y;
#if !WV_DEVICE
	// (what the tiling promises: a tile wider than SCALED_CARRY columns decodes a block row in one run)
	if (q.nc > (uint32_t)SCALED_CARRY && bxb - bxa + 1u > rec.run_blocks) __builtin_trap();
#endif
	ScaledStage sink = { tile.stage };
	ScaledWindow win;
	win.w.x = ax0; win.w.end_x = ax1 + 1u; win.w.y = ay0; win.w.end_y = ay1 + 1u; win.w.z = rec.z; win.w.end_z = rec.z + 1u;
	win.w.slice_texels = 0;
	SCALED_ACC_DECL;
	uint32_t decoded = 0;
	for (uint32_t by = bya; by <= byb; by++)
	{
		const uint32_t y0 = by * block_y;
		// the block row's texel rows inside the rectangle: [ty0, ty1) of the block row, source rows ky0 + (ty - ty0) of the window
		const uint32_t ty0 = ay0 > y0 ? ay0 - y0 : 0u, ty1 = ay1 - y0 < block_y - 1u ? ay1 - y0 + 1u : block_y;
		const uint32_t ky0 = y0 + ty0 - rec.y;
		for (uint32_t bx = bxa; bx <= bxb; bx += rec.run_blocks)
		{
			const uint32_t count = bxb - bx + 1u < rec.run_blocks ? bxb - bx + 1u : rec.run_blocks;
			const uint32_t x0 = bx * block_x, pitch = count * block_x;
			const bool first_run = bx == bxa, last_run = bx + count > bxb;
			win.x0 = x0; win.y0 = y0;
			win.w.row_texels = pitch;
			decode_row_batch(rec.img, rec.blocks, bx, by, rec.z, (int)count, batch, sink, win);
			decoded += count;
			// The run holds source columns [ka, kb] of the window (inside the rectangle).  x pass: every lane continues its
			// column's tap sum of every staged source row; after the block row's last run the sum is complete and goes, weighted,
			// into the output rows whose y taps hold the source row (y pass), top to bottom
			const uint32_t ka = x0 > ax0 ? x0 - rec.x : q.sx0, kb = x0 + pitch - 1u < ax1 ? x0 + pitch - 1u - rec.x : q.sx1;
			WV_FOR64(l, q.nc)
			{
				const ScaledTaps t = tile.xt[l];
				const bool mine = t.hi >= ka && t.lo <= kb;
				const uint32_t j = q.c0 + (uint32_t)l;
				const int slot = l & (SCALED_CARRY - 1);          // (several runs: the tile has at most SCALED_CARRY columns)
				for (uint32_t ty = ty0; ty < ty1; ty++)
				{
					double r[4] = { 0.0, 0.0, 0.0, 0.0 };
					if (!first_run) for (int c = 0; c < 4; c++) r[c] = tile.carry[ty][c][slot];
					if (mine)
					{
						// (the staged texel of source column k of this row: at = base + k)
						const size_t base = (size_t)ty * pitch + rec.x - x0;
						double v[4];
						if (filter == 0)
						{
							if (t.lo >= ka && t.lo <= kb)
							{
								scaled_staged(tile.stage, data_type, base + t.lo, v);
								for (int c = 0; c < 4; c++) r[c] = (double)t.w0 * v[c];
							}
							if (t.w1 != 0u && t.hi >= ka && t.hi <= kb)
							{
								scaled_staged(tile.stage, data_type, base + t.hi, v);
								for (int c = 0; c < 4; c++) r[c] = r[c] + (double)t.w1 * v[c];
							}
						}
						else
						{
							const uint32_t k0 = t.lo > ka ? t.lo : ka, k1 = t.hi < kb ? t.hi : kb;
							for (uint32_t k = k0; k <= k1; k++)
							{
								const double w = (double)scaled_box_weight(Sx, Dx, j, k);
								scaled_staged(tile.stage, data_type, base + k, v);
								for (int c = 0; c < 4; c++) r[c] = k == t.lo ? w * v[c] : r[c] + w * v[c];
							}
						}
					}
					if (!last_run)
					{
						for (int c = 0; c < 4; c++) tile.carry[ty][c][slot] = r[c];
						continue;
					}
					const uint32_t ky = ky0 + (ty - ty0);
#if WV_DEVICE
					#pragma unroll
#endif
					for (uint32_t jj = 0; jj < (uint32_t)SCALED_BAND; jj++)
					{
						if (jj >= q.nr) continue;
						const ScaledTaps u = tile.yt[jj];
						if (ky < u.lo || ky > u.hi) continue;
						if (filter == 0)
						{
							if (ky == u.lo) for (int c = 0; c < 4; c++) SCALED_ACC(l, jj, c) = (double)u.w0 * r[c];
							if (u.w1 != 0u && ky == u.hi) for (int c = 0; c < 4; c++) SCALED_ACC(l, jj, c) = SCALED_ACC(l, jj, c) + (double)u.w1 * r[c];
						}
						else
						{
							const double w = (double)scaled_box_weight(Sy, Dy, q.r0 + jj, ky);
							for (int c = 0; c < 4; c++) SCALED_ACC(l, jj, c) = ky == u.lo ? w * r[c] : SCALED_ACC(l, jj, c) + w * r[c];
						}
					}
				}
			}
			WV_SYNC();
		}
	}

	// divide, convert, place
	const double den = (filter == 0 ? 2.0 * (double)Dx : (double)Sx) * (filter == 0 ? 2.0 * (double)Dy : (double)Sy);
	TensorStore<kType, kLayout> store = { rec.fmt };
	WV_FOR64(l, q.nc)
	{
		const uint32_t i = q.c0 + (uint32_t)l;
		const uint32_t io = (rec.flags & 1u) ? Dx - 1u - i : i;
#if WV_DEVICE
		#pragma unroll
#endif
		for (uint32_t jj = 0; jj < (uint32_t)SCALED_BAND; jj++)
		{
			if (jj >= q.nr) continue;
			const uint32_t j = q.r0 + jj;
			const uint32_t jo = (rec.flags & 2u) ? Dy - 1u - j : j;
			float s[4];
			for (int c = 0; c < 4; c++) s[c] = (float)(SCALED_ACC(l, jj, c) / den);
			store.template put<false>(rec.img, (size_t)jo * rec.row + (size_t)io * rec.x_step, s);
		}
	}
	WV_SYNC();
	return decoded;
}

} } // namespace astcd::ASTC_VARIANT
