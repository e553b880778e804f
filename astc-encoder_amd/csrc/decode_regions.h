// SPDX-License-Identifier: Apache-2.0
// Windows of compressed images (astcenc_amd_decompress_regions_device): the table of a call's regions and what one work item
// does with it.  A work item is a run of at most DECODE_BATCH consecutive covered blocks of one block row and one layer of
// blocks of one region; the runs of all regions sit back to back, a run finds its region in the table (image_set.h) and decodes
// its blocks with the window policy of wave_decode.h (DecodeWindow): blocks outside a window's covered range are never read.
// The table is built on the host by plain code over the frame of decode_table.h (decode_regions_build: kernel_decode.hip calls it for the kernel,
// tests/harness/decode_region_check.cpp for the sequential build); decode_region_run is the kernel's body.
//
// Layout (16-byte aligned), as image_set.h lays an image set out: ImageSetTable (count = regions, total = runs), first[count],
// padding, DecodeRegionRecord[count].
#pragma once
#include "backend.h"          // DecodeRegionLaunch: one region as the host hands it over, everything checked already
#include "decode_table.h"

namespace astcd { inline namespace ASTC_VARIANT {

struct DecodeRegionRecord {
	DecodeImage img;                  // the entry's image; data = the region's `out`
	const uint8_t* blocks;            // the entry's stream
	DecodeWindow win;
	uint32_t bx0, by0, bz0;           // first covered block column / row / layer
	uint32_t cols;                    // covered block columns
	uint32_t runs_x;                  // runs per covered block row: ceil(cols / DECODE_BATCH)
	uint32_t runs_xy;                 // ... per covered layer of blocks
};
static_assert(sizeof(DecodeRegionRecord) % 8 == 0, "records are read word by word and hold pointers");

/* The covered blocks of a window along one axis: first block and how many. */
inline void decode_region_cover(uint32_t at, uint32_t size, uint32_t block, uint32_t& first, uint32_t& count)
{
	first = at / block;
	count = (at + size - 1u) / block - first + 1u;
}

/* Runs of one window (64 bits: the caller bounds the sum). */
inline unsigned long long decode_region_runs(uint32_t x, uint32_t y, uint32_t z, uint32_t size_x, uint32_t size_y, uint32_t size_z,
                                             uint32_t block_x, uint32_t block_y, uint32_t block_z)
{
	uint32_t f, cx, cy, cz;
	decode_region_cover(x, size_x, block_x, f, cx);
	decode_region_cover(y, size_y, block_y, f, cy);
	decode_region_cover(z, size_z, block_z, f, cz);
	return (unsigned long long)((cx + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH) * cy * cz;
}

inline size_t decode_regions_bytes(uint32_t count) { return decode_table_bytes<DecodeRegionRecord>(count); }

/* Writes the table of `count` regions over the images `images` (prepared, `data` unused) and their streams; returns the runs
 * of all regions (the caller has made sure they fit 32 bits). */
inline uint32_t decode_regions_build(void* out, const DecodeImage* images, const uint8_t* const* streams, const DecodeRegionLaunch* regions, uint32_t count)
{
	uint32_t* first;
	DecodeRegionRecord* rec = decode_table_begin<DecodeRegionRecord>(out, decode_regions_bytes(count), count, first);
	uint32_t runs = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeRegionLaunch& g = regions[i];
		DecodeRegionRecord& r = rec[i];
		r.img = images[g.entry];
		r.img.data = g.d_out;
		r.blocks = streams[g.entry];
		const size_t texel = r.img.data_type == 0 ? 4 : r.img.data_type == 1 ? 8 : 16;
		r.win.x = g.x; r.win.y = g.y; r.win.z = g.z;
		r.win.end_x = g.x + g.size_x; r.win.end_y = g.y + g.size_y; r.win.end_z = g.z + g.size_z;
		r.win.row_texels = g.row_pitch / texel;
		r.win.slice_texels = g.slice_pitch / texel;
		uint32_t rows, layers;
		decode_region_cover(g.x, g.size_x, r.img.block_x, r.bx0, r.cols);
		decode_region_cover(g.y, g.size_y, r.img.block_y, r.by0, rows);
		decode_region_cover(g.z, g.size_z, r.img.block_z, r.bz0, layers);
		r.runs_x = (r.cols + (uint32_t)DECODE_BATCH - 1u) / (uint32_t)DECODE_BATCH;
		r.runs_xy = r.runs_x * rows;
		first[i] = runs;
		runs += r.runs_xy * layers;
	}
	return decode_table_finish(out, count, runs);
}

/* Run `local` of the region of `rec` (all 64 lanes call this; `local` is uniform): its place among the covered blocks -- run,
 * block row, layer -- split off with scalar arithmetic, then the decoder's routine over the window. */
template <class Sink>
WV_FN void decode_region_run(const DecodeRegionRecord& rec, uint32_t local, DecodeBatch& batch, Sink& sink)
{
	const uint32_t lz = local / rec.runs_xy;
	const uint32_t in_layer = local - lz * rec.runs_xy;
	const uint32_t ly = in_layer / rec.runs_x;
	const uint32_t c0 = (in_layer - ly * rec.runs_x) * (uint32_t)DECODE_BATCH;
	const uint32_t left = rec.cols - c0;
	decode_row_batch(rec.img, rec.blocks, rec.bx0 + c0, rec.by0 + ly, rec.bz0 + lz, (int)(left < (uint32_t)DECODE_BATCH ? left : (uint32_t)DECODE_BATCH), batch, sink, rec.win);
}

} } // namespace astcd::ASTC_VARIANT
