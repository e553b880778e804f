// SPDX-License-Identifier: Apache-2.0
// What the host side of every table-driven decode launch shares (the image set, the windowed and the sampled decoders, the
// block quality pass): an entry's DecodeLaunch made the prepared DecodeImage of the kernels, the images and streams of a call's
// entries, and the frame of a table -- cleared, first[] and the records located, the head written (image_set.h has the layout).
// Plain host code: the sequential build of tests/harness compiles it with g++ through decode_regions.h.
#pragma once
#include "backend.h"          // DecodeLaunch
#include "image_set.h"
#include "wave_decode.h"
#include <cstring>
#include <vector>

namespace astcd { inline namespace ASTC_VARIANT {

/* The image of an entry's launch, prepared; `data`: where the texels go, null where a table's records carry that. */
inline DecodeImage decode_image_of(const DecodeLaunch& d, void* data)
{
	DecodeImage img;
	img.data = data;
	img.tabs = static_cast<const DecodeTables*>(d.d_tables);
	img.dim_x = d.dim_x; img.dim_y = d.dim_y; img.dim_z = d.dim_z;
	img.data_type = d.data_type;
	for (int i = 0; i < 4; i++) img.swz[i] = d.swz[i];
	img.block_x = d.block_x; img.block_y = d.block_y; img.block_z = d.block_z;
	img.blocks_x = (d.dim_x + d.block_x - 1) / d.block_x;
	img.blocks_y = (d.dim_y + d.block_y - 1) / d.block_y;
	img.blocks_z = (d.dim_z + d.block_z - 1) / d.block_z;
	img.profile = d.profile;
	decode_image_prepare(img);
	return img;
}

/* The images (`data` null) and the streams of a call's entries, as the table builders take them. */
struct DecodeEntries {
	std::vector<DecodeImage> images;
	std::vector<const uint8_t*> streams;
	DecodeEntries(const DecodeLaunch* entries, uint32_t count) : images(count), streams(count)
	{
		for (uint32_t e = 0; e < count; e++)
		{
			images[e] = decode_image_of(entries[e], nullptr);
			streams[e] = entries[e].d_blocks;
		}
	}
};

/* Bytes of a table of `count` records and nothing behind them. */
template <class Record>
inline size_t decode_table_bytes(uint32_t count)
{
	return (size_t)image_set_records_offset(count) + (size_t)count * sizeof(Record);
}

/* The frame of a table of `bytes` bytes at `out`: all of it cleared; returns record 0 and, in `first`, first[]. */
template <class Record>
inline Record* decode_table_begin(void* out, size_t bytes, uint32_t count, uint32_t*& first)
{
	uint8_t* t = static_cast<uint8_t*>(out);
	memset(t, 0, bytes);
	first = reinterpret_cast<uint32_t*>(t + image_set_first_offset());
	return reinterpret_cast<Record*>(t + image_set_records_offset(count));
}

/* ... and its head, once first[] and the records are written; returns `total`. */
inline uint32_t decode_table_finish(void* out, uint32_t count, uint32_t total)
{
	ImageSetTable* h = static_cast<ImageSetTable*>(out);
	h->count = count;
	h->total = total;
	return total;
}

} } // namespace astcd::ASTC_VARIANT
