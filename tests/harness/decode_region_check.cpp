// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the windowed decode of astcenc_amd_decompress_regions_device (decode_regions.h: the host-built table,
// decode_region_run over the window policy of wave_decode.h) against decode_row_batch of the whole image followed by a crop,
// on the host, as plain sequential code under the sanitizers.  Random 16-byte patterns mixed with constant-colour blocks
// (UNORM16 and FP16) and reserved-mode blocks; footprints 4x4, 6x6, 10x5, 12x12, 3x3x3 and 6x6x6; the three data types, the four
// profiles, an identity, a BGRA and the Z swizzle; images 34 blocks wide, the last block partial on every axis, two block rows
// and two slices / layers.  Per image one table of all its windows, each once tight and once with padded pitches.  Required:
// every window byte equal to the crop, every other byte of every buffer (guards in front, behind and in the padding) intact,
// the inputs unchanged, ceil(window columns of the run / 64) trips per run on 2D footprints, as many runs as the table says and
// as the windows' covered blocks need.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_region_check.cpp -o decode_region_check
// `decode_region_check tables` prints the tables of a few hand-computed cases instead (tests/test_decode_regions_cpu.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_regions.h"
#include "decode_check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

/* The decoder's store, counting the trips of the texel phase. */
struct CountingStore : DecodeStore {
	int trips = 0;
	void trip_end(int, int, int) { trips++; }
};

struct Window { uint32_t x, y, z, sx, sy, sz; };

static void check(int bx, int by, int bz, int profile, uint32_t dtype, const uint32_t swz[4])
{
	// 34 blocks per row (a full run and one of two blocks), the last block partial on every axis; two block rows, two slices / layers
	const uint32_t dim_x = 34u * bx - (uint32_t)bx / 2u, dim_y = 2u * by - 1u, dim_z = bz == 1 ? 2u : (uint32_t)bz + 1u;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%dx%d %ux%ux%u profile %d type %u swizzle %u%u%u%u", bx, by, bz, dim_x, dim_y, dim_z, profile, dtype, swz[0], swz[1], swz[2], swz[3]);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
	DecodeImage img = make_image(bx, by, bz, dim_x, dim_y, dim_z, profile, dtype, swz, tabs.data());
	const size_t nblocks = (size_t)img.blocks_x * img.blocks_y * img.blocks_z, texels = (size_t)dim_x * dim_y * dim_z;
	const size_t tb = dtype == 0 ? 4 : dtype == 1 ? 8 : 16;

	std::vector<uint8_t> blocks(nblocks * 16);
	for (size_t b = 0; b < nblocks; b++)
	{
		uint8_t* p = blocks.data() + b * 16;
		for (int i = 0; i < 16; i++) p[i] = (uint8_t)rnd();
		const uint32_t kind = rnd() % 16u;
		if (kind < 3)
		{
			// constant colour without an extent: 0x1FC, the FP16 flag, the reserved bits and the extent all ones
			p[0] = 0xFC; p[1] = kind == 2 ? 0xFF : 0xFD;
			for (int i = 2; i < 8; i++) p[i] = 0xFF;
			if (kind == 2) for (int i = 0; i < 4; i++) { const uint16_t h = (uint16_t)(rnd() % 0x7C00u); memcpy(p + 8 + 2 * i, &h, 2); }
		}
		else if (kind == 3) memset(p, 0, 16);       // a reserved block mode: an error block
	}
	const std::vector<uint8_t> blocks_before = blocks;

	// the whole image, as the decoder writes it
	std::vector<uint8_t> whole(texels * tb, 0x5A);
	img.data = whole.data();
	std::vector<DecodeBatch> batch(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	for (uint32_t z = 0; z < img.blocks_z; z++)
		for (uint32_t y = 0; y < img.blocks_y; y++)
			for (uint32_t x0 = 0; x0 < img.blocks_x; x0 += DECODE_BATCH)
				decode_row_batch(img, blocks.data(), x0, y, z, i_min(DECODE_BATCH, (int)(img.blocks_x - x0)), batch[0]);
	img.data = nullptr;

	const uint32_t ubx = (uint32_t)bx, uby = (uint32_t)by, ubz = (uint32_t)bz;
	const uint32_t in_x = ubx > 2 ? ubx - 2 : 1, in_y = uby > 2 ? uby - 2 : 1;
	std::vector<Window> windows = {
		{ 0, 0, 0, dim_x, dim_y, dim_z },                                           // the whole image
		{ dim_x / 2, dim_y / 2, dim_z - 1, 1, 1, 1 },                               // one texel
		{ 3 * ubx + 1, uby + 1, 0, in_x, in_y, 1 },                                 // inside one block
		{ ubx / 2, uby / 2, 0, 33 * ubx, uby, 1 },                                  // mid-block to mid-block over 34 blocks and both block rows: two runs a row
		{ ubx + 1, 0, dim_z - 1, 70, uby + 1, 1 },                                  // more than 64 texels wide: two trips
		{ 5 * ubx, uby, 0, 2 * ubx + 1, uby - 1, 1 },                               // first covered block is block 5, row 1
		{ dim_x - 5, dim_y - 2, dim_z - 1, 5, 2, 1 },                               // ends in the partial last block of every axis
		bz == 1 ? Window{ 2 * ubx + 1, 1, 0, 3 * ubx, uby, 2 }                      // two array slices
		        : Window{ 2 * ubx + 1, 1, ubz - 1, 3 * ubx, uby, 2 },               // ... two layers of blocks
	};

	// one call: every window once tight, once with a row pitch padded by 3 texels and a slice pitch padded by one row
	const size_t guard = 64;
	const uint32_t count = (uint32_t)windows.size() * 2u;
	std::vector<DecodeRegionLaunch> regions(count);
	std::vector<std::vector<uint8_t>> outs(count);
	for (uint32_t i = 0; i < count; i++)
	{
		const Window& w = windows[i / 2];
		const bool padded = (i & 1u) != 0u;
		const size_t row_pitch = ((size_t)w.sx + (padded ? 3 : 0)) * tb, slice_pitch = row_pitch * ((size_t)w.sy + (padded ? 1 : 0));
		outs[i].assign(guard + slice_pitch * w.sz + guard, 0xA5);
		DecodeRegionLaunch& r = regions[i];
		r.entry = 0;
		r.x = w.x; r.y = w.y; r.z = w.z; r.size_x = w.sx; r.size_y = w.sy; r.size_z = w.sz;
		r.d_out = outs[i].data() + guard;
		r.row_pitch = row_pitch; r.slice_pitch = slice_pitch;
	}
	std::vector<uint8_t> table(decode_regions_bytes(count));
	const uint8_t* stream = blocks.data();
	const uint32_t total = decode_regions_build(table.data(), &img, &stream, regions.data(), count);
	const std::vector<uint8_t> table_before = table;

	// the runs the windows need, counted block by block
	uint32_t want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Window& w = windows[i / 2];
		const uint32_t cols = (w.x + w.sx - 1) / ubx - w.x / ubx + 1, rows = (w.y + w.sy - 1) / uby - w.y / uby + 1, layers = (w.z + w.sz - 1) / ubz - w.z / ubz + 1;
		uint32_t runs_x = 0;
		for (uint32_t c = 0; c < cols; c += DECODE_BATCH) runs_x++;
		want_total += runs_x * rows * layers;
	}

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	uint32_t executed = 0;
	for (uint32_t r = 0; r < head->total; r++, executed++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeRegionRecord rec = image_set_record<DecodeRegionRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeRegionRecord)));
		const uint32_t local = r - first[g];
		CountingStore sink;
		decode_region_run(rec, local, batch[0], sink);
		if (bz == 1)
		{
			// the run's blocks, then the window's columns among theirs
			const uint32_t c0 = (local % rec.runs_x) * DECODE_BATCH;
			const uint32_t b0 = rec.bx0 + c0, nb = rec.cols - c0 < (uint32_t)DECODE_BATCH ? rec.cols - c0 : (uint32_t)DECODE_BATCH;
			const uint32_t lo = regions[g].x > b0 * ubx ? regions[g].x : b0 * ubx;
			const uint32_t end = regions[g].x + regions[g].size_x, hi = end < (b0 + nb) * ubx ? end : (b0 + nb) * ubx;
			if (sink.trips != (int)((hi - lo + 63u) / 64u)) fail("trips of a run", tag, g, sink.trips);
		}
	}
	if (executed != want_total) fail("runs executed", tag, -1, executed);

	if (blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeRegionLaunch& r = regions[i];
		const std::vector<uint8_t>& o = outs[i];
		std::vector<uint8_t> want(o.size(), 0xA5);
		for (uint32_t k = 0; k < r.size_z; k++)
			for (uint32_t j = 0; j < r.size_y; j++)
				memcpy(want.data() + guard + k * r.slice_pitch + j * r.row_pitch,
				       whole.data() + ((((size_t)(r.z + k) * dim_y + (r.y + j)) * dim_x) + r.x) * tb, (size_t)r.size_x * tb);
		if (o != want)
		{
			size_t at = 0;
			while (o[at] == want[at]) at++;
			const bool inside = at >= guard && at < o.size() - guard && (at - guard) % r.row_pitch < (size_t)r.size_x * tb && (at - guard) % r.slice_pitch < r.row_pitch * r.size_y;
			fail(inside ? "a window byte differs from the crop" : "a byte outside the window was written", tag, i, (long)at - (long)guard);
		}
	}
}

/* The tables of a few hand-computed cases (6x6, a 230 x 50 x 2 and a 100 x 30 image), one line each. */
static void print_table(const char* name, const DecodeImage* images, uint32_t entries, const std::vector<DecodeRegionLaunch>& regions)
{
	std::vector<const uint8_t*> streams(entries, nullptr);
	std::vector<uint8_t> table(decode_regions_bytes((uint32_t)regions.size()));
	const uint32_t total = decode_regions_build(table.data(), images, streams.data(), regions.data(), (uint32_t)regions.size());
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeRegionRecord* rec = reinterpret_cast<const DecodeRegionRecord*>(table.data() + image_set_records_offset(head->count));
	printf("%s: count %u total %u returned %u first", name, head->count, head->total, total);
	for (uint32_t i = 0; i < head->count; i++) printf(" %u", first[i]);
	printf(" records");
	for (uint32_t i = 0; i < head->count; i++)
		printf(" [bx0 %u by0 %u bz0 %u cols %u runs_x %u runs_xy %u dim_x %u]", rec[i].bx0, rec[i].by0, rec[i].bz0, rec[i].cols, rec[i].runs_x, rec[i].runs_xy, rec[i].img.dim_x);
	printf("\n");
}

static int tables()
{
	const uint32_t rgba[4] = { 0, 1, 2, 3 };
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 6, 6, 1);
	const DecodeImage images[2] = { make_image(6, 6, 1, 230, 50, 2, 0, 0, rgba, tabs.data()), make_image(6, 6, 1, 100, 30, 1, 0, 1, rgba, tabs.data()) };
	static uint8_t sink[16];
	auto region = [](uint32_t entry, uint32_t x, uint32_t y, uint32_t z, uint32_t sx, uint32_t sy, uint32_t sz)
	{
		DecodeRegionLaunch r;
		memset(&r, 0, sizeof(r));
		r.entry = entry; r.x = x; r.y = y; r.z = z; r.size_x = sx; r.size_y = sy; r.size_z = sz;
		r.d_out = sink; r.row_pitch = (size_t)sx * (entry == 0 ? 4 : 8); r.slice_pitch = r.row_pitch * sy;
		return r;
	};
	print_table("exactly 32 blocks", images, 2, { region(0, 6, 0, 0, 192, 6, 1) });
	print_table("33 blocks", images, 2, { region(0, 5, 5, 0, 193, 2, 1) });
	print_table("one block", images, 2, { region(0, 7, 7, 1, 1, 1, 1) });
	print_table("shared entry", images, 2, { region(0, 6, 0, 0, 192, 6, 1), region(0, 5, 5, 0, 193, 2, 1), region(1, 7, 7, 0, 1, 1, 1), region(0, 0, 0, 0, 230, 50, 2), region(1, 94, 29, 0, 6, 1, 1) });
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	const int footprints[6][3] = { { 4, 4, 1 }, { 6, 6, 1 }, { 10, 5, 1 }, { 12, 12, 1 }, { 3, 3, 3 }, { 6, 6, 6 } };
	const uint32_t swizzles[3][4] = { { 0, 1, 2, 3 }, { 2, 1, 0, 3 }, { 0, 3, 6, 5 } };     // identity, BGRA, a normal map's: r, a, the reconstructed z, 1
	for (const int* f : footprints)
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 3; dtype++)
				for (const uint32_t* swz : swizzles) check(f[0], f[1], f[2], profile, dtype, swz);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	return g_bad == 0 ? 0 : 1;
}
