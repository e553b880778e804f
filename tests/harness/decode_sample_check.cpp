// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the coordinate sampler of astcenc_amd_sample_tensors_device (decode_sample.h: the host-built table and
// decode_sample_tile -- taps, the batches of distinct blocks, decode_batch_blocks over a list, decode_batch_texel per tap, the
// sums) against decode_row_batch of the whole image followed by the definition written out in plain C++ below from the header's
// comment, on the host, as sequential code under the sanitizers.  Random 16-byte patterns mixed with constant-colour blocks
// (UNORM16 and FP16) and reserved-mode blocks; footprints 4x4, 6x6, 10x8 and 12x12; the three data types, the four profiles;
// images of 33 blocks and three texels by two block rows and one texel, two slices.  Each image is sampled with both filters and
// six formats -- every tensor type with both layouts -- the address modes turning from table to table so that every pair is met,
// and per table several grids: random points over the image and a block of margin, the texel centres of a window, 64 equal
// points, grids of 2, 3 and 5 rows whose width is no multiple of the tile's, the special coordinates (edges, -0.0, tiny, NaN,
// infinities, 2^30 and the next binary32), points far outside; tight and padded pitches alternate, for outputs and coordinates.
// Then, per footprint, a 17 x 17-block image sampled at 64 block corners whose taps reach 256 distinct blocks: eight full batches.
// Required: every element of every grid equal to the model's bits, every other byte of every buffer intact, the inputs
// unchanged, as many tiles as the grids' sizes need.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_sample_check.cpp -o decode_sample_check
// `decode_sample_check tables` prints the tables of a few hand-computed cases instead (tests/test_decode_sample_cpu.py);
// `blocks` runs the tiles of one grid read from a file and counts batches and blocks decoded (tools/time_decode_sample.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_sample.h"
#define DECODE_CHECK_ITEM "grid"
#include "decode_check_common.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_decoded = 0, g_batches = 0;
static unsigned g_pairs_seen = 0;              // bit (address_x * 4 + address_y)

/* The model (include/astcenc_amd.h), one operation at a time: a texel's component widened (source_value, decode_check_common.h) ... */
/* ... the taps of a coordinate along an axis: indices before addressing and weights in tap order, zero weights left out ... */
struct Tap { int64_t i; double w; };
static void model_taps(uint32_t filter, float u, std::vector<Tap>& taps)
{
	taps.clear();
	if (filter == 0)
	{
		taps.push_back({ (int64_t)std::floor((double)u), 1.0 });
		return;
	}
	volatile double t = (double)u - 0.5;
	const double fl = std::floor(t);
	volatile double f = t - fl;
	volatile double w0 = 1.0 - f;
	taps.push_back({ (int64_t)fl, w0 });
	if (f != 0.0) taps.push_back({ (int64_t)fl + 1, f });
}

/* ... the address modes, on 64-bit integers; false: a BORDER tap outside ... */
static bool model_address(uint32_t mode, int64_t i, int64_t S, int64_t& k)
{
	if (mode == 0) { k = i < 0 ? 0 : i > S - 1 ? S - 1 : i; return true; }
	if (mode == 1) { k = ((i % S) + S) % S; return true; }
	if (mode == 2)
	{
		const int64_t m = ((i % (2 * S)) + 2 * S) % (2 * S);
		k = m < S ? m : 2 * S - 1 - m;
		return true;
	}
	k = i;
	return i >= 0 && i <= S - 1;
}

struct Grid { uint32_t z, ox, oy; std::vector<float> xy; };       // xy: ox * oy pairs, row by row

static SampleTileCount run_tile(const DecodeSampleRecord& rec, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	return with_build(rec.fmt.type, rec.fmt.layout, [&](auto t, auto l) { return decode_sample_tile<decltype(t)::value, decltype(l)::value>(rec, local, batch, tile); });
}

/* One table of all `wanted` grids over one image; returns the batches and blocks of its tiles through `per_tile` when given. */
static void check_table(const char* image_tag, const DecodeImage& img, const std::vector<uint8_t>& blocks, const std::vector<uint8_t>& whole,
                        const std::vector<Grid>& wanted, DecodeBatch& batch, SampleTile& tile, const Format& f, const DecodeSampler& smp, uint32_t turn,
                        std::vector<SampleTileCount>* per_tile = nullptr)
{
	char tag[256];
	snprintf(tag, sizeof(tag), "%s -> filter %u address %u %u type %u layout %u channels %u", image_tag, smp.filter, smp.address_x, smp.address_y, f.type, f.layout, f.channels);
	const uint32_t dim_x = img.dim_x, dim_y = img.dim_y, dtype = img.data_type;
	const size_t tb = dtype == 0 ? 4 : dtype == 1 ? 8 : 16, eb = f.type == 0 ? 4 : 2;
	const bool planar = f.layout == 0;
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = f.type; format.layout = f.layout; format.channels = f.channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 1.0f / 255.0f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }
	g_pairs_seen |= 1u << (smp.address_x * 4u + smp.address_y);

	const size_t guard = 64;
	const uint32_t count = (uint32_t)wanted.size();
	std::vector<DecodeSampleLaunch> grids(count);
	std::vector<std::vector<uint8_t>> outs(count);
	std::vector<std::vector<float>> coords(count);
	unsigned long long want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Grid& w = wanted[i];
		const bool padded = ((i + turn) & 1u) != 0u, coords_padded = ((i + turn) & 2u) != 0u;
		const size_t row = (size_t)w.ox * (planar ? 1 : f.channels) + (padded ? 3 : 0);
		const size_t plane = planar ? row * w.oy + (padded ? 5 : 0) : 0;
		const size_t elements = planar ? plane * f.channels : row * w.oy;
		outs[i].assign(guard + elements * eb + guard, 0xA5);
		const size_t crow = 2u * (size_t)w.ox + (coords_padded ? 6 : 0);
		// (the padding of a coordinate row holds NaNs: read into a point they would show)
		coords[i].assign(crow * w.oy, __builtin_nanf(""));
		for (uint32_t j = 0; j < w.oy; j++) memcpy(coords[i].data() + j * crow, w.xy.data() + (size_t)j * 2u * w.ox, 2u * (size_t)w.ox * sizeof(float));
		DecodeSampleLaunch& g = grids[i];
		memset(&g, 0, sizeof(g));
		g.entry = 0;
		g.z = w.z; g.out_x = w.ox; g.out_y = w.oy;
		g.d_coords = coords[i].data(); g.coord_row_pitch = crow;
		g.d_out = outs[i].data() + guard;
		g.row_pitch = row; g.plane_pitch = plane;
		// (the tiles, spelled out: 64 x 1, 32 x 2, 16 x 4, 8 x 8 from five rows on)
		const uint32_t th = w.oy >= 5 ? 8u : w.oy >= 3 ? 4u : w.oy, tw = 64u / th;
		want_total += (unsigned long long)((w.ox + tw - 1u) / tw) * ((w.oy + th - 1u) / th);
	}
	std::vector<uint8_t> table(decode_sample_bytes(count));
	const uint8_t* stream = blocks.data();
	const uint32_t total = decode_sample_build(table.data(), &img, &stream, format, smp, grids.data(), count);
	const std::vector<uint8_t> table_before = table, blocks_before = blocks;
	const std::vector<std::vector<float>> coords_before = coords;

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	// (the LDS of a fresh workgroup holds anything)
	memset(static_cast<void*>(&tile), 0xCD, sizeof(SampleTile));
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeSampleRecord rec = image_set_record<DecodeSampleRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeSampleRecord)));
		const SampleTileCount n = run_tile(rec, r - first[g], batch, tile);
		if (n.blocks > 256u || n.batches > 256u || n.batches * (uint32_t)DECODE_BATCH < n.blocks) fail("a tile's batches and blocks", tag, g, (long)n.blocks);
		if (per_tile) per_tile->push_back(n);
		g_decoded += n.blocks;
		g_batches += n.batches;
	}
	if (blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);
	for (uint32_t i = 0; i < count; i++)
		if (memcmp(coords[i].data(), coords_before[i].data(), coords[i].size() * sizeof(float)) != 0) fail("the coordinates changed", tag, i, 0);

	std::vector<Tap> tx, ty;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeSampleLaunch& g = grids[i];
		const std::vector<uint8_t>& o = outs[i];
		std::vector<uint8_t> want(o.size(), 0xA5);
		for (uint32_t j = 0; j < g.out_y; j++)
			for (uint32_t x = 0; x < g.out_x; x++)
			{
				const float cx = g.d_coords[j * g.coord_row_pitch + 2u * x], cy = g.d_coords[j * g.coord_row_pitch + 2u * x + 1u];
				const bool valid = std::isfinite(cx) && std::isfinite(cy) && std::fabs((double)cx) <= 1073741824.0 && std::fabs((double)cy) <= 1073741824.0;
				if (valid) { model_taps(smp.filter, cx, tx); model_taps(smp.filter, cy, ty); }
				for (uint32_t c = 0; c < f.channels; c++)
				{
					volatile double acc = 0.0;
					for (size_t b = 0; valid && b < ty.size(); b++)
					{
						volatile double row = 0.0;
						int64_t ky;
						const bool in_y = model_address(smp.address_y, ty[b].i, (int64_t)dim_y, ky);
						for (size_t a = 0; a < tx.size(); a++)
						{
							int64_t kx;
							const bool in_x = model_address(smp.address_x, tx[a].i, (int64_t)dim_x, kx);
							double v = 0.0;
							if (in_x && in_y) v = source_value(whole.data() + ((((size_t)g.z * dim_y + (size_t)ky) * dim_x) + (size_t)kx) * tb, dtype, c);
							volatile double p = tx[a].w * v;
							row = a == 0 ? p : row + p;
						}
						volatile double p = ty[b].w * row;
						acc = b == 0 ? p : acc + p;
					}
					const float s = valid ? (float)acc : 0.0f;
					const uint32_t bits = model_bits(s, format.scale[c], format.bias[c], f.type);
					const size_t at = planar ? c * g.plane_pitch + j * g.row_pitch + x : j * g.row_pitch + (size_t)x * f.channels + c;
					memcpy(want.data() + guard + at * eb, &bits, eb);
				}
			}
		if (o != want)
		{
			size_t at = 0;
			while (o[at] == want[at]) at++;
			fail(want[at] == 0xA5 && (at < guard || at >= o.size() - guard) ? "a guard byte was written" : "a byte differs from the model (or padding was written)", tag, i,
			     (long)at - (long)guard);
		}
	}
}

static Grid random_grid(uint32_t z, uint32_t ox, uint32_t oy, float x0, float x1, float y0, float y1)
{
	Grid g = { z, ox, oy, {} };
	for (uint32_t k = 0; k < ox * oy; k++)
	{
		g.xy.push_back(x0 + (x1 - x0) * rnd_unit());
		g.xy.push_back(y0 + (y1 - y0) * rnd_unit());
	}
	return g;
}

static void check(int bx, int by, int profile, uint32_t dtype, uint32_t config)
{
	const uint32_t ubx = (uint32_t)bx, uby = (uint32_t)by;
	const uint32_t dim_x = 33u * ubx + 3u, dim_y = 2u * uby + 1u, dim_z = 2u;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%d %ux%ux%u profile %d type %u", bx, by, dim_x, dim_y, dim_z, profile, dtype);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	DecodeImage img = make_image(bx, by, dim_x, dim_y, dim_z, profile, dtype, tabs.data());
	std::vector<uint8_t> blocks, whole;
	random_blocks(blocks, (size_t)img.blocks_x * img.blocks_y * img.blocks_z);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	decode_whole(img, blocks, whole, batch[0]);

	const float W = (float)dim_x, H = (float)dim_y, inf = __builtin_inff(), nan = __builtin_nanf("");
	std::vector<Grid> grids;
	grids.push_back(random_grid(0, 37, 11, -(float)bx, W + (float)bx, -(float)by, H + (float)by));      // the image and a block of margin
	{
		// the texel centres of a window that starts mid-block
		Grid g = { 1, 41, uby + 2u, {} };
		for (uint32_t j = 0; j < g.oy; j++)
			for (uint32_t i = 0; i < g.ox; i++) { g.xy.push_back((float)(ubx / 2u + i) + 0.5f); g.xy.push_back((float)(1u + j) + 0.5f); }
		grids.push_back(g);
	}
	{
		// 64 equal points: one block in one tile
		Grid g = { 0, 64, 1, {} };
		for (uint32_t i = 0; i < 64; i++) { g.xy.push_back(2.0f * (float)bx + 1.25f); g.xy.push_back((float)by + 0.75f); }
		grids.push_back(g);
	}
	grids.push_back(random_grid(1, 35, 2, 0.0f, W, 0.0f, H));                                          // 32 x 2 tiles
	grids.push_back(random_grid(0, 19, 3, 0.0f, W, 0.0f, H));                                          // 16 x 4
	grids.push_back(random_grid(1, 11, 5, -3.0f, W + 3.0f, -3.0f, H + 3.0f));                          // 8 x 8
	{
		// the special coordinates, each against each
		const float big = 1073741824.0f, next = __builtin_nextafterf(big, inf);
		const float s[] = { 0.5f, 0.0f, -0.0f, W - 0.5f, W, 1e-30f, -3.25f, nan, inf, -inf, big, next, -big, -next, H - 0.5f, H, -0.5f, -1.0f, 0.49999997f };
		const uint32_t n = sizeof(s) / sizeof(s[0]);
		Grid g = { 0, n, n, {} };
		for (uint32_t j = 0; j < n; j++)
			for (uint32_t i = 0; i < n; i++) { g.xy.push_back(s[i]); g.xy.push_back(s[j]); }
		grids.push_back(g);
	}
	grids.push_back(random_grid(1, 23, 1, -1.0e6f, 1.0e6f, -1.0e9f, 1.0e9f));                          // far outside: REPEAT and MIRROR over many periods

	// (every build of the store: three types x two layouts; channels 1, 3 and 4)
	const Format formats[6] = { { 1, 0, 3 }, { 2, 1, 4 }, { 0, 1, 1 }, { 0, 0, 4 }, { 1, 1, 3 }, { 2, 0, 1 } };
	for (uint32_t filter = 0; filter < 2; filter++)
		for (uint32_t f = 0; f < 6; f++)
		{
			const uint32_t t = config * 12u + filter * 6u + f;
			const DecodeSampler smp = { filter, t & 3u, ((t >> 2) + t) & 3u };
			check_table(tag, img, blocks, whole, grids, batch[0], tile[0], formats[f], smp, t);
		}
}

/* 64 points at the block corners (bx i, by j), i, j even in 2 .. 16, of a 17 x 17-block image, BILINEAR: the four taps of a
 * point lie in four blocks and no two points share one -- 256 distinct blocks in one tile, eight full batches. */
static int corners(int bx, int by)
{
	const uint32_t ubx = (uint32_t)bx, uby = (uint32_t)by;
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	DecodeImage img = make_image(bx, by, 17u * ubx, 17u * uby, 1, 0, 0, tabs.data());
	std::vector<uint8_t> blocks, whole;
	random_blocks(blocks, (size_t)img.blocks_x * img.blocks_y);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	decode_whole(img, blocks, whole, batch[0]);
	Grid g = { 0, 64, 1, {} };
	for (uint32_t j = 2; j <= 16; j += 2)
		for (uint32_t i = 2; i <= 16; i += 2) { g.xy.push_back((float)(ubx * i)); g.xy.push_back((float)(uby * j)); }
	char tag[64];
	snprintf(tag, sizeof(tag), "%dx%d corners", bx, by);
	std::vector<SampleTileCount> per_tile;
	const Format f = { 1, 0, 3 };
	const DecodeSampler smp = { 1, 0, 0 };
	check_table(tag, img, blocks, whole, { g }, batch[0], tile[0], f, smp, 0, &per_tile);
	const bool ok = per_tile.size() == 1 && per_tile[0].batches == 8u && per_tile[0].blocks == 256u;
	printf("%s: tiles %zu batches %u blocks %u\n", tag, per_tile.size(), per_tile.empty() ? 0u : per_tile[0].batches, per_tile.empty() ? 0u : per_tile[0].blocks);
	if (!ok) fail("the corner tile does not run eight full batches of 256 blocks", tag, 0, 0);
	return ok ? 0 : 1;
}

/* The tables of a few hand-computed cases (6x6, a 230 x 50 x 2 U8 and a 100 x 30 F32 image): a line per table, then a line per tile. */
static int tables()
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 6, 6, 1);
	const DecodeImage images[2] = { make_image(6, 6, 230, 50, 2, 0, 0, tabs.data()), make_image(6, 6, 100, 30, 1, 0, 2, tabs.data()) };
	static uint8_t sink[16];
	static float xy[2];
	auto grid = [](uint32_t entry, uint32_t z, uint32_t ox, uint32_t oy, size_t crow, size_t row, size_t plane)
	{
		DecodeSampleLaunch g;
		memset(&g, 0, sizeof(g));
		g.entry = entry; g.z = z; g.out_x = ox; g.out_y = oy;
		g.d_coords = xy; g.coord_row_pitch = crow; g.d_out = sink; g.row_pitch = row; g.plane_pitch = plane;
		return g;
	};
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 1; format.layout = 1; format.channels = 3;
	const DecodeSampler smp = { 1, 2, 3 };
	const std::vector<DecodeSampleLaunch> grids = { grid(0, 1, 100, 1, 200, 300, 0), grid(1, 0, 33, 2, 70, 99, 0), grid(0, 0, 17, 3, 34, 51, 0), grid(1, 0, 9, 5, 18, 27, 0),
	                                                grid(0, 1, 20, 17, 40, 64, 0) };
	const std::vector<const uint8_t*> streams(2, nullptr);
	std::vector<uint8_t> table(decode_sample_bytes((uint32_t)grids.size()));
	const uint32_t total = decode_sample_build(table.data(), images, streams.data(), format, smp, grids.data(), (uint32_t)grids.size());
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeSampleRecord* rec = reinterpret_cast<const DecodeSampleRecord*>(table.data() + image_set_records_offset(head->count));
	printf("table: count %u total %u returned %u first", head->count, head->total, total);
	for (uint32_t i = 0; i < head->count; i++) printf(" %u", first[i]);
	printf(" records");
	for (uint32_t i = 0; i < head->count; i++)
		printf(" [tw %u th %u tiles_x %u dim_x %u data_type %u z %u out_x %u out_y %u coord_row %zu row %zu plane %zu x_step %u filter %u address_x %u address_y %u type %u layout %u channels %u]",
		       1u << rec[i].tw_log2, 64u >> rec[i].tw_log2, rec[i].tiles_x, rec[i].img.dim_x, rec[i].img.data_type, rec[i].z, rec[i].out_x, rec[i].out_y, rec[i].coord_row, rec[i].row,
		       rec[i].fmt.plane, rec[i].x_step, rec[i].filter, rec[i].address_x, rec[i].address_y, rec[i].fmt.type, rec[i].fmt.layout, rec[i].fmt.channels);
	printf("\n");
	// the taps of a few coordinates along an axis of 10 texels, under each address mode: "x: filter f mode m -> n [index weight] ..."
	const float xs[] = { 0.5f, 0.0f, -0.0f, 9.5f, 10.0f, 1e-30f, -3.25f };
	for (float x : xs)
		for (uint32_t filter = 0; filter < 2; filter++)
			for (uint32_t mode = 0; mode < 4; mode++)
			{
				const SampleAxis a = sample_axis(filter, x);
				printf("taps %a filter %u mode %u:", (double)x, filter, mode);
				for (uint32_t t = 0; t < a.n; t++)
				{
					uint32_t k = 0;
					const bool in = sample_address(mode, a.i0 + (int32_t)t, 10u, k);
					printf(" [%ld %a]", in ? (long)k : -1L, t == 0 ? a.w0 : a.w1);
				}
				printf("\n");
			}
	return 0;
}

/* `blocks <filter> <address_x> <address_y> <block_x> <block_y> <dim_x> <dim_y> <out_x> <out_y> <file>`: the tiles of the grid
 * whose out_x * out_y coordinate pairs (binary32, x then y, row by row) are the file's bytes, run over an image of constant-colour
 * blocks; prints the tiles, the batches and the blocks they decoded (tools/time_decode_sample.py). */
static int blocks_mode(char** a)
{
	const uint32_t filter = (uint32_t)atoi(a[0]), ax = (uint32_t)atoi(a[1]), ay = (uint32_t)atoi(a[2]), bx = (uint32_t)atoi(a[3]), by = (uint32_t)atoi(a[4]);
	const uint32_t dim_x = (uint32_t)atoi(a[5]), dim_y = (uint32_t)atoi(a[6]), ox = (uint32_t)atoi(a[7]), oy = (uint32_t)atoi(a[8]);
	if (filter > 1 || ax > 3 || ay > 3 || bx < 4 || bx > 12 || by < 4 || by > 12 || dim_x < 1 || dim_y < 1 || ox < 1 || ox > 65535 || oy < 1 || oy > 65535) return 2;
	std::vector<float> xy((size_t)ox * oy * 2u);
	FILE* fp = fopen(a[9], "rb");
	if (!fp || fread(xy.data(), sizeof(float), xy.size(), fp) != xy.size()) return 2;
	fclose(fp);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], (int)bx, (int)by, 1);
	const DecodeImage img = make_image((int)bx, (int)by, dim_x, dim_y, 1, 0, 0, tabs.data());
	const size_t nblocks = (size_t)img.blocks_x * img.blocks_y;
	std::vector<uint8_t> blocks(nblocks * 16, 0xFF);
	for (size_t b = 0; b < nblocks; b++) { blocks[b * 16] = 0xFC; blocks[b * 16 + 1] = 0xFD; }
	std::vector<uint16_t> out((size_t)ox * oy * 3u);
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 1; format.layout = 0; format.channels = 3;
	for (int c = 0; c < 3; c++) format.scale[c] = 1.0f;
	DecodeSampleLaunch g;
	memset(&g, 0, sizeof(g));
	g.out_x = ox; g.out_y = oy; g.d_coords = xy.data(); g.coord_row_pitch = 2u * (size_t)ox; g.d_out = out.data(); g.row_pitch = ox; g.plane_pitch = (size_t)ox * oy;
	const DecodeSampler smp = { filter, ax, ay };
	std::vector<uint8_t> table(decode_sample_bytes(1));
	const uint8_t* stream = blocks.data();
	const uint32_t tiles = decode_sample_build(table.data(), &img, &stream, format, smp, &g, 1);
	DecodeSampleRecord rec;
	memcpy(&rec, table.data() + image_set_records_offset(1), sizeof(rec));
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	unsigned long long batches = 0, decoded = 0;
	for (uint32_t t = 0; t < tiles; t++)
	{
		const SampleTileCount n = decode_sample_tile<1, 0>(rec, t, batch[0], tile[0]);
		batches += n.batches; decoded += n.blocks;
	}
	printf("tiles %u batches %llu decoded %llu points %llu\n", tiles, batches, decoded, (unsigned long long)ox * oy);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	if (argc == 12 && strcmp(argv[1], "blocks") == 0) return blocks_mode(argv + 2);
	const int footprints[4][2] = { { 4, 4 }, { 6, 6 }, { 10, 8 }, { 12, 12 } };
	uint32_t config = 0;
	for (const int* f : footprints)
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 3; dtype++) check(f[0], f[1], profile, dtype, config++);
	for (const int* f : footprints) corners(f[0], f[1]);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	printf("address mode pairs met: %d of 16\n", __builtin_popcount(g_pairs_seen));
	printf("%llu blocks decoded in %llu batches\n", g_decoded, g_batches);
	return g_bad == 0 ? 0 : 1;
}
