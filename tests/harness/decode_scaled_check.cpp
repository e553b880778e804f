// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the scaled tensor decode of astcenc_amd_decompress_scaled_tensors_device (decode_scaled.h: the host-built
// table, decode_scaled_tile over ScaledWindow and ScaledStage) against decode_row_batch of the whole image followed by the
// filter, the conversion and the placement written out in plain C++ below from the header's definition, on the host, as
// sequential code under the sanitizers.  Random 16-byte patterns mixed with constant-colour blocks (UNORM16 and FP16) and
// reserved-mode blocks; footprints 4x4, 6x6, 10x8 and 12x12; the three data types, the four profiles; images of 33 blocks and
// three texels by two block rows and one texel, two slices.  Each image is resampled with both filters and six formats -- every
// tensor type with both layouts -- and per (filter, format) one table of all its regions: a wide image to more than 64 columns
// and to one element, ratio 1, down along one axis and up along the other, windows of one and of 3 x 3 texels enlarged, a
// window that ends at the image's last texel; tight and padded pitches alternate, the flips rotate.  Required: every element of
// every region equal to the model's bits, every other byte of every buffer intact, the inputs unchanged, as many tiles as the
// regions' output sizes need.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_scaled_check.cpp -o decode_scaled_check
// `decode_scaled_check tables` prints the tables of a few hand-computed cases instead, `sweep` checks the tiling's promise over
// sizes, footprints and data types (tests/test_decode_scaled_cpu.py); `blocks` counts the blocks the tiles of given windows decode
// (tools/time_decode_scaled.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_scaled.h"
#include "decode_check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned long long g_decoded = 0;

/* The model (include/astcenc_amd.h), one operation at a time: a texel's component widened (source_value, decode_check_common.h) ... */
/* ... the taps of output position p along an axis: indices and weights in tap order, zero weights left out ... */
struct Tap { uint32_t k; uint32_t w; };
static int model_taps(uint32_t filter, uint32_t S, uint32_t D, uint32_t p, std::vector<Tap>& taps, uint32_t& den)
{
	taps.clear();
	if (filter == 0)
	{
		const int64_t n = (2 * (int64_t)p + 1) * (int64_t)S - (int64_t)D, d2 = 2 * (int64_t)D;
		int64_t i0 = n / d2;
		if (n % d2 != 0 && n < 0) i0--;                        // floor
		const int64_t f = n - i0 * d2;
		auto clamp = [S](int64_t v) { return (uint32_t)(v < 0 ? 0 : v > (int64_t)S - 1 ? (int64_t)S - 1 : v); };
		taps.push_back({ clamp(i0), (uint32_t)(d2 - f) });
		if (f != 0) taps.push_back({ clamp(i0 + 1), (uint32_t)f });
		den = (uint32_t)d2;
	}
	else
	{
		const uint64_t a = (uint64_t)p * S, b = a + S;
		for (uint64_t k = a / D; k <= (b - 1) / D; k++)
		{
			const uint64_t hi = b < (k + 1) * D ? b : (k + 1) * D, lo = a > k * D ? a : k * D;
			taps.push_back({ (uint32_t)k, (uint32_t)(hi - lo) });
		}
		den = S;
	}
	return (int)taps.size();
}

struct Region { uint32_t x, y, z, sx, sy, ox, oy; };

static void check_format(const char* image_tag, const DecodeImage& img, const std::vector<uint8_t>& blocks, const std::vector<uint8_t>& whole,
                         const std::vector<Region>& wanted, DecodeBatch& batch, ScaledTile& tile, const Format& f, uint32_t filter, uint32_t flip0)
{
	char tag[224];
	snprintf(tag, sizeof(tag), "%s -> filter %u type %u layout %u channels %u", image_tag, filter, f.type, f.layout, f.channels);
	const uint32_t dim_x = img.dim_x, dim_y = img.dim_y, dtype = img.data_type;
	const size_t tb = dtype == 0 ? 4 : dtype == 1 ? 8 : 16, eb = f.type == 0 ? 4 : 2;
	const bool planar = f.layout == 0;
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = f.type; format.layout = f.layout; format.channels = f.channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 1.0f / 255.0f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }

	const size_t guard = 64;
	const uint32_t count = (uint32_t)wanted.size();
	std::vector<DecodeScaledLaunch> regions(count);
	std::vector<std::vector<uint8_t>> outs(count);
	unsigned long long want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Region& w = wanted[i];
		const bool padded = ((i + flip0) & 1u) != 0u;
		const size_t row = (size_t)w.ox * (planar ? 1 : f.channels) + (padded ? 3 : 0);
		const size_t plane = planar ? row * w.oy + (padded ? 5 : 0) : 0;
		const size_t elements = planar ? plane * f.channels : row * w.oy;
		outs[i].assign(guard + elements * eb + guard, 0xA5);
		DecodeScaledLaunch& r = regions[i];
		memset(&r, 0, sizeof(r));
		r.entry = 0;
		r.x = w.x; r.y = w.y; r.z = w.z; r.size_x = w.sx; r.size_y = w.sy; r.out_x = w.ox; r.out_y = w.oy;
		r.flags = (flip0 + i) & 3u;
		r.d_out = outs[i].data() + guard;
		r.row_pitch = row; r.plane_pitch = plane;
		// (the tiles, spelled out: a run of n blocks holds (n - 1) block_x + 1 texels wherever they start, c columns reach c S / D + 3)
		const uint32_t band = w.oy < 8 ? w.oy : 8;
		const uint32_t fit = 6144u / (uint32_t)tb / (img.block_x * img.block_y), run = fit < 32u ? fit : 32u, hold = (run - 1u) * img.block_x + 1u;
		const uint64_t c = hold > 3u ? (uint64_t)(hold - 3u) * w.ox / w.sx : 0u;
		const uint32_t cols = c >= 64u ? 64u : c >= 8u ? (uint32_t)c : 8u;
		want_total += (unsigned long long)((w.ox + cols - 1u) / cols) * ((w.oy + band - 1) / band);
	}
	std::vector<uint8_t> table(decode_scaled_bytes(count));
	const uint8_t* stream = blocks.data();
	const uint32_t total = decode_scaled_build(table.data(), &img, &stream, format, filter, regions.data(), count);
	const std::vector<uint8_t> table_before = table, blocks_before = blocks;

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	// (the LDS of a fresh workgroup holds anything)
	memset(static_cast<void*>(&tile), 0xCD, sizeof(ScaledTile));
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeScaledRecord rec = image_set_record<DecodeScaledRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeScaledRecord)));
		const uint32_t local = r - first[g];
		uint32_t decoded;
		switch (rec.fmt.type * 2u + rec.fmt.layout)
		{
		case 0: decoded = decode_scaled_tile<0, 0>(rec, local, batch, tile); break;
		case 1: decoded = decode_scaled_tile<0, 1>(rec, local, batch, tile); break;
		case 2: decoded = decode_scaled_tile<1, 0>(rec, local, batch, tile); break;
		case 3: decoded = decode_scaled_tile<1, 1>(rec, local, batch, tile); break;
		case 4: decoded = decode_scaled_tile<2, 0>(rec, local, batch, tile); break;
		default: decoded = decode_scaled_tile<2, 1>(rec, local, batch, tile); break;
		}
		// (the count the `blocks` and `sweep` modes go by is the one the tile routine makes)
		if (decoded != decode_scaled_tile_blocks(rec, local)) fail("the blocks a tile decoded are not decode_scaled_tile_blocks", tag, g, (long)local);
		g_decoded += decoded;
	}
	if (blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);

	std::vector<Tap> tx, ty;
	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeScaledLaunch& r = regions[i];
		const std::vector<uint8_t>& o = outs[i];
		std::vector<uint8_t> want(o.size(), 0xA5);
		for (uint32_t j = 0; j < r.out_y; j++)
			for (uint32_t x = 0; x < r.out_x; x++)
			{
				uint32_t den_x, den_y;
				model_taps(filter, r.size_x, r.out_x, x, tx, den_x);
				model_taps(filter, r.size_y, r.out_y, j, ty, den_y);
				const uint32_t xo = (r.flags & 1u) ? r.out_x - 1u - x : x, yo = (r.flags & 2u) ? r.out_y - 1u - j : j;
				for (uint32_t c = 0; c < f.channels; c++)
				{
					volatile double acc = 0.0;
					for (size_t b = 0; b < ty.size(); b++)
					{
						volatile double row = 0.0;
						for (size_t a = 0; a < tx.size(); a++)
						{
							const uint8_t* texel = whole.data() + ((((size_t)r.z * dim_y + (r.y + ty[b].k)) * dim_x) + r.x + tx[a].k) * tb;
							volatile double p = (double)tx[a].w * source_value(texel, dtype, c);
							row = a == 0 ? p : row + p;
						}
						volatile double p = (double)ty[b].w * row;
						acc = b == 0 ? p : acc + p;
					}
					volatile double quotient = acc / ((double)den_x * (double)den_y);
					const uint32_t bits = model_bits((float)quotient, format.scale[c], format.bias[c], f.type);
					const size_t at = planar ? c * r.plane_pitch + yo * r.row_pitch + xo : yo * r.row_pitch + (size_t)xo * f.channels + c;
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

static void check(int bx, int by, int profile, uint32_t dtype)
{
	const uint32_t ubx = (uint32_t)bx, uby = (uint32_t)by;
	const uint32_t dim_x = 33u * ubx + 3u, dim_y = 2u * uby + 1u, dim_z = 2u;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%d %ux%ux%u profile %d type %u", bx, by, dim_x, dim_y, dim_z, profile, dtype);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	DecodeImage img = make_image(bx, by, dim_x, dim_y, dim_z, profile, dtype, tabs.data());
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

	// the whole image, as the decoder writes it
	std::vector<uint8_t> whole(texels * tb, 0x5A);
	img.data = whole.data();
	std::vector<DecodeBatch> batch(1);
	std::vector<ScaledTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	for (uint32_t z = 0; z < img.blocks_z; z++)
		for (uint32_t y = 0; y < img.blocks_y; y++)
			for (uint32_t x0 = 0; x0 < img.blocks_x; x0 += DECODE_BATCH)
				decode_row_batch(img, blocks.data(), x0, y, z, i_min(DECODE_BATCH, (int)(img.blocks_x - x0)), batch[0]);
	img.data = nullptr;

	const std::vector<Region> regions = {
		{ 0, 0, 0, dim_x, dim_y, 130, 5 },                                          // the whole image: more than 64 columns, more than 32 blocks under a row
		{ 0, 0, 1, dim_x, dim_y, 1, 1 },                                            // ... to one element
		{ ubx / 2, 1, 0, 37, uby + 2, 37, uby + 2 },                                // ratio 1, mid-block, both block rows
		{ ubx + 1, 0, 1, 37, 5, 23, 11 },                                           // down along x, up along y
		{ 3, 2, 0, 23, uby + 3, 37, 3 },                                            // up along x, down along y
		{ dim_x / 2, dim_y / 2, 1, 1, 1, 5, 3 },                                    // one texel: everything clamps
		{ 2 * ubx - 1, uby - 1, 0, 3, 3, 17, 11 },                                  // 3 x 3 across a block corner, two bands
		{ dim_x - 10, dim_y - 4, 1, 10, 4, 7, 9 },                                  // ends at the image's last texel, in the partial blocks
	};
	// (every build of the store: three types x two layouts; channels 1, 3 and 4)
	const Format formats[6] = { { 1, 0, 3 }, { 2, 1, 4 }, { 0, 1, 1 }, { 0, 0, 4 }, { 1, 1, 3 }, { 2, 0, 1 } };
	for (uint32_t filter = 0; filter < 2; filter++)
		for (uint32_t f = 0; f < 6; f++) check_format(tag, img, blocks, whole, regions, batch[0], tile[0], formats[f], filter, f + filter);
}

/* The tables of a few hand-computed cases (6x6, a 230 x 50 x 2 U8 and a 100 x 30 F32 image): a line per table, then a line per tile. */
static void print_table(const char* name, const DecodeImage* images, uint32_t entries, const DecodeTensorFormat& format, uint32_t filter,
                        const std::vector<DecodeScaledLaunch>& regions)
{
	std::vector<const uint8_t*> streams(entries, nullptr);
	std::vector<uint8_t> table(decode_scaled_bytes((uint32_t)regions.size()));
	const uint32_t total = decode_scaled_build(table.data(), images, streams.data(), format, filter, regions.data(), (uint32_t)regions.size());
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeScaledRecord* rec = reinterpret_cast<const DecodeScaledRecord*>(table.data() + image_set_records_offset(head->count));
	printf("%s: count %u total %u returned %u first", name, head->count, head->total, total);
	for (uint32_t i = 0; i < head->count; i++) printf(" %u", first[i]);
	printf(" records");
	for (uint32_t i = 0; i < head->count; i++)
		printf(" [cols %u strips %u band %u run_blocks %u dim_x %u x %u y %u z %u size_x %u size_y %u out_x %u out_y %u row %zu plane %zu x_step %u flags %u filter %u type %u layout %u channels %u]",
		       rec[i].cols, rec[i].strips, rec[i].band, rec[i].run_blocks, rec[i].img.dim_x, rec[i].x, rec[i].y, rec[i].z, rec[i].size_x, rec[i].size_y, rec[i].out_x, rec[i].out_y,
		       rec[i].row, rec[i].fmt.plane, rec[i].x_step, rec[i].flags, rec[i].filter, rec[i].fmt.type, rec[i].fmt.layout, rec[i].fmt.channels);
	printf("\n");
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const ScaledTileRect q = decode_scaled_rect(rec[g], r - first[g]);
		printf("%s tile %u: region %u [c0 %u nc %u r0 %u nr %u sx0 %u sx1 %u sy0 %u sy1 %u]\n", name, r, g, q.c0, q.nc, q.r0, q.nr, q.sx0, q.sx1, q.sy0, q.sy1);
	}
}

static int tables()
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 6, 6, 1);
	const DecodeImage images[2] = { make_image(6, 6, 230, 50, 2, 0, 0, tabs.data()), make_image(6, 6, 100, 30, 1, 0, 2, tabs.data()) };
	static uint8_t sink[16];
	auto region = [](uint32_t entry, uint32_t x, uint32_t y, uint32_t z, uint32_t sx, uint32_t sy, uint32_t ox, uint32_t oy, uint32_t flags, size_t row, size_t plane)
	{
		DecodeScaledLaunch r;
		memset(&r, 0, sizeof(r));
		r.entry = entry; r.x = x; r.y = y; r.z = z; r.size_x = sx; r.size_y = sy; r.out_x = ox; r.out_y = oy; r.flags = flags;
		r.d_out = sink; r.row_pitch = row; r.plane_pitch = plane;
		return r;
	};
	DecodeTensorFormat planar3, inter4;
	memset(&planar3, 0, sizeof(planar3)); memset(&inter4, 0, sizeof(inter4));
	planar3.type = 1; planar3.layout = 0; planar3.channels = 3;
	inter4.type = 2; inter4.layout = 1; inter4.channels = 4;
	print_table("bilinear", images, 2, planar3, 0,
	            { region(0, 6, 0, 0, 192, 48, 224, 20, 1, 224, 4480), region(1, 10, 5, 0, 37, 23, 23, 37, 2, 30, 1200), region(0, 229, 49, 1, 1, 1, 5, 3, 0, 5, 15) });
	print_table("box", images, 2, inter4, 1, { region(0, 0, 0, 0, 230, 50, 3, 2, 3, 12, 0), region(1, 94, 24, 0, 6, 6, 4, 9, 0, 16, 0) });
	return 0;
}

/* One region's record, as decode_scaled_build makes it, without a stream or a buffer. */
static DecodeScaledRecord record_of(const DecodeImage& img, uint32_t filter, uint32_t x, uint32_t y, uint32_t sx, uint32_t sy, uint32_t ox, uint32_t oy, uint32_t& tiles)
{
	static uint8_t sink[16];
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 1; format.layout = 0; format.channels = 3;
	DecodeScaledLaunch r;
	memset(&r, 0, sizeof(r));
	r.x = x; r.y = y; r.size_x = sx; r.size_y = sy; r.out_x = ox; r.out_y = oy;
	r.d_out = sink; r.row_pitch = ox; r.plane_pitch = (size_t)ox * oy;
	std::vector<uint8_t> table(decode_scaled_bytes(1));
	const uint8_t* stream = nullptr;
	tiles = decode_scaled_build(table.data(), &img, &stream, format, filter, &r, 1);
	DecodeScaledRecord rec;
	memcpy(&rec, table.data() + image_set_records_offset(1), sizeof(rec));
	return rec;
}

/* The tiling's promise (decode_scaled_tiling), checked tile by tile: a tile wider than SCALED_CARRY columns decodes every block
 * row in one run.  Footprints x data types x both filters x window widths 1 .. 700 and a few large ones x output widths 1 .. 300
 * and a few large ones x origins 0 .. block_x - 1 (every alignment of the window to the blocks). */
static int sweep()
{
	const int footprints[5][2] = { { 4, 4 }, { 6, 6 }, { 10, 8 }, { 12, 12 }, { 5, 4 } };
	std::vector<uint32_t> sizes, outs;
	for (uint32_t v = 1; v <= 700; v += v < 70 ? 1 : 13) sizes.push_back(v);
	for (uint32_t v : { 1023u, 4097u, 65535u }) sizes.push_back(v);
	for (uint32_t v = 1; v <= 300; v += v < 70 ? 1 : 7) outs.push_back(v);
	for (uint32_t v : { 1000u, 65535u }) outs.push_back(v);
	unsigned long long tiles_checked = 0, wide = 0, broken = 0;
	for (const int* f : footprints)
		for (uint32_t dtype = 0; dtype < 3; dtype++)
		{
			const DecodeImage img = make_image(f[0], f[1], 70000, 64, 1, 0, dtype, nullptr);
			for (uint32_t filter = 0; filter < 2; filter++)
				for (uint32_t S : sizes)
					for (uint32_t D : outs)
						for (uint32_t x = 0; x < (uint32_t)f[0]; x += (S > 700 || D > 300) ? (uint32_t)f[0] - 1u : 1u)
						{
							uint32_t tiles;
							const DecodeScaledRecord rec = record_of(img, filter, x, 0, S, 1, D, 1, tiles);
							if (tiles != rec.strips || rec.cols < (uint32_t)SCALED_CARRY || rec.cols > (uint32_t)SCALED_COLS || rec.run_blocks < 1 || rec.run_blocks > (uint32_t)DECODE_BATCH) broken++;
							for (uint32_t t = 0; t < tiles; t++)
							{
								uint32_t widest;
								decode_scaled_tile_blocks(rec, t, &widest);
								const ScaledTileRect q = decode_scaled_rect(rec, t);
								tiles_checked++;
								if (q.nc <= (uint32_t)SCALED_CARRY) continue;
								wide++;
								if (widest > rec.run_blocks && ++broken <= 10)
									fprintf(stderr, "%dx%d type %u filter %u x %u S %u D %u tile %u: %u blocks in a block row, a run is %u\n", f[0], f[1], dtype, filter, x, S, D, t, widest, rec.run_blocks);
							}
						}
		}
	printf("%llu tiles, %llu wider than %d columns, %llu broken\n", tiles_checked, wide, SCALED_CARRY, broken);
	return broken == 0 ? 0 : 1;
}

/* `blocks <filter> <block_x> <block_y> <data type> <out_x> <out_y>`: for the windows "x y size_x size_y" on standard input, the
 * blocks the tiles of all of them decode and the blocks the windows cover (tools/time_decode_scaled.py). */
static int blocks_mode(char** a)
{
	const uint32_t filter = (uint32_t)atoi(a[0]), bx = (uint32_t)atoi(a[1]), by = (uint32_t)atoi(a[2]), dtype = (uint32_t)atoi(a[3]), ox = (uint32_t)atoi(a[4]), oy = (uint32_t)atoi(a[5]);
	if (filter > 1 || bx < 4 || bx > 12 || by < 4 || by > 12 || dtype > 2 || ox < 1 || ox > 65535 || oy < 1 || oy > 65535) return 2;
	const DecodeImage img = make_image((int)bx, (int)by, 1u << 20, 1u << 20, 1, 0, dtype, nullptr);
	unsigned long long decoded = 0, covered = 0, tiles_all = 0;
	uint32_t x, y, sx, sy;
	while (scanf("%u %u %u %u", &x, &y, &sx, &sy) == 4)
	{
		if (sx < 1 || sx > 65535 || sy < 1 || sy > 65535) return 2;
		uint32_t tiles;
		const DecodeScaledRecord rec = record_of(img, filter, x, y, sx, sy, ox, oy, tiles);
		for (uint32_t t = 0; t < tiles; t++) decoded += decode_scaled_tile_blocks(rec, t);
		covered += (unsigned long long)((x + sx - 1) / bx - x / bx + 1) * ((y + sy - 1) / by - y / by + 1);
		tiles_all += tiles;
	}
	printf("decoded %llu covered %llu tiles %llu\n", decoded, covered, tiles_all);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	if (argc > 1 && strcmp(argv[1], "sweep") == 0) return sweep();
	if (argc == 8 && strcmp(argv[1], "blocks") == 0) return blocks_mode(argv + 2);
	const int footprints[4][2] = { { 4, 4 }, { 6, 6 }, { 10, 8 }, { 12, 12 } };
	for (const int* f : footprints)
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 3; dtype++) check(f[0], f[1], profile, dtype);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	printf("%llu blocks decoded\n", g_decoded);
	return g_bad == 0 ? 0 : 1;
}
