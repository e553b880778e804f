// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the tensor decode of astcenc_amd_decompress_tensors_device (decode_tensors.h: the host-built table,
// decode_tensor_run over TensorWindow and TensorStore) against decode_row_batch of the whole image followed by a crop, a
// conversion and a placement written out in plain C++ below, on the host, as sequential code under the sanitizers.  Random
// 16-byte patterns mixed with constant-colour blocks (UNORM16 and FP16) and reserved-mode blocks; footprints 4x4, 6x6, 12x12 and
// 3x3x3; the three data types, the four profiles, an identity, a BGRA and the Z swizzle; images 34 blocks wide, the last block
// partial on every axis, two block rows and two slices / layers.  Each image is decoded with six formats -- F16 planar 3
// channels, BF16 interleaved 4, F32 interleaved 1, F32 planar 4, F16 interleaved 3, BF16 planar 1: every type with both layouts --
// and per format one table of all its windows, each once tight and once with
// padded row, slice and plane pitches; the flips rotate through the four states from window to window.  Required: every element
// of every window equal to the model's bits, every other byte of every buffer (guards in front, behind, in the padding and
// between planes) intact, the inputs unchanged, as many runs as the table says and as the windows' covered blocks need.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_tensor_check.cpp -o decode_tensor_check
// `decode_tensor_check tables` prints the tables of a few hand-computed cases instead (tests/test_decode_tensors_cpu.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_tensors.h"
#include "decode_check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>

struct Window { uint32_t x, y, z, sx, sy, sz; };

static void check_format(const char* image_tag, const DecodeImage& img, const std::vector<uint8_t>& blocks, const std::vector<uint8_t>& whole,
                         const std::vector<Window>& windows, DecodeBatch& batch, const Format& f, uint32_t flip0)
{
	char tag[192];
	snprintf(tag, sizeof(tag), "%s -> type %u layout %u channels %u", image_tag, f.type, f.layout, f.channels);
	const uint32_t dim_x = img.dim_x, dim_y = img.dim_y, dtype = img.data_type;
	const size_t tb = dtype == 0 ? 4 : dtype == 1 ? 8 : 16, eb = f.type == 0 ? 4 : 2;
	const bool planar = f.layout == 0;
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = f.type; format.layout = f.layout; format.channels = f.channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 1.0f / 255.0f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }

	// one call: every window once tight, once with a row pitch padded by 3 elements, a slice pitch by one row, a plane pitch by 5 elements
	const size_t guard = 64;
	const uint32_t count = (uint32_t)windows.size() * 2u;
	std::vector<DecodeTensorLaunch> regions(count);
	std::vector<std::vector<uint8_t>> outs(count);
	for (uint32_t i = 0; i < count; i++)
	{
		const Window& w = windows[i / 2];
		const bool padded = (i & 1u) != 0u;
		const size_t row = (size_t)w.sx * (planar ? 1 : f.channels) + (padded ? 3 : 0), slice = row * ((size_t)w.sy + (padded ? 1 : 0));
		const size_t plane = planar ? slice * w.sz + (padded ? 5 : 0) : 0;
		const size_t elements = planar ? plane * f.channels : slice * w.sz;
		outs[i].assign(guard + elements * eb + guard, 0xA5);
		DecodeTensorLaunch& r = regions[i];
		r.entry = 0;
		r.x = w.x; r.y = w.y; r.z = w.z; r.size_x = w.sx; r.size_y = w.sy; r.size_z = w.sz;
		r.flags = (flip0 + i / 2) & 3u;
		r.d_out = outs[i].data() + guard;
		r.row_pitch = row; r.slice_pitch = slice; r.plane_pitch = plane;
	}
	std::vector<uint8_t> table(decode_tensors_bytes(count));
	const uint8_t* stream = blocks.data();
	const uint32_t total = decode_tensors_build(table.data(), &img, &stream, format, regions.data(), count);
	const std::vector<uint8_t> table_before = table, blocks_before = blocks;

	uint32_t want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Window& w = windows[i / 2];
		const uint32_t ubx = img.block_x, uby = img.block_y, ubz = img.block_z;
		const uint32_t cols = (w.x + w.sx - 1) / ubx - w.x / ubx + 1, rows = (w.y + w.sy - 1) / uby - w.y / uby + 1, layers = (w.z + w.sz - 1) / ubz - w.z / ubz + 1;
		want_total += ((cols + DECODE_BATCH - 1) / DECODE_BATCH) * rows * layers;
	}

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeTensorRecord rec = image_set_record<DecodeTensorRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeTensorRecord)));
		// (the kernel build the host picks for the format)
		const uint32_t local = r - first[g];
		switch (rec.fmt.type * 2u + rec.fmt.layout)
		{
		case 0: decode_tensor_run<0, 0>(rec, local, batch); break;
		case 1: decode_tensor_run<0, 1>(rec, local, batch); break;
		case 2: decode_tensor_run<1, 0>(rec, local, batch); break;
		case 3: decode_tensor_run<1, 1>(rec, local, batch); break;
		case 4: decode_tensor_run<2, 0>(rec, local, batch); break;
		default: decode_tensor_run<2, 1>(rec, local, batch); break;
		}
	}
	if (blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);

	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeTensorLaunch& r = regions[i];
		const std::vector<uint8_t>& o = outs[i];
		std::vector<uint8_t> want(o.size(), 0xA5);
		for (uint32_t k = 0; k < r.size_z; k++)
			for (uint32_t j = 0; j < r.size_y; j++)
				for (uint32_t x = 0; x < r.size_x; x++)
				{
					const uint8_t* texel = whole.data() + ((((size_t)(r.z + k) * dim_y + (r.y + j)) * dim_x) + r.x + x) * tb;
					const uint32_t xo = (r.flags & 1u) ? r.size_x - 1u - x : x, yo = (r.flags & 2u) ? r.size_y - 1u - j : j;
					for (uint32_t c = 0; c < f.channels; c++)
					{
						const uint32_t bits = model_bits((float)source_value(texel, dtype, c), format.scale[c], format.bias[c], f.type);
						const size_t at = planar ? c * r.plane_pitch + k * r.slice_pitch + yo * r.row_pitch + xo : k * r.slice_pitch + yo * r.row_pitch + (size_t)xo * f.channels + c;
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
	const std::vector<Window> windows = {
		{ 0, 0, 0, dim_x, dim_y, dim_z },                                           // the whole image
		{ dim_x / 2, dim_y / 2, dim_z - 1, 1, 1, 1 },                               // one texel
		{ 3 * ubx + 1, uby + 1, 0, in_x, in_y, 1 },                                 // inside one block
		{ ubx / 2, uby / 2, 0, 33 * ubx, uby, 1 },                                  // mid-block to mid-block over 34 blocks and both block rows: two runs a row
		{ ubx + 1, 0, dim_z - 1, 70, uby + 1, 1 },                                  // more than 64 texels wide: two trips
		{ dim_x - 5, dim_y - 2, dim_z - 1, 5, 2, 1 },                               // ends in the partial last block of every axis
		bz == 1 ? Window{ 2 * ubx + 1, 1, 0, 3 * ubx, uby, 2 }                      // two array slices
		        : Window{ 2 * ubx + 1, 1, ubz - 1, 3 * ubx, uby, 2 },               // ... two layers of blocks
	};
	// (every build of the sink: three types x two layouts; channels 1, 3 and 4; the vector store and the per-channel ones of both widths)
	const Format formats[6] = { { 1, 0, 3 }, { 2, 1, 4 }, { 0, 1, 1 }, { 0, 0, 4 }, { 1, 1, 3 }, { 2, 0, 1 } };
	for (uint32_t f = 0; f < 6; f++) check_format(tag, img, blocks, whole, windows, batch[0], formats[f], f);
}

/* The tables of a few hand-computed cases (6x6, a 230 x 50 x 2 and a 100 x 30 image), one line each. */
static void print_table(const char* name, const DecodeImage* images, uint32_t entries, const DecodeTensorFormat& format, const std::vector<DecodeTensorLaunch>& regions)
{
	std::vector<const uint8_t*> streams(entries, nullptr);
	std::vector<uint8_t> table(decode_tensors_bytes((uint32_t)regions.size()));
	const uint32_t total = decode_tensors_build(table.data(), images, streams.data(), format, regions.data(), (uint32_t)regions.size());
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeTensorRecord* rec = reinterpret_cast<const DecodeTensorRecord*>(table.data() + image_set_records_offset(head->count));
	printf("%s: count %u total %u returned %u first", name, head->count, head->total, total);
	for (uint32_t i = 0; i < head->count; i++) printf(" %u", first[i]);
	printf(" records");
	for (uint32_t i = 0; i < head->count; i++)
		printf(" [bx0 %u by0 %u bz0 %u cols %u runs_x %u runs_xy %u dim_x %u row %zu slice %zu plane %zu x_step %u flags %u type %u layout %u channels %u]", rec[i].bx0,
		       rec[i].by0, rec[i].bz0, rec[i].cols, rec[i].runs_x, rec[i].runs_xy, rec[i].img.dim_x, rec[i].win.w.row_texels, rec[i].win.w.slice_texels, rec[i].fmt.plane,
		       rec[i].win.x_step, rec[i].win.flags, rec[i].fmt.type, rec[i].fmt.layout, rec[i].fmt.channels);
	printf("\n");
}

static int tables()
{
	const uint32_t rgba[4] = { 0, 1, 2, 3 };
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 6, 6, 1);
	const DecodeImage images[2] = { make_image(6, 6, 1, 230, 50, 2, 0, 0, rgba, tabs.data()), make_image(6, 6, 1, 100, 30, 1, 0, 1, rgba, tabs.data()) };
	static uint8_t sink[16];
	auto region = [](uint32_t entry, uint32_t x, uint32_t y, uint32_t z, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t flags, size_t row, size_t slice, size_t plane)
	{
		DecodeTensorLaunch r;
		memset(&r, 0, sizeof(r));
		r.entry = entry; r.x = x; r.y = y; r.z = z; r.size_x = sx; r.size_y = sy; r.size_z = sz; r.flags = flags;
		r.d_out = sink; r.row_pitch = row; r.slice_pitch = slice; r.plane_pitch = plane;
		return r;
	};
	DecodeTensorFormat planar3, inter4;
	memset(&planar3, 0, sizeof(planar3)); memset(&inter4, 0, sizeof(inter4));
	planar3.type = 1; planar3.layout = 0; planar3.channels = 3;
	inter4.type = 2; inter4.layout = 1; inter4.channels = 4;
	print_table("planar", images, 2, planar3, { region(0, 6, 0, 0, 192, 6, 1, 1, 192, 1152, 1152), region(0, 5, 5, 0, 193, 2, 1, 2, 200, 400, 500), region(1, 94, 29, 0, 6, 1, 1, 0, 6, 6, 6) });
	print_table("interleaved", images, 2, inter4, { region(0, 0, 0, 0, 230, 50, 2, 3, 920, 46000, 0), region(1, 7, 7, 0, 1, 1, 1, 0, 4, 4, 0) });
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	const int footprints[4][3] = { { 4, 4, 1 }, { 6, 6, 1 }, { 12, 12, 1 }, { 3, 3, 3 } };
	const uint32_t swizzles[3][4] = { { 0, 1, 2, 3 }, { 2, 1, 0, 3 }, { 0, 3, 6, 5 } };     // identity, BGRA, a normal map's: r, a, the reconstructed z, 1
	for (const int* f : footprints)
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 3; dtype++)
				for (const uint32_t* swz : swizzles) check(f[0], f[1], f[2], profile, dtype, swz);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	return g_bad == 0 ? 0 : 1;
}
