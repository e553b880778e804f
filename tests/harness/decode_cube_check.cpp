// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the cube sampler of astcenc_amd_sample_cube_tensors_device (decode_cube.h: the host-built table, the
// coordinate stage -- cube_valid, cube_face, the quotients, cube_coordinate, cube_point_taps -- and decode_cube_tile on
// decode_lod.h's level walk) on the host, as sequential code under the sanitizers.  The model is tests/sample_cube_model.py: this
// program computes and prints or writes what the header's routines give, tests/test_decode_cube_cpu.py compares.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_cube_check.cpp -o decode_cube_check
// `points <file> <n>`: for each of the n directions (binary32 triples) of the file a line
//     D i valid valid_with_nan_lambda face sc tc ma p q                        (hex floats; face -1 and zeros when invalid)
//   and, when valid, for each face size s in 1, 2, 3, 5, 8, 64 and each filter a line
//     T i s filter x y nx ny wx0 wx1 wy0 wy1 then per tap slot: face tx ty     (-1 -1 -1: no such tap)
//   the taps read back from SamplePoint::blk and txy of cube 1 of a 5x4-block image of 12 layers.
// `tiles <bx> <by> <profile> <kind> <seed> <s0> <levels> <cube> <filter> <mip> <type> <layout> <channels> <ox> <oy> <dirs> <lod>
//        <bias> <pads> <prefix>`: a chain of `levels` levels of faces s0 >> l (at least 1), 12 layers each, every level a random
//   stream of its own (kind 0 U8, 1 F16, 2 F32, 3 the three in turn) with constant-colour and reserved-mode blocks; the grid's
//   directions and levels of detail (lod "-": NULL) are the files' bytes; pads: bit 0 a padded output, bit 1 padded rows of
//   directions, bit 2 padded rows of lod (the padding holds NaNs).  Writes what the decoder gives for every whole level to
//   <prefix>.level<l> and the guard-filled output buffer after all tiles to <prefix>.out; prints "level l s dtype", "out guard row
//   plane elements" and per tile "tile t passes batches blocks mask most" (most: the most blocks one pass listed).
// `blocks <filter> <mip> <bx> <by> <s> <levels> <ox> <oy> <dirs> <lod>`: the tiles of one grid over the first `levels` levels of
//   the chain of a cube of s x s faces of constant-colour blocks; prints tiles, passes, batches, blocks decoded
//   (tools/time_decode_cube.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_cube.h"
#define DECODE_CHECK_ITEM "grid"
#include "decode_lod_check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int points_mode(char** a)
{
	const uint32_t n = (uint32_t)atoi(a[1]);
	std::vector<float> d((size_t)n * 3u);
	if (!read_floats(a[0], d)) return 2;
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 5, 4, 1);
	const uint32_t sizes[6] = { 1, 2, 3, 5, 8, 64 };
	const float nan = __builtin_nanf("");
	for (uint32_t i = 0; i < n; i++)
	{
		const float dx = d[3u * i], dy = d[3u * i + 1u], dz = d[3u * i + 2u];
		const bool ok = cube_valid(dx, dy, dz, 0.0f);
		if (!ok)
		{
			printf("D %u 0 %d -1 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0\n", i, cube_valid(dx, dy, dz, nan) ? 1 : 0);
			continue;
		}
		const CubeFace f = cube_face(dx, dy, dz);
		// (the quotients as the tile routine keeps them)
		std::vector<float> one = { dx, dy, dz };
		DecodeCubeRecord rec;
		memset(static_cast<void*>(&rec), 0, sizeof(rec));
		rec.dirs = one.data(); rec.dir_row = 3;
		const CubeAt at = CubePoints::read(rec, 0, 0);
		printf("D %u 1 %d %d %a %a %a %a %a\n", i, cube_valid(dx, dy, dz, nan) ? 1 : 0, (int)at.face, (double)f.sc, (double)f.tc, (double)f.ma, at.p, at.q);
		if (at.face != f.face || !CubePoints::valid(at, 0.0f) || CubePoints::valid(at, nan)) return 3;
		for (uint32_t s : sizes)
			for (uint32_t filter = 0; filter < 2; filter++)
			{
				const DecodeImage img = make_image(5, 4, s, s, 12, 0, 0, tabs.data());
				const double x = cube_coordinate(at.p, s), y = cube_coordinate(at.q, s);
				SamplePoint P;
				P.live = 3u;
				sample_point_clear(P);
				cube_point_taps(P, img, 1u, filter, at.face, x, y);
				printf("T %u %u %u %a %a %u %u %a %a %a %a", i, s, filter, x, y, P.nx, P.ny, P.wx[0], P.wx[1], P.wy[0], P.wy[1]);
				for (int t = 0; t < SAMPLE_TAPS; t++)
				{
					if (!((P.pending >> t) & 1u)) { printf(" -1 -1 -1"); continue; }
					const uint32_t bx = P.blk[t] % img.blocks_x, rest = P.blk[t] / img.blocks_x, by = rest % img.blocks_y, layer = rest / img.blocks_y;
					if (layer < 6u || layer >= 12u) return 3;
					printf(" %u %u %u", layer - 6u, bx * 5u + (P.txy[t] & 0xFFu), by * 4u + (P.txy[t] >> 8));
				}
				printf("\n");
			}
	}
	return 0;
}

static int tiles_mode(char** a)
{
	const int bx = atoi(a[0]), by = atoi(a[1]), profile = atoi(a[2]);
	const uint32_t kind = (uint32_t)atoi(a[3]), seed = (uint32_t)atoi(a[4]), s0 = (uint32_t)atoi(a[5]), levels = (uint32_t)atoi(a[6]), cube = (uint32_t)atoi(a[7]);
	const uint32_t filter = (uint32_t)atoi(a[8]), mip = (uint32_t)atoi(a[9]), type = (uint32_t)atoi(a[10]), layout = (uint32_t)atoi(a[11]), channels = (uint32_t)atoi(a[12]);
	const uint32_t ox = (uint32_t)atoi(a[13]), oy = (uint32_t)atoi(a[14]);
	const float bias = (float)atof(a[17]);
	const uint32_t pads = (uint32_t)atoi(a[18]);
	const std::string prefix = a[19];
	if (filter > 1 || mip > 1 || type > 2 || layout > 1 || channels < 1 || channels > 4 || kind > 3 || levels < 1 || levels > 32 || cube > 1 || s0 < 1 || s0 > 4096 || ox < 1 ||
	    oy < 1 || ox > 4096 || oy > 4096)
		return 2;
	g_x ^= (uint64_t)seed * 0x100000001B3ull;
	std::vector<float> dirs((size_t)ox * oy * 3u), lod((size_t)ox * oy);
	if (!read_floats(a[15], dirs)) return 2;
	const bool has_lod = strcmp(a[16], "-") != 0;
	if (has_lod && !read_floats(a[16], lod)) return 2;

	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	memset(static_cast<void*>(tile.data()), 0xCD, sizeof(SampleTile));
	// (the chain is entries 1 .. L of the call: entry 0 is another image, which no grid may touch)
	std::vector<DecodeImage> images(1 + levels);
	std::vector<std::vector<uint8_t>> blocks(levels);
	std::vector<const uint8_t*> streams(1 + levels, nullptr);
	memset(static_cast<void*>(&images[0]), 0, sizeof(DecodeImage));
	for (uint32_t l = 0; l < levels; l++)
	{
		const uint32_t s = s0 >> l ? s0 >> l : 1u, t = kind == 3 ? l % 3u : kind;
		DecodeImage img = make_image(bx, by, s, s, 12, profile, t, tabs.data());
		random_blocks(blocks[l], (size_t)img.blocks_x * img.blocks_y * img.blocks_z);
		std::vector<uint8_t> whole;
		decode_whole(img, blocks[l], whole, batch[0]);
		if (!write_bytes(prefix + ".level" + std::to_string(l), whole)) return 2;
		printf("level %u %u %u\n", l, s, t);
		images[1 + l] = img;
		streams[1 + l] = blocks[l].data();
	}

	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = type; format.layout = layout; format.channels = channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 0.00390625f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }
	const size_t eb = type == 0 ? 4 : 2, guard = 64;
	const bool planar = layout == 0;
	const size_t row = (size_t)ox * (planar ? 1 : channels) + ((pads & 1u) ? 3 : 0);
	const size_t plane = planar ? row * oy + ((pads & 1u) ? 5 : 0) : 0;
	const size_t elements = planar ? plane * channels : row * oy;
	std::vector<uint8_t> out(guard + elements * eb + guard, 0xA5);
	const size_t drow = 3u * (size_t)ox + ((pads & 2u) ? 5 : 0), lrow = (size_t)ox + ((pads & 4u) ? 7 : 0);
	std::vector<float> dheld(drow * oy, __builtin_nanf("")), lheld(lrow * oy, __builtin_nanf(""));
	for (uint32_t j = 0; j < oy; j++)
	{
		memcpy(dheld.data() + j * drow, dirs.data() + (size_t)j * 3u * ox, 3u * (size_t)ox * sizeof(float));
		memcpy(lheld.data() + j * lrow, lod.data() + (size_t)j * ox, (size_t)ox * sizeof(float));
	}
	DecodeLodLaunch g;
	memset(&g, 0, sizeof(g));
	g.first_entry = 1; g.level_count = levels; g.z = cube; g.out_x = ox; g.out_y = oy;
	g.d_coords = dheld.data(); g.coord_row_pitch = drow;
	g.d_lod = has_lod ? lheld.data() : nullptr; g.lod_row_pitch = lrow; g.lod_bias = bias;
	g.d_out = out.data() + guard; g.row_pitch = row; g.plane_pitch = plane;
	const DecodeLodSampler smp = { filter, 0, 0, mip };
	std::vector<uint8_t> table(decode_cube_bytes(&g, 1));
	const uint32_t tiles = decode_cube_build(table.data(), images.data(), streams.data(), format, smp, &g, 1);
	const std::vector<uint8_t> table_before = table;
	const std::vector<float> dirs_before = dheld, lod_before = lheld;
	const std::vector<std::vector<uint8_t>> blocks_before = blocks;
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(1);
	if (head->count != 1u || head->total != tiles || first[0] != 0u) return 3;
	printf("out %zu %zu %zu %zu\n", guard, row, plane, elements);
	for (uint32_t t = 0; t < tiles; t++)
	{
		const DecodeCubeRecord rec = image_set_record<DecodeCubeRecord>(reinterpret_cast<const uint32_t*>(records));
		const LevelsOfGrid level = { table.data() + rec.levels };
		const LodTileCount n = with_build(type, layout, [&](auto ty, auto la) { return decode_cube_tile<decltype(ty)::value, decltype(la)::value>(rec, level, t, batch[0], tile[0]); });
		printf("tile %u %u %u %u %u %u\n", t, n.passes, n.batches, n.blocks, n.level_mask, n.most);
	}
	if (table != table_before || blocks != blocks_before || memcmp(dheld.data(), dirs_before.data(), dheld.size() * sizeof(float)) != 0 ||
	    memcmp(lheld.data(), lod_before.data(), lheld.size() * sizeof(float)) != 0)
	{
		fprintf(stderr, "an input changed\n");
		return 1;
	}
	return write_bytes(prefix + ".out", out) ? 0 : 2;
}

static int blocks_mode(char** a)
{
	const uint32_t filter = (uint32_t)atoi(a[0]), mip = (uint32_t)atoi(a[1]), bx = (uint32_t)atoi(a[2]), by = (uint32_t)atoi(a[3]), s0 = (uint32_t)atoi(a[4]);
	const uint32_t levels = (uint32_t)atoi(a[5]), ox = (uint32_t)atoi(a[6]), oy = (uint32_t)atoi(a[7]);
	if (filter > 1 || mip > 1 || bx < 4 || bx > 12 || by < 4 || by > 12 || s0 < 1 || s0 > 65536 || levels < 1 || levels > 32 || ox < 1 || ox > 65535 || oy < 1 || oy > 65535) return 2;
	std::vector<float> dirs((size_t)ox * oy * 3u), lod((size_t)ox * oy);
	if (!read_floats(a[8], dirs)) return 2;
	const bool has_lod = strcmp(a[9], "-") != 0;
	if (has_lod && !read_floats(a[9], lod)) return 2;
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], (int)bx, (int)by, 1);
	std::vector<DecodeImage> images;
	std::vector<std::vector<uint8_t>> blocks;
	for (uint32_t l = 0; l < levels; l++)
	{
		images.push_back(make_image((int)bx, (int)by, s0 >> l ? s0 >> l : 1u, s0 >> l ? s0 >> l : 1u, 6, 0, 0, tabs.data()));
		const size_t nblocks = (size_t)images[l].blocks_x * images[l].blocks_y * 6u;
		blocks.emplace_back(nblocks * 16, (uint8_t)0xFF);
		for (size_t b = 0; b < nblocks; b++) { blocks[l][b * 16] = 0xFC; blocks[l][b * 16 + 1] = 0xFD; }
	}
	std::vector<const uint8_t*> streams;
	for (uint32_t l = 0; l < levels; l++) streams.push_back(blocks[l].data());
	std::vector<uint16_t> out((size_t)ox * oy * 3u);
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 1; format.layout = 0; format.channels = 3;
	for (int c = 0; c < 3; c++) format.scale[c] = 1.0f;
	DecodeLodLaunch g;
	memset(&g, 0, sizeof(g));
	g.first_entry = 0; g.level_count = levels; g.z = 0; g.out_x = ox; g.out_y = oy;
	g.d_coords = dirs.data(); g.coord_row_pitch = 3u * (size_t)ox;
	g.d_lod = has_lod ? lod.data() : nullptr; g.lod_row_pitch = ox;
	g.d_out = out.data(); g.row_pitch = ox; g.plane_pitch = (size_t)ox * oy;
	const DecodeLodSampler smp = { filter, 0, 0, mip };
	std::vector<uint8_t> table(decode_cube_bytes(&g, 1));
	const uint32_t tiles = decode_cube_build(table.data(), images.data(), streams.data(), format, smp, &g, 1);
	DecodeCubeRecord rec;
	memcpy(static_cast<void*>(&rec), table.data() + image_set_records_offset(1), sizeof(rec));
	const LevelsOfGrid level = { table.data() + rec.levels };
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	unsigned long long passes = 0, batches = 0, decoded = 0;
	for (uint32_t t = 0; t < tiles; t++)
	{
		const LodTileCount n = decode_cube_tile<1, 0>(rec, level, t, batch[0], tile[0]);
		passes += n.passes; batches += n.batches; decoded += n.blocks;
	}
	printf("tiles %u passes %llu batches %llu decoded %llu points %llu\n", tiles, passes, batches, decoded, (unsigned long long)ox * oy);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 4 && strcmp(argv[1], "points") == 0) return points_mode(argv + 2);
	if (argc == 22 && strcmp(argv[1], "tiles") == 0) return tiles_mode(argv + 2);
	if (argc == 12 && strcmp(argv[1], "blocks") == 0) return blocks_mode(argv + 2);
	fprintf(stderr, "usage: decode_cube_check points|tiles|blocks ... (see the head of the source)\n");
	return 2;
}
