// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the volume sampler of astcenc_amd_sample_volume_tensors_device (decode_volume.h: the host-built table, the
// tap stage -- volume_valid, volume_point_taps -- and decode_volume_tile on decode_lod.h's level walk) on the host, as sequential
// code under the sanitizers.  The model is tests/sample_volume_model.py: this program computes and prints or writes what the
// header's routines give, tests/test_decode_volume_cpu.py compares.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_volume_check.cpp -o decode_volume_check
// `points <bx> <by> <bz> <W> <H> <D> <file> <n>`: for each of the n triples (binary32) of the file a line
//     V i valid valid_with_nan_lambda
//   and, when valid, for each filter f and each turn m of the address modes (x: m, y: m + 1, z: m + 2, each mod 4) a line
//     T i f m x y z nx ny nz wx0 wx1 wy0 wy1 wz0 wz1 then per tap slot: kx ky kz     (hex floats; -1 -1 -1: no such tap)
//   the taps read back from VolumePoint::blk and txyz of a W x H x D image of that footprint.
// `tiles <bx> <by> <bz> <profile> <kind> <seed> <W> <H> <D> <levels> <filter> <ax> <ay> <az> <mip> <type> <layout> <channels> <ox>
//        <oy> <coords> <lod> <bias> <pads> <prefix>`: a chain of `levels` levels of max(1, W >> l) x max(1, H >> l) x
//   max(1, D >> l) texels, every level a random stream of its own (kind 0 U8, 1 F16, 2 F32, 3 the three in turn) with
//   constant-colour and reserved-mode blocks; the grid's triples and levels of detail (lod "-": NULL) are the files' bytes; pads:
//   bit 0 a padded output, bit 1 padded rows of triples, bit 2 padded rows of lod (the padding holds NaNs).  Writes what the
//   decoder gives for every whole level to <prefix>.level<l> and the guard-filled output buffer after all tiles to <prefix>.out;
//   prints "level l W H D dtype", "out guard row plane elements" and per tile "tile t passes batches blocks mask most blended
//   single" (most: the most blocks one pass listed).
// `blocks <bx> <by> <bz> <filter> <mip> <W> <H> <D> <levels> <ox> <oy> <coords> <lod>`: the tiles of one grid over the first `levels`
//   levels of the chain of a W x H x D volume of constant-colour blocks, CLAMP on every axis; prints tiles, passes, batches,
//   blocks decoded (tools/time_decode_volume.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_volume.h"
#define DECODE_CHECK_ITEM "grid"
#include "decode_lod_check_common.h"
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static_assert(VOLUME_TILE_BLOCKS == 512, "the listed-block trap of sample_batches (eight slots) bounds a pass at 512 blocks");

static const uint32_t RGBA[4] = { 0, 1, 2, 3 };

static int points_mode(char** a)
{
	const int bx = atoi(a[0]), by = atoi(a[1]), bz = atoi(a[2]);
	const uint32_t W = (uint32_t)atoi(a[3]), H = (uint32_t)atoi(a[4]), D = (uint32_t)atoi(a[5]);
	const uint32_t n = (uint32_t)atoi(a[7]);
	if (bx < 3 || by < 3 || bz < 1 || W < 1 || H < 1 || D < 1) return 2;
	std::vector<float> p((size_t)n * 3u);
	if (!read_floats(a[6], p)) return 2;
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
	const DecodeImage img = make_image(bx, by, bz, W, H, D, 0, 0, RGBA, tabs.data());
	std::vector<DecodeLodLevel> lv(1);
	lv[0].img = img; lv[0].blocks = nullptr;
	const float nan = __builtin_nanf("");
	for (uint32_t i = 0; i < n; i++)
	{
		std::vector<float> one = { p[3u * i], p[3u * i + 1u], p[3u * i + 2u] };
		DecodeVolumeRecord rec;
		memset(static_cast<void*>(&rec), 0, sizeof(rec));
		rec.coords = one.data(); rec.coord_row = 3;
		const VolumeUVW at = VolumePoints::read(rec, 0, 0);
		const bool ok = VolumePoints::valid(at, 0.0f);
		printf("V %u %d %d\n", i, ok ? 1 : 0, VolumePoints::valid(at, nan) ? 1 : 0);
		if (ok != volume_valid(one[0], one[1], one[2], 0.0f)) return 3;
		if (!ok) continue;
		for (uint32_t filter = 0; filter < 2; filter++)
			for (uint32_t m = 0; m < 4; m++)
			{
				rec.filter = filter; rec.address_x = m; rec.address_y = (m + 1u) & 3u; rec.address_z = (m + 2u) & 3u;
				VolumePoint P;
				P.live = 3u;
				sample_point_clear(P);
				VolumePoints::taps(P, rec, lv[0], at);
				printf("T %u %u %u %a %a %a %u %u %u %a %a %a %a %a %a", i, filter, m, (double)at.u * (double)W, (double)at.v * (double)H, (double)at.w * (double)D, P.nx, P.ny, P.nz,
				       P.wx[0], P.wx[1], P.wy[0], P.wy[1], P.wz[0], P.wz[1]);
				for (int t = 0; t < VOLUME_TAPS; t++)
				{
					if (!((P.pending >> t) & 1u)) { printf(" -1 -1 -1"); continue; }
					const uint32_t cx = P.blk[t] % img.blocks_x, rest = P.blk[t] / img.blocks_x, cy = rest % img.blocks_y, cz = rest / img.blocks_y;
					const uint32_t tx = P.txyz[t] & 0xFFu, ty = (P.txyz[t] >> 8) & 0xFFu, tz = P.txyz[t] >> 16;
					if (cz >= img.blocks_z || tx >= (uint32_t)bx || ty >= (uint32_t)by || tz >= (uint32_t)bz) return 3;
					printf(" %u %u %u", cx * bx + tx, cy * by + ty, cz * bz + tz);
				}
				printf("\n");
			}
	}
	return 0;
}

static int tiles_mode(char** a)
{
	const int bx = atoi(a[0]), by = atoi(a[1]), bz = atoi(a[2]), profile = atoi(a[3]);
	const uint32_t kind = (uint32_t)atoi(a[4]), seed = (uint32_t)atoi(a[5]), W0 = (uint32_t)atoi(a[6]), H0 = (uint32_t)atoi(a[7]), D0 = (uint32_t)atoi(a[8]);
	const uint32_t levels = (uint32_t)atoi(a[9]), filter = (uint32_t)atoi(a[10]), ax = (uint32_t)atoi(a[11]), ay = (uint32_t)atoi(a[12]), az = (uint32_t)atoi(a[13]);
	const uint32_t mip = (uint32_t)atoi(a[14]), type = (uint32_t)atoi(a[15]), layout = (uint32_t)atoi(a[16]), channels = (uint32_t)atoi(a[17]);
	const uint32_t ox = (uint32_t)atoi(a[18]), oy = (uint32_t)atoi(a[19]);
	const float bias = (float)atof(a[22]);
	const uint32_t pads = (uint32_t)atoi(a[23]);
	const std::string prefix = a[24];
	if (filter > 1 || ax > 3 || ay > 3 || az > 3 || mip > 1 || type > 2 || layout > 1 || channels < 1 || channels > 4 || kind > 3 || levels < 1 || levels > 32 || bx < 3 || by < 3 ||
	    bz < 1 || W0 < 1 || H0 < 1 || D0 < 1 || W0 > 4096 || H0 > 4096 || D0 > 4096 || ox < 1 || oy < 1 || ox > 4096 || oy > 4096)
		return 2;
	g_x ^= (uint64_t)seed * 0x100000001B3ull;
	std::vector<float> coords((size_t)ox * oy * 3u), lod((size_t)ox * oy);
	if (!read_floats(a[20], coords)) return 2;
	const bool has_lod = strcmp(a[21], "-") != 0;
	if (has_lod && !read_floats(a[21], lod)) return 2;

	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
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
		const uint32_t W = W0 >> l ? W0 >> l : 1u, H = H0 >> l ? H0 >> l : 1u, D = D0 >> l ? D0 >> l : 1u, t = kind == 3 ? l % 3u : kind;
		DecodeImage img = make_image(bx, by, bz, W, H, D, profile, t, RGBA, tabs.data());
		random_blocks(blocks[l], (size_t)img.blocks_x * img.blocks_y * img.blocks_z);
		std::vector<uint8_t> whole;
		decode_whole(img, blocks[l], whole, batch[0]);
		if (!write_bytes(prefix + ".level" + std::to_string(l), whole)) return 2;
		printf("level %u %u %u %u %u\n", l, W, H, D, t);
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
	const size_t crow = 3u * (size_t)ox + ((pads & 2u) ? 5 : 0), lrow = (size_t)ox + ((pads & 4u) ? 7 : 0);
	std::vector<float> cheld(crow * oy, __builtin_nanf("")), lheld(lrow * oy, __builtin_nanf(""));
	for (uint32_t j = 0; j < oy; j++)
	{
		memcpy(cheld.data() + j * crow, coords.data() + (size_t)j * 3u * ox, 3u * (size_t)ox * sizeof(float));
		memcpy(lheld.data() + j * lrow, lod.data() + (size_t)j * ox, (size_t)ox * sizeof(float));
	}
	DecodeLodLaunch g;
	memset(&g, 0, sizeof(g));
	g.first_entry = 1; g.level_count = levels; g.out_x = ox; g.out_y = oy;
	g.d_coords = cheld.data(); g.coord_row_pitch = crow;
	g.d_lod = has_lod ? lheld.data() : nullptr; g.lod_row_pitch = lrow; g.lod_bias = bias;
	g.d_out = out.data() + guard; g.row_pitch = row; g.plane_pitch = plane;
	const DecodeLodSampler smp = { filter, ax, ay, mip, az };
	std::vector<uint8_t> table(decode_volume_bytes(&g, 1));
	const uint32_t tiles = decode_volume_build(table.data(), images.data(), streams.data(), format, smp, &g, 1);
	const std::vector<uint8_t> table_before = table;
	const std::vector<float> coords_before = cheld, lod_before = lheld;
	const std::vector<std::vector<uint8_t>> blocks_before = blocks;
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(1);
	if (head->count != 1u || head->total != tiles || first[0] != 0u) return 3;
	printf("out %zu %zu %zu %zu\n", guard, row, plane, elements);
	for (uint32_t t = 0; t < tiles; t++)
	{
		const DecodeVolumeRecord rec = image_set_record<DecodeVolumeRecord>(reinterpret_cast<const uint32_t*>(records));
		const LevelsOfGrid level = { table.data() + rec.levels };
		const LodTileCount n = with_build(type, layout, [&](auto ty, auto la) { return decode_volume_tile<decltype(ty)::value, decltype(la)::value>(rec, level, t, batch[0], tile[0]); });
		printf("tile %u %u %u %u %u %u %u %u\n", t, n.passes, n.batches, n.blocks, n.level_mask, n.most, n.blended, n.single);
	}
	if (table != table_before || blocks != blocks_before || memcmp(cheld.data(), coords_before.data(), cheld.size() * sizeof(float)) != 0 ||
	    memcmp(lheld.data(), lod_before.data(), lheld.size() * sizeof(float)) != 0)
	{
		fprintf(stderr, "an input changed\n");
		return 1;
	}
	return write_bytes(prefix + ".out", out) ? 0 : 2;
}

static int blocks_mode(char** a)
{
	const int bx = atoi(a[0]), by = atoi(a[1]), bz = atoi(a[2]);
	const uint32_t filter = (uint32_t)atoi(a[3]), mip = (uint32_t)atoi(a[4]), W0 = (uint32_t)atoi(a[5]), H0 = (uint32_t)atoi(a[6]), D0 = (uint32_t)atoi(a[7]);
	const uint32_t levels = (uint32_t)atoi(a[8]), ox = (uint32_t)atoi(a[9]), oy = (uint32_t)atoi(a[10]);
	if (filter > 1 || mip > 1 || bx < 3 || by < 3 || bz < 1 || W0 < 1 || H0 < 1 || D0 < 1 || W0 > 65536 || H0 > 65536 || D0 > 65536 || levels < 1 || levels > 32 || ox < 1 ||
	    ox > 65535 || oy < 1 || oy > 65535)
		return 2;
	std::vector<float> coords((size_t)ox * oy * 3u), lod((size_t)ox * oy);
	if (!read_floats(a[11], coords)) return 2;
	const bool has_lod = strcmp(a[12], "-") != 0;
	if (has_lod && !read_floats(a[12], lod)) return 2;
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
	std::vector<DecodeImage> images;
	std::vector<std::vector<uint8_t>> blocks;
	for (uint32_t l = 0; l < levels; l++)
	{
		images.push_back(make_image(bx, by, bz, W0 >> l ? W0 >> l : 1u, H0 >> l ? H0 >> l : 1u, D0 >> l ? D0 >> l : 1u, 0, 0, RGBA, tabs.data()));
		const size_t nblocks = (size_t)images[l].blocks_x * images[l].blocks_y * images[l].blocks_z;
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
	g.first_entry = 0; g.level_count = levels; g.out_x = ox; g.out_y = oy;
	g.d_coords = coords.data(); g.coord_row_pitch = 3u * (size_t)ox;
	g.d_lod = has_lod ? lod.data() : nullptr; g.lod_row_pitch = ox;
	g.d_out = out.data(); g.row_pitch = ox; g.plane_pitch = (size_t)ox * oy;
	const DecodeLodSampler smp = { filter, 0, 0, mip };
	std::vector<uint8_t> table(decode_volume_bytes(&g, 1));
	const uint32_t tiles = decode_volume_build(table.data(), images.data(), streams.data(), format, smp, &g, 1);
	DecodeVolumeRecord rec;
	memcpy(static_cast<void*>(&rec), table.data() + image_set_records_offset(1), sizeof(rec));
	const LevelsOfGrid level = { table.data() + rec.levels };
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	unsigned long long passes = 0, batches = 0, decoded = 0;
	for (uint32_t t = 0; t < tiles; t++)
	{
		const LodTileCount n = decode_volume_tile<1, 0>(rec, level, t, batch[0], tile[0]);
		passes += n.passes; batches += n.batches; decoded += n.blocks;
	}
	printf("tiles %u passes %llu batches %llu decoded %llu points %llu\n", tiles, passes, batches, decoded, (unsigned long long)ox * oy);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 10 && strcmp(argv[1], "points") == 0) return points_mode(argv + 2);
	if (argc == 27 && strcmp(argv[1], "tiles") == 0) return tiles_mode(argv + 2);
	if (argc == 15 && strcmp(argv[1], "blocks") == 0) return blocks_mode(argv + 2);
	fprintf(stderr, "usage: decode_volume_check points|tiles|blocks ... (see the head of the source)\n");
	return 2;
}
