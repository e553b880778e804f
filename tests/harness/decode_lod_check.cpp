// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the level-of-detail sampler of astcenc_amd_sample_lod_tensors_device (decode_lod.h: the host-built table and
// decode_lod_tile -- the levels of every point, a pass per distinct level through decode_sample.h's taps, batches and sums, the
// blend) against decode_row_batch of every whole level followed by the definition written out in plain C++ below from the header's
// comment, on the host, as sequential code under the sanitizers.  A chain is the full mip chain of a 17 x 17-block image (6x6:
// 102, 51, 25, 12, 6, 3, 1), two slices; every level is a random stream of its own -- random 16-byte patterns mixed with
// constant-colour blocks (UNORM16 and FP16) and reserved-mode blocks -- so the levels look nothing alike.  Footprints 4x4, 6x6,
// 10x8 and 12x12; the four profiles; chains of U8, F16 and F32 levels and one mixing them.  Each chain is sampled with both
// filters x both mip filters and six formats -- every tensor type with both layouts -- the address modes turning from table to
// table so that every pair is met, and per table several grids: random (u, v) in [-0.25, 1.25] with random lambda in
// [-1, L + 0.5]; an image-shaped grid with a smoothly varying lambda; integer lambda; 64 equal points; the special values of u, v
// and lambda, each against each; lod NULL with a bias; grids of 1, 2, 3 and 5 rows whose width is no multiple of the tile's; tight
// and padded pitches alternate, for outputs, coordinates and lod (the padding of both inputs holds NaNs).
// Then, per footprint: 64 points at level-0 block corners with lambda = 0.5 (256 distinct blocks in the level-0 pass), and a chain
// whose odd levels decode to NaN everywhere sampled at even integer lambda (a level of weight zero is not read).
// Required: every element of every grid equal to the model's bits, every other byte of every buffer intact, the inputs
// unchanged, as many tiles as the grids' sizes need, and per tile as many passes as its points have distinct levels and as many
// blocks decoded as their taps of non-zero weight reach in levels of non-zero weight; some tile with at least four distinct
// levels; points with g = 0 and with g != 0.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_lod_check.cpp -o decode_lod_check
// `decode_lod_check tables` prints the table of a hand-computed case and the levels of a few lambda instead
// (tests/test_decode_lod_cpu.py); `blocks` runs the tiles of one grid read from files and counts passes, batches and blocks
// decoded (tools/time_decode_lod.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_lod.h"
#define DECODE_CHECK_ITEM "grid"
#include "decode_lod_check_common.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

static unsigned long long g_decoded = 0, g_batches = 0, g_passes = 0, g_tiles = 0;
static unsigned g_pairs_seen = 0;              // bit (address_x * 4 + address_y)
static uint32_t g_most_levels = 0;             // the most distinct levels a tile had
static bool g_blended = false, g_single = false;

/* A chain: per level the image, its stream and what the decoder writes for the whole of it. */
struct Chain {
	std::vector<DecodeImage> images;
	std::vector<std::vector<uint8_t>> blocks, whole;
	uint32_t levels() const { return (uint32_t)images.size(); }
};

/* The model (include/astcenc_amd.h), one operation at a time: a texel's component widened (source_value, decode_check_common.h) ... */
/* ... the taps of a binary64 level coordinate along an axis: indices before addressing and weights in tap order, zero weights
 * left out ... */
struct Tap { int64_t i; double w; };
static void model_taps(uint32_t filter, double u, std::vector<Tap>& taps)
{
	taps.clear();
	if (filter == 0)
	{
		taps.push_back({ (int64_t)std::floor(u), 1.0 });
		return;
	}
	volatile double t = u - 0.5;
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

/* ... the levels of lambda' and the weight of the second (l1 < 0: one level) ... */
struct ModelLevels { int l0, l1; double g; };
static ModelLevels model_levels(uint32_t mip_filter, uint32_t level_count, float lambda)
{
	const float top = (float)((int)level_count - 1);
	const float lc = lambda < 0.0f ? 0.0f : lambda > top ? top : lambda;
	ModelLevels r = { 0, -1, 0.0 };
	if (mip_filter == 0)
	{
		volatile double sum = (double)lc + 0.5;
		r.l0 = (int)std::ceil(sum) - 1;
		return r;
	}
	r.l0 = (int)std::floor((double)lc);
	r.g = (double)lc - (double)r.l0;
	if (r.g != 0.0) r.l1 = r.l0 + 1;
	return r;
}

/* ... the sample of a level at the point, as the sample call defines it; the blocks its taps read go into `reached` ... */
static float model_level_sample(const Chain& ch, int level, const DecodeLodSampler& smp, uint32_t z, float u, float v, uint32_t c, std::set<uint64_t>* reached)
{
	const DecodeImage& img = ch.images[(size_t)level];
	const size_t tb = img.data_type == 0 ? 4 : img.data_type == 1 ? 8 : 16;
	volatile double x = (double)u * (double)img.dim_x, y = (double)v * (double)img.dim_y;
	std::vector<Tap> tx, ty;
	model_taps(smp.filter, x, tx);
	model_taps(smp.filter, y, ty);
	volatile double acc = 0.0;
	for (size_t b = 0; b < ty.size(); b++)
	{
		volatile double row = 0.0;
		int64_t ky;
		const bool in_y = model_address(smp.address_y, ty[b].i, (int64_t)img.dim_y, ky);
		for (size_t a = 0; a < tx.size(); a++)
		{
			int64_t kx;
			const bool in_x = model_address(smp.address_x, tx[a].i, (int64_t)img.dim_x, kx);
			double val = 0.0;
			if (in_x && in_y)
			{
				val = source_value(ch.whole[(size_t)level].data() + ((((size_t)z * img.dim_y + (size_t)ky) * img.dim_x) + (size_t)kx) * tb, img.data_type, c);
				if (reached)
					reached->insert(((uint64_t)level << 40) | (uint64_t)(((size_t)z * img.blocks_y + (size_t)ky / img.block_y) * img.blocks_x + (size_t)kx / img.block_x));
			}
			volatile double p = tx[a].w * val;
			row = a == 0 ? p : row + p;
		}
		volatile double p = ty[b].w * row;
		acc = b == 0 ? p : acc + p;
	}
	return (float)acc;
}

/* ... the point: validity, the levels, the blend ... */
static float model_point(const Chain& ch, const DecodeLodSampler& smp, uint32_t z, float u, float v, float lod, float bias, uint32_t c, std::set<uint64_t>* reached,
                         uint32_t* level_mask)
{
	volatile float lambda = lod + bias;
	const bool valid = std::isfinite(u) && std::isfinite(v) && std::fabs((double)u) <= 16384.0 && std::fabs((double)v) <= 16384.0 && !std::isnan(lambda);
	if (!valid) return 0.0f;
	const ModelLevels lv = model_levels(smp.mip_filter, ch.levels(), lambda);
	if (level_mask) *level_mask |= 1u << lv.l0 | (lv.l1 >= 0 ? 1u << lv.l1 : 0u);
	const float s0 = model_level_sample(ch, lv.l0, smp, z, u, v, c, reached);
	if (lv.l1 < 0) return s0;
	const float s1 = model_level_sample(ch, lv.l1, smp, z, u, v, c, reached);
	volatile double w0 = 1.0 - lv.g;
	volatile double p0 = w0 * (double)s0, p1 = lv.g * (double)s1;
	volatile double sum = p0 + p1;
	return (float)sum;
}

struct Grid { uint32_t z, ox, oy; std::vector<float> uv; std::vector<float> lod; bool has_lod; float bias; };       // uv: ox * oy pairs, row by row

static LodTileCount run_tile(const DecodeLodRecord& rec, const uint8_t* table, uint32_t local, DecodeBatch& batch, SampleTile& tile)
{
	const LevelsOfGrid levels = { table + rec.levels };
	return with_build(rec.fmt.type, rec.fmt.layout, [&](auto t, auto l) { return decode_lod_tile<decltype(t)::value, decltype(l)::value>(rec, levels, local, batch, tile); });
}

/* One table of all `wanted` grids over one chain (entries first_entry .. of a call whose other entries are left null). */
static void check_table(const char* chain_tag, const Chain& ch, const std::vector<Grid>& wanted, DecodeBatch& batch, SampleTile& tile, const Format& f,
                        const DecodeLodSampler& smp, uint32_t turn, std::vector<LodTileCount>* per_tile = nullptr)
{
	char tag[256];
	snprintf(tag, sizeof(tag), "%s -> filter %u address %u %u mip %u type %u layout %u channels %u", chain_tag, smp.filter, smp.address_x, smp.address_y, smp.mip_filter, f.type,
	         f.layout, f.channels);
	const size_t eb = f.type == 0 ? 4 : 2;
	const bool planar = f.layout == 0;
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = f.type; format.layout = f.layout; format.channels = f.channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 1.0f / 255.0f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }
	g_pairs_seen |= 1u << (smp.address_x * 4u + smp.address_y);

	// (the chain is entries 1 .. L of the call: entry 0 is another image, which no grid may touch)
	const uint32_t first_entry = 1, L = ch.levels();
	std::vector<DecodeImage> images(1 + L);
	std::vector<const uint8_t*> streams(1 + L, nullptr);
	memset(static_cast<void*>(&images[0]), 0, sizeof(DecodeImage));
	for (uint32_t l = 0; l < L; l++) { images[1 + l] = ch.images[l]; streams[1 + l] = ch.blocks[l].data(); }

	const size_t guard = 64;
	const uint32_t count = (uint32_t)wanted.size();
	std::vector<DecodeLodLaunch> grids(count);
	std::vector<std::vector<uint8_t>> outs(count);
	std::vector<std::vector<float>> coords(count), lods(count);
	unsigned long long want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Grid& w = wanted[i];
		const bool padded = ((i + turn) & 1u) != 0u, coords_padded = ((i + turn) & 2u) != 0u, lod_padded = ((i + turn) % 3u) == 1u;
		const size_t row = (size_t)w.ox * (planar ? 1 : f.channels) + (padded ? 3 : 0);
		const size_t plane = planar ? row * w.oy + (padded ? 5 : 0) : 0;
		const size_t elements = planar ? plane * f.channels : row * w.oy;
		outs[i].assign(guard + elements * eb + guard, 0xA5);
		const size_t crow = 2u * (size_t)w.ox + (coords_padded ? 6 : 0), lrow = (size_t)w.ox + (lod_padded ? 5 : 0);
		// (the padding of a row of coordinates or of levels of detail holds NaNs: read into a point they would show)
		coords[i].assign(crow * w.oy, __builtin_nanf(""));
		lods[i].assign(lrow * w.oy, __builtin_nanf(""));
		for (uint32_t j = 0; j < w.oy; j++)
		{
			memcpy(coords[i].data() + j * crow, w.uv.data() + (size_t)j * 2u * w.ox, 2u * (size_t)w.ox * sizeof(float));
			if (w.has_lod) memcpy(lods[i].data() + j * lrow, w.lod.data() + (size_t)j * w.ox, (size_t)w.ox * sizeof(float));
		}
		DecodeLodLaunch& g = grids[i];
		memset(&g, 0, sizeof(g));
		g.first_entry = first_entry; g.level_count = L;
		g.z = w.z; g.out_x = w.ox; g.out_y = w.oy;
		g.d_coords = coords[i].data(); g.coord_row_pitch = crow;
		g.d_lod = w.has_lod ? lods[i].data() : nullptr; g.lod_row_pitch = lrow;
		g.lod_bias = w.bias;
		g.d_out = outs[i].data() + guard;
		g.row_pitch = row; g.plane_pitch = plane;
		// (the tiles, spelled out: 64 x 1, 32 x 2, 16 x 4, 8 x 8 from five rows on)
		const uint32_t th = w.oy >= 5 ? 8u : w.oy >= 3 ? 4u : w.oy, tw = 64u / th;
		want_total += (unsigned long long)((w.ox + tw - 1u) / tw) * ((w.oy + th - 1u) / th);
	}
	std::vector<uint8_t> table(decode_lod_bytes(grids.data(), count));
	const uint32_t total = decode_lod_build(table.data(), images.data(), streams.data(), format, smp, grids.data(), count);
	const std::vector<uint8_t> table_before = table;
	const std::vector<std::vector<uint8_t>> blocks_before = ch.blocks;
	const std::vector<std::vector<float>> coords_before = coords, lods_before = lods;

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	// (the LDS of a fresh workgroup holds anything)
	memset(static_cast<void*>(&tile), 0xCD, sizeof(SampleTile));
	std::vector<std::vector<LodTileCount>> did(count);
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeLodRecord rec = image_set_record<DecodeLodRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeLodRecord)));
		const LodTileCount n = run_tile(rec, table.data(), r - first[g], batch, tile);
		if (n.passes > L || n.blocks > 256u * n.passes || n.batches * (uint32_t)DECODE_BATCH < n.blocks) fail("a tile's passes, batches and blocks", tag, g, (long)n.blocks);
		if (per_tile) per_tile->push_back(n);
		did[g].push_back(n);
		g_decoded += n.blocks; g_batches += n.batches; g_passes += n.passes; g_tiles++;
		if (n.blended) g_blended = true;
		if (n.single) g_single = true;
		const uint32_t distinct = (uint32_t)__builtin_popcount(n.level_mask);
		if (distinct > g_most_levels) g_most_levels = distinct;
	}
	if (ch.blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);
	for (uint32_t i = 0; i < count; i++)
		if (memcmp(coords[i].data(), coords_before[i].data(), coords[i].size() * sizeof(float)) != 0 || memcmp(lods[i].data(), lods_before[i].data(), lods[i].size() * sizeof(float)) != 0)
			fail("the coordinates or the levels of detail changed", tag, i, 0);

	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeLodLaunch& g = grids[i];
		const std::vector<uint8_t>& o = outs[i];
		std::vector<uint8_t> want(o.size(), 0xA5);
		const uint32_t th = g.out_y >= 5 ? 8u : g.out_y >= 3 ? 4u : g.out_y, tw = 64u / th, tiles_x = (g.out_x + tw - 1u) / tw;
		std::vector<std::set<uint64_t>> reached(did[i].size());
		std::vector<uint32_t> masks(did[i].size(), 0u);
		for (uint32_t j = 0; j < g.out_y; j++)
			for (uint32_t x = 0; x < g.out_x; x++)
			{
				const float u = g.d_coords[j * g.coord_row_pitch + 2u * x], v = g.d_coords[j * g.coord_row_pitch + 2u * x + 1u];
				const float lod = g.d_lod ? g.d_lod[j * g.lod_row_pitch + x] : 0.0f;
				const size_t t = (size_t)(j / th) * tiles_x + x / tw;
				// (all four components decide what a tile reads, whatever the format keeps)
				for (uint32_t c = 0; c < 4; c++)
				{
					const float s = model_point(ch, smp, g.z, u, v, lod, g.lod_bias, c, &reached[t], &masks[t]);
					if (c >= f.channels) continue;
					const uint32_t bits = model_bits(s, format.scale[c], format.bias[c], f.type);
					const size_t at = planar ? c * g.plane_pitch + j * g.row_pitch + x : j * g.row_pitch + (size_t)x * f.channels + c;
					memcpy(want.data() + guard + at * eb, &bits, eb);
				}
			}
		for (size_t t = 0; t < did[i].size(); t++)
		{
			if (did[i][t].level_mask != masks[t] || did[i][t].passes != (uint32_t)__builtin_popcount(masks[t])) fail("a tile's level passes are not its points' distinct levels", tag, i, (long)t);
			if (did[i][t].blocks != reached[t].size()) fail("a tile decoded other blocks than its taps of non-zero weight reach", tag, i, (long)t);
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

/* The full chain of a dim_x x dim_y x dim_z image; dtype 3: levels of U8, F16, F32 in turn; nan_odd: odd levels are F16 and hold
 * reserved-mode blocks only. */
static Chain make_chain(int bx, int by, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, int profile, uint32_t dtype, const DecodeTables* tabs, DecodeBatch& batch,
                        bool nan_odd = false)
{
	Chain ch;
	for (uint32_t l = 0; ; l++)
	{
		const uint32_t w = dim_x >> l ? dim_x >> l : 1u, h = dim_y >> l ? dim_y >> l : 1u;
		const uint32_t t = nan_odd ? ((l & 1u) ? 1u : dtype) : dtype == 3 ? l % 3u : dtype;
		DecodeImage img = make_image(bx, by, w, h, dim_z, profile, t, tabs);
		ch.blocks.emplace_back();
		ch.whole.emplace_back();
		random_blocks(ch.blocks.back(), (size_t)img.blocks_x * img.blocks_y * img.blocks_z, nan_odd && (l & 1u));
		decode_whole(img, ch.blocks.back(), ch.whole.back(), batch);
		ch.images.push_back(img);
		if (w == 1 && h == 1) break;
	}
	return ch;
}

static Grid random_grid(uint32_t z, uint32_t ox, uint32_t oy, float lo, float hi, float l0, float l1, bool has_lod = true, float bias = 0.0f)
{
	Grid g = { z, ox, oy, {}, {}, has_lod, bias };
	for (uint32_t k = 0; k < ox * oy; k++)
	{
		g.uv.push_back(lo + (hi - lo) * rnd_unit());
		g.uv.push_back(lo + (hi - lo) * rnd_unit());
		g.lod.push_back(l0 + (l1 - l0) * rnd_unit());
	}
	return g;
}

static void check(int bx, int by, int profile, uint32_t dtype, uint32_t config)
{
	const uint32_t ubx = (uint32_t)bx, uby = (uint32_t)by;
	const uint32_t dim_x = 17u * ubx, dim_y = 17u * uby, dim_z = 2u;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%d %ux%ux%u profile %d type %u", bx, by, dim_x, dim_y, dim_z, profile, dtype);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	const Chain ch = make_chain(bx, by, dim_x, dim_y, dim_z, profile, dtype, tabs.data(), batch[0]);
	const float top = (float)(ch.levels() - 1u), inf = __builtin_inff(), nan = __builtin_nanf("");

	std::vector<Grid> grids;
	grids.push_back(random_grid(0, 37, 11, -0.25f, 1.25f, -1.0f, top + 1.5f));                          // anywhere, any level
	{
		// an image-shaped grid: the texture seen at an angle, lambda rising smoothly from the near edge to the far one
		Grid g = { 1, 24, 16, {}, {}, true, 0.0f };
		for (uint32_t j = 0; j < g.oy; j++)
			for (uint32_t i = 0; i < g.ox; i++)
			{
				g.uv.push_back(((float)i + 0.5f) / 24.0f); g.uv.push_back(((float)j + 0.5f) / 16.0f);
				g.lod.push_back(top * ((float)j * 24.0f + (float)i) / (16.0f * 24.0f));
			}
		grids.push_back(g);
	}
	{
		// integer lambda: the level itself under either mip filter
		Grid g = random_grid(0, 21, 4, 0.0f, 1.0f, 0.0f, 0.0f);
		for (size_t k = 0; k < g.lod.size(); k++) g.lod[k] = (float)(rnd() % ch.levels());
		grids.push_back(g);
	}
	{
		// 64 equal points: one block a level in one tile
		Grid g = { 0, 64, 1, {}, {}, true, 0.0f };
		for (uint32_t i = 0; i < 64; i++) { g.uv.push_back(0.3f); g.uv.push_back(0.7f); g.lod.push_back(1.25f); }
		grids.push_back(g);
	}
	grids.push_back(random_grid(1, 35, 2, 0.0f, 1.0f, 0.0f, top, false, 1.5f));                        // 32 x 2 tiles; lod NULL: the bias alone
	grids.push_back(random_grid(0, 19, 3, 0.0f, 1.0f, -0.5f, 2.0f, true, 0.75f));                      // 16 x 4; a bias moves points across levels
	grids.push_back(random_grid(1, 11, 5, -0.1f, 1.1f, 0.0f, top));                                    // 8 x 8
	grids.push_back(random_grid(0, 70, 1, -3.0f, 3.0f, 2.0f, top + 1.0f));                             // 64 x 1; REPEAT and MIRROR over several periods
	{
		// the special values of u, v and lambda: every u against every v, lambda turning through its list
		const float big = 16384.0f, next = __builtin_nextafterf(big, inf);
		const float s[] = { 0.5f, 0.0f, -0.0f, 1.0f, 0.99999994f, 1e-30f, -0.25f, nan, inf, -inf, big, next, -big, -next, 1.0f / 34.0f, 1.5f };
		const float lam[] = { -1.0f, 0.0f, -0.0f, 0.5f, 1.0f, 1.5f, top, top + 3.0f, inf, -inf, nan, 0.49999997f, 0.50000006f, 1e-30f, top - 0.25f };
		const uint32_t n = sizeof(s) / sizeof(s[0]), m = sizeof(lam) / sizeof(lam[0]);
		Grid g = { 0, n, n, {}, {}, true, 0.0f };
		for (uint32_t j = 0; j < n; j++)
			for (uint32_t i = 0; i < n; i++) { g.uv.push_back(s[i]); g.uv.push_back(s[j]); g.lod.push_back(lam[(j * n + i + config) % m]); }
		grids.push_back(g);
	}

	// (every build of the store: three types x two layouts; channels 1, 3 and 4)
	const Format formats[6] = { { 1, 0, 3 }, { 2, 1, 4 }, { 0, 1, 1 }, { 0, 0, 4 }, { 1, 1, 3 }, { 2, 0, 1 } };
	for (uint32_t mip = 0; mip < 2; mip++)
		for (uint32_t filter = 0; filter < 2; filter++)
			for (uint32_t f = 0; f < 6; f++)
			{
				const uint32_t t = config * 24u + mip * 12u + filter * 6u + f;
				const DecodeLodSampler smp = { filter, t & 3u, ((t >> 2) + t) & 3u, mip };
				check_table(tag, ch, grids, batch[0], tile[0], formats[f], smp, t);
			}
}

/* 64 points at the level-0 block corners (bx i, by j), i, j even in 2 .. 16, of the 17 x 17-block chain with lambda = 0.5,
 * BILINEAR, MIP_LINEAR: in the level-0 pass the four taps of a point lie in four blocks and no two points share one -- 256
 * distinct blocks, eight full batches -- and the level-1 pass follows.  (u = i / 17 is not a binary32, but u W is within 2^-17 of
 * the corner: the taps are the corner's.) */
static void corners(int bx, int by)
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	const Chain ch = make_chain(bx, by, 17u * (uint32_t)bx, 17u * (uint32_t)by, 1, 0, 0, tabs.data(), batch[0]);
	Grid g = { 0, 64, 1, {}, {}, true, 0.0f };
	for (uint32_t j = 2; j <= 16; j += 2)
		for (uint32_t i = 2; i <= 16; i += 2) { g.uv.push_back((float)i / 17.0f); g.uv.push_back((float)j / 17.0f); g.lod.push_back(0.5f); }
	char tag[64];
	snprintf(tag, sizeof(tag), "%dx%d corners", bx, by);
	const Format f = { 1, 0, 3 };
	for (uint32_t mip = 0; mip < 2; mip++)
	{
		std::vector<LodTileCount> per_tile;
		const DecodeLodSampler smp = { 1, 0, 0, mip };
		check_table(tag, ch, { g }, batch[0], tile[0], f, smp, 0, &per_tile);
		// MIP_NEAREST at 0.5: level 0 alone; MIP_LINEAR: levels 0 and 1, and level 1 has at most 9 x 9 blocks
		const bool ok = per_tile.size() == 1 && per_tile[0].passes == 1u + mip && per_tile[0].level_mask == (mip ? 3u : 1u) &&
		                (mip ? per_tile[0].blocks > 256u && per_tile[0].blocks <= 256u + 81u && per_tile[0].batches >= 9u : per_tile[0].blocks == 256u && per_tile[0].batches == 8u);
		printf("%s mip %u: tiles %zu passes %u batches %u blocks %u\n", tag, mip, per_tile.size(), per_tile.empty() ? 0u : per_tile[0].passes,
		       per_tile.empty() ? 0u : per_tile[0].batches, per_tile.empty() ? 0u : per_tile[0].blocks);
		if (!ok) fail("the corner tile does not run eight full batches of 256 blocks in its level-0 pass", tag, 0, (long)mip);
	}
}

/* A chain whose odd levels are F16 under the HDR profile and hold reserved-mode blocks only -- NaN everywhere -- sampled at even
 * integer lambda (with a bias: lod + lod_bias is the even integer): no NaN may reach a result. */
static void nan_neighbours(int bx, int by)
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, 1);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	const Chain ch = make_chain(bx, by, 17u * (uint32_t)bx, 17u * (uint32_t)by, 1, 3 /* the HDR profile */, 0, tabs.data(), batch[0], true);
	char tag[64];
	snprintf(tag, sizeof(tag), "%dx%d NaN neighbours", bx, by);
	// (the odd levels do decode to NaN, every component of every texel)
	for (uint32_t l = 1; l < ch.levels(); l += 2)
		for (size_t k = 0; k < ch.whole[l].size(); k += 2)
		{
			uint16_t h;
			memcpy(&h, ch.whole[l].data() + k, 2);
			if ((h & 0x7FFFu) <= 0x7C00u) { fail("an odd level holds a number", tag, (long)l, (long)k); break; }
		}
	Grid g = random_grid(0, 29, 6, -0.25f, 1.25f, 0.0f, 0.0f, true, -3.0f);
	for (size_t k = 0; k < g.lod.size(); k++) g.lod[k] = 3.0f + (float)(2u * (rnd() % ((ch.levels() + 1u) / 2u)));
	const Format f = { 0, 1, 4 };
	for (uint32_t mip = 0; mip < 2; mip++)
		for (uint32_t filter = 0; filter < 2; filter++)
		{
			std::vector<LodTileCount> per_tile;
			const DecodeLodSampler smp = { filter, 1, 2, mip };
			check_table(tag, ch, { g }, batch[0], tile[0], f, smp, 0, &per_tile);
			for (const LodTileCount& n : per_tile)
				if (n.level_mask & 0xAAAAAAAAu) fail("a tile ran a pass over a level of weight zero", tag, 0, (long)n.level_mask);
		}
	// (check_table has compared every byte with the model, which reads the levels of non-zero weight only: a NaN would differ --
	//  U8 levels hold none, so the model's values are numbers)
}

static DecodeLodLaunch plain_grid(uint32_t first, uint32_t levels, uint32_t z, uint32_t ox, uint32_t oy, const float* uv, size_t crow, const float* lod, size_t lrow, float bias,
                                  void* out, size_t row, size_t plane)
{
	DecodeLodLaunch g;
	memset(&g, 0, sizeof(g));
	g.first_entry = first; g.level_count = levels; g.z = z; g.out_x = ox; g.out_y = oy;
	g.d_coords = uv; g.coord_row_pitch = crow; g.d_lod = lod; g.lod_row_pitch = lrow; g.lod_bias = bias; g.d_out = out; g.row_pitch = row; g.plane_pitch = plane;
	return g;
}

/* The table of a hand-computed case (6x6): entries 0 .. 2 are a chain of 100 x 60 x 2 U8, 50 x 30 x 2 F16 and 25 x 15 x 2 F32, entry 3
 * is 64 x 64 U8.  A line for the table, then the levels of a few lambda under both mip filters. */
static int tables()
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 6, 6, 1);
	const DecodeImage images[4] = { make_image(6, 6, 100, 60, 2, 0, 0, tabs.data()), make_image(6, 6, 50, 30, 2, 0, 1, tabs.data()),
	                                make_image(6, 6, 25, 15, 2, 0, 2, tabs.data()), make_image(6, 6, 64, 64, 1, 0, 0, tabs.data()) };
	static uint8_t sink[16];
	static float uv[2], lod[1];
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 2; format.layout = 0; format.channels = 2;
	const DecodeLodSampler smp = { 1, 3, 1, 1 };
	const std::vector<DecodeLodLaunch> grids = { plain_grid(0, 3, 1, 100, 1, uv, 200, lod, 100, 0.5f, sink, 100, 100), plain_grid(3, 1, 0, 9, 5, uv, 24, lod, 16, 0.0f, sink, 12, 70),
	                                             plain_grid(1, 2, 0, 20, 17, uv, 40, nullptr, 20, -1.0f, sink, 20, 340) };
	const std::vector<const uint8_t*> streams(4, nullptr);
	std::vector<uint8_t> table(decode_lod_bytes(grids.data(), (uint32_t)grids.size()));
	const uint32_t total = decode_lod_build(table.data(), images, streams.data(), format, smp, grids.data(), (uint32_t)grids.size());
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeLodRecord* rec = reinterpret_cast<const DecodeLodRecord*>(table.data() + image_set_records_offset(head->count));
	printf("table: bytes %zu levels_at %zu level_bytes %zu count %u total %u returned %u first", table.size(), decode_lod_levels_offset(head->count), sizeof(DecodeLodLevel),
	       head->count, head->total, total);
	for (uint32_t i = 0; i < head->count; i++) printf(" %u", first[i]);
	printf(" records");
	for (uint32_t i = 0; i < head->count; i++)
	{
		printf(" [tw %u th %u tiles_x %u levels %zu level_count %u z %u out_x %u out_y %u coord_row %zu has_lod %u lod_row %zu bias_x4 %d row %zu plane %zu x_step %u filter %u"
		       " address_x %u address_y %u mip_filter %u type %u layout %u channels %u dims",
		       1u << rec[i].tw_log2, 64u >> rec[i].tw_log2, rec[i].tiles_x, rec[i].levels, rec[i].level_count, rec[i].z, rec[i].out_x, rec[i].out_y, rec[i].coord_row,
		       rec[i].lod ? 1u : 0u, rec[i].lod_row, (int)(rec[i].lod_bias * 4.0f), rec[i].row, rec[i].fmt.plane, rec[i].x_step, rec[i].filter, rec[i].address_x,
		       rec[i].address_y, rec[i].mip_filter, rec[i].fmt.type, rec[i].fmt.layout, rec[i].fmt.channels);
		for (uint32_t l = 0; l < rec[i].level_count; l++)
		{
			const DecodeLodLevel lv = LevelsOfGrid{ table.data() + rec[i].levels }(l);
			printf(" %ux%ut%u", lv.img.dim_x, lv.img.dim_y, lv.img.data_type);
		}
		printf("]");
	}
	printf("\n");
	// the levels of a few lambda' in a chain of 5 levels: "lambda <hex> mip m: l0 l1 g" (l1 -1: one level)
	const float inf = __builtin_inff();
	const float lams[] = { -1.0f, 0.0f, -0.0f, 0.5f, 1.0f, 1.5f, 4.0f, 7.0f, inf, -inf, 0.49999997f, 0.50000006f, 1e-30f, 3.75f, 2.0000002f };
	for (float lam : lams)
		for (uint32_t mip = 0; mip < 2; mip++)
		{
			const LodLevels lv = lod_levels(mip, 5u, lam);
			printf("lambda %a mip %u: %u %d %a\n", (double)lam, mip, lv.l0, lv.l1 == LOD_NO_LEVEL ? -1 : (int)lv.l1, lv.g);
		}
	// validity: "valid u v lambda: 0/1"
	const float big = 16384.0f, next = __builtin_nextafterf(big, inf), nan = __builtin_nanf("");
	const float pts[][3] = { { big, -big, 0.0f }, { next, 0.0f, 0.0f }, { 0.0f, -next, 0.0f }, { nan, 0.0f, 0.0f }, { 0.0f, inf, 0.0f }, { 0.0f, 0.0f, nan }, { 0.0f, 0.0f, inf },
	                         { 0.0f, 0.0f, -inf } };
	for (const float* p : pts) printf("valid %a %a %a: %d\n", (double)p[0], (double)p[1], (double)p[2], lod_valid(p[0], p[1], p[2]) ? 1 : 0);
	return 0;
}

/* `blocks <filter> <address_x> <address_y> <mip_filter> <block_x> <block_y> <dim_x> <dim_y> <levels> <out_x> <out_y> <coords> <lod>`:
 * the tiles of the grid whose out_x * out_y (u, v) pairs and levels of detail (binary32, row by row) are the two files' bytes
 * (lod "-": NULL), run over the first `levels` levels of the mip chain of a dim_x x dim_y image of constant-colour blocks; prints
 * the tiles, the level passes, the batches and the blocks they decoded (tools/time_decode_lod.py). */
static int blocks_mode(char** a)
{
	const uint32_t filter = (uint32_t)atoi(a[0]), ax = (uint32_t)atoi(a[1]), ay = (uint32_t)atoi(a[2]), mip = (uint32_t)atoi(a[3]), bx = (uint32_t)atoi(a[4]), by = (uint32_t)atoi(a[5]);
	const uint32_t dim_x = (uint32_t)atoi(a[6]), dim_y = (uint32_t)atoi(a[7]), levels = (uint32_t)atoi(a[8]), ox = (uint32_t)atoi(a[9]), oy = (uint32_t)atoi(a[10]);
	if (filter > 1 || ax > 3 || ay > 3 || mip > 1 || bx < 4 || bx > 12 || by < 4 || by > 12 || dim_x < 1 || dim_y < 1 || dim_x > 65536 || dim_y > 65536 || levels < 1 || levels > 32 ||
	    ox < 1 || ox > 65535 || oy < 1 || oy > 65535)
		return 2;
	std::vector<float> uv((size_t)ox * oy * 2u), lod((size_t)ox * oy);
	FILE* fp = fopen(a[11], "rb");
	if (!fp || fread(uv.data(), sizeof(float), uv.size(), fp) != uv.size()) return 2;
	fclose(fp);
	const bool has_lod = strcmp(a[12], "-") != 0;
	if (has_lod)
	{
		fp = fopen(a[12], "rb");
		if (!fp || fread(lod.data(), sizeof(float), lod.size(), fp) != lod.size()) return 2;
		fclose(fp);
	}
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], (int)bx, (int)by, 1);
	std::vector<DecodeImage> images;
	std::vector<std::vector<uint8_t>> blocks;
	for (uint32_t l = 0; l < levels; l++)
	{
		images.push_back(make_image((int)bx, (int)by, dim_x >> l ? dim_x >> l : 1u, dim_y >> l ? dim_y >> l : 1u, 1, 0, 0, tabs.data()));
		const size_t nblocks = (size_t)images[l].blocks_x * images[l].blocks_y;
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
	const DecodeLodLaunch g = plain_grid(0, levels, 0, ox, oy, uv.data(), 2u * (size_t)ox, has_lod ? lod.data() : nullptr, ox, 0.0f, out.data(), ox, (size_t)ox * oy);
	const DecodeLodSampler smp = { filter, ax, ay, mip };
	std::vector<uint8_t> table(decode_lod_bytes(&g, 1));
	const uint32_t tiles = decode_lod_build(table.data(), images.data(), streams.data(), format, smp, &g, 1);
	DecodeLodRecord rec;
	memcpy(&rec, table.data() + image_set_records_offset(1), sizeof(rec));
	const LevelsOfGrid level = { table.data() + rec.levels };
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	unsigned long long passes = 0, batches = 0, decoded = 0;
	for (uint32_t t = 0; t < tiles; t++)
	{
		const LodTileCount n = decode_lod_tile<1, 0>(rec, level, t, batch[0], tile[0]);
		passes += n.passes; batches += n.batches; decoded += n.blocks;
	}
	printf("tiles %u passes %llu batches %llu decoded %llu points %llu\n", tiles, passes, batches, decoded, (unsigned long long)ox * oy);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	if (argc == 15 && strcmp(argv[1], "blocks") == 0) return blocks_mode(argv + 2);
	const int footprints[4][2] = { { 4, 4 }, { 6, 6 }, { 10, 8 }, { 12, 12 } };
	uint32_t config = 0;
	for (const int* f : footprints)
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 4; dtype++) check(f[0], f[1], profile, dtype, config++);
	for (const int* f : footprints) corners(f[0], f[1]);
	for (const int* f : footprints) nan_neighbours(f[0], f[1]);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	printf("address mode pairs met: %d of 16\n", __builtin_popcount(g_pairs_seen));
	printf("%llu tiles, %llu level passes, %llu blocks decoded in %llu batches\n", g_tiles, g_passes, g_decoded, g_batches);
	printf("most distinct levels in a tile: %u\n", g_most_levels);
	printf("g = 0 met: %d, g != 0 met: %d\n", g_single ? 1 : 0, g_blended ? 1 : 0);
	if (g_most_levels < 4u) { fprintf(stderr, "no tile had four distinct levels\n"); return 1; }
	if (!g_single || !g_blended) { fprintf(stderr, "g = 0 and g != 0 did not both occur\n"); return 1; }
	return g_bad == 0 ? 0 : 1;
}
