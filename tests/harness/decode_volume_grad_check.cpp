// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the gradients of the volume sampler, astcenc_amd_sample_volume_grad_device (decode_volume_grad.h: the
// host-built table and decode_volume_grad_tile -- the levels of every point, a pass per distinct level with all eight taps of a
// trilinear point, the difference sums along x, y and z against the upstream gradient, the blend) against decode_row_batch of
// every whole level followed by the definition written out in plain C++ below from the header's comment, on the host, as
// sequential code under the sanitizers.  A chain is the full mip chain of a 20 x 14 x 9 volume, every level a random stream of
// its own (random patterns mixed with constant-colour and reserved-mode blocks).  Footprints 4x4 (slices), 3x3x3 and 5x5x4;
// chains of U8 levels (LDR profile), of F16 and of F32 levels and one mixing the three (HDR profile).  Each chain is
// differentiated with both filters x both mip filters and six formats of grad_out -- every tensor type with both layouts, one to
// four channels -- the address modes turning from table to table so that every triple is met, and per table several grids:
// random (u, v, w) in [-0.25, 1.25] with random lambda in [-1, L + 0.5]; integer lambda; texel centres of level 1 on all three
// axes and on each alone; the special values of u, v, w and lambda; lod NULL with a bias; grad_lod NULL; grids of 1, 2, 3, 5 and 9
// rows whose width is no multiple of the tile's (the three tile shapes); tight and padded pitches alternate for all five
// buffers (the padding of the three inputs holds NaNs); a NaN and the infinities among the upstream values.
// Required: every element of grad_coords and grad_lod equal to the model's bits, every other byte of both buffers intact, the
// inputs unchanged, as many tiles as the grids' sizes need, and per tile a pass for every level its points need -- level l0 + 1 of
// weight zero among them exactly where grad_lod is wanted and lambda' is not clamped -- and no other.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/decode_volume_grad_check.cpp -o decode_volume_grad_check
// `decode_volume_grad_check tables` prints the table of a hand-computed case instead (tests/test_decode_volume_grad_cpu.py).
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "decode_volume_grad.h"
#define DECODE_CHECK_ITEM "grid"
#include "decode_lod_check_common.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

static const uint32_t RGBA[4] = { 0, 1, 2, 3 };

static unsigned long long g_passes = 0, g_tiles = 0, g_extra = 0;       // g_extra: points that read l0 + 1 at weight zero
static unsigned long long g_triples_seen = 0;                          // bit (address_x * 16 + address_y * 4 + address_z)
static unsigned g_shapes_seen = 0;                                     // bit tw_log2 of a record

/* A chain: per level the image, its stream and what the decoder writes for the whole of it. */
struct Chain {
	std::vector<DecodeImage> images;
	std::vector<std::vector<uint8_t>> blocks, whole;
	uint32_t levels() const { return (uint32_t)images.size(); }
};

/* The model (include/astcenc_amd.h), one operation at a time.  The address modes, on 64-bit integers; false: a BORDER tap outside ... */
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

/* ... the bilinear taps of a binary64 level coordinate along an axis: i0, the weights, how many taps the forward sums have ... */
struct Axis { int64_t i0; double w[2]; int n; };
static Axis model_axis(uint32_t filter, double x)
{
	Axis a;
	if (filter == 0) { a.i0 = (int64_t)std::floor(x); a.w[0] = 1.0; a.w[1] = 0.0; a.n = 1; return a; }
	volatile double t = x - 0.5;
	const double fl = std::floor(t);
	volatile double f = t - fl;
	volatile double w0 = 1.0 - f;
	a.i0 = (int64_t)fl; a.w[0] = w0; a.w[1] = f; a.n = f != 0.0 ? 2 : 1;
	return a;
}

/* ... w[0] * p[0] [+ w[1] * p[1]], a sum that starts as its first product ... */
static double model_over(const Axis& a, double p0, double p1)
{
	volatile double r = a.w[0] * p0;
	if (a.n > 1)
	{
		volatile double q = a.w[1] * p1;
		r = r + q;
	}
	return r;
}

static double model_sub(double a, double b)
{
	volatile double d = a - b;
	return d;
}

/* ... Dx, Dy, Dz and S of a level at the point for the upstream a[0 .. channels) ... */
struct Terms { double d[3], s; };
static Terms model_level_terms(const Chain& ch, int level, const DecodeLodSampler& smp, float u, float v, float w, const double* a, uint32_t channels)
{
	const DecodeImage& img = ch.images[(size_t)level];
	const size_t tb = img.data_type == 0 ? 4 : img.data_type == 1 ? 8 : 16;
	volatile double x = (double)u * (double)img.dim_x, y = (double)v * (double)img.dim_y, z = (double)w * (double)img.dim_z;
	const Axis ax = model_axis(smp.filter, x), ay = model_axis(smp.filter, y), az = model_axis(smp.filter, z);
	int64_t kx[2], ky[2], kz[2];
	bool in_x[2], in_y[2], in_z[2];
	for (int t = 0; t < 2; t++)
	{
		in_x[t] = model_address(smp.address_x, ax.i0 + t, (int64_t)img.dim_x, kx[t]);
		in_y[t] = model_address(smp.address_y, ay.i0 + t, (int64_t)img.dim_y, ky[t]);
		in_z[t] = model_address(smp.address_z, az.i0 + t, (int64_t)img.dim_z, kz[t]);
	}
	auto val = [&](int tx, int ty, int tz, uint32_t c) -> double
	{
		if (!in_x[tx] || !in_y[ty] || !in_z[tz]) return 0.0;
		return source_value(ch.whole[(size_t)level].data() + ((((size_t)kz[tz] * img.dim_y + (size_t)ky[ty]) * img.dim_x) + (size_t)kx[tx]) * tb, img.data_type, c);
	};
	// (a second term is formed only where the forward call has the tap: under NEAREST index i0 + 1 is never looked at)
	auto at = [&](int tx, int ty, int tz, uint32_t c) -> double { return smp.filter == 0 && (tx | ty | tz) ? 0.0 : val(tx, ty, tz, c); };
	volatile double sum_s = 0.0, sum_x = 0.0, sum_y = 0.0, sum_z = 0.0;
	for (uint32_t c = 0; c < channels; c++)
	{
		// the forward level sample, binary32: rows, planes, then the z taps
		double plane[2] = { 0.0, 0.0 };
		for (int tz = 0; tz < az.n; tz++)
		{
			double row[2] = { 0.0, 0.0 };
			for (int ty = 0; ty < ay.n; ty++) row[ty] = model_over(ax, at(0, ty, tz, c), ax.n > 1 ? at(1, ty, tz, c) : 0.0);
			plane[tz] = model_over(ay, row[0], row[1]);
		}
		const float s = (float)model_over(az, plane[0], plane[1]);
		volatile double ps = a[c] * (double)s;
		sum_s = c == 0 ? ps : sum_s + ps;
		if (smp.filter == 0) continue;
		double q[2] = { 0.0, 0.0 };
		for (int tz = 0; tz < az.n; tz++)
			q[tz] = model_over(ay, model_sub(val(1, 0, tz, c), val(0, 0, tz, c)), ay.n > 1 ? model_sub(val(1, 1, tz, c), val(0, 1, tz, c)) : 0.0);
		const double dsdx = model_over(az, q[0], q[1]);
		for (int tz = 0; tz < az.n; tz++)
			q[tz] = model_over(ax, model_sub(val(0, 1, tz, c), val(0, 0, tz, c)), ax.n > 1 ? model_sub(val(1, 1, tz, c), val(1, 0, tz, c)) : 0.0);
		const double dsdy = model_over(az, q[0], q[1]);
		q[1] = 0.0;
		for (int ty = 0; ty < ay.n; ty++)
			q[ty] = model_over(ax, model_sub(val(0, ty, 1, c), val(0, ty, 0, c)), ax.n > 1 ? model_sub(val(1, ty, 1, c), val(1, ty, 0, c)) : 0.0);
		const double dsdz = model_over(ay, q[0], q[1]);
		volatile double px = a[c] * dsdx, py = a[c] * dsdy, pz = a[c] * dsdz;
		sum_x = c == 0 ? px : sum_x + px;
		sum_y = c == 0 ? py : sum_y + py;
		sum_z = c == 0 ? pz : sum_z + pz;
	}
	Terms r;
	volatile double dx = sum_x * (double)img.dim_x, dy = sum_y * (double)img.dim_y, dz = sum_z * (double)img.dim_z;
	r.d[0] = smp.filter == 0 ? 0.0 : dx;
	r.d[1] = smp.filter == 0 ? 0.0 : dy;
	r.d[2] = smp.filter == 0 ? 0.0 : dz;
	r.s = sum_s;
	return r;
}

static uint32_t stored(double x)
{
	const float f = (float)x;
	uint32_t u;
	memcpy(&u, &f, 4);
	return (u & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : u;
}

static bool model_fine(float c) { return std::isfinite(c) && std::fabs((double)c) <= 16384.0; }

/* ... the point: validity, the levels, the blend, the difference along lambda; the levels it needs go into *level_mask. */
static void model_point(const Chain& ch, const DecodeLodSampler& smp, const float* uvw, float lod, float bias, const double* a, uint32_t channels, bool want_lod, uint32_t out[4],
                        uint32_t* level_mask)
{
	out[0] = out[1] = out[2] = out[3] = 0u;
	volatile float lambda = lod + bias;
	const float lam = lambda;
	if (!model_fine(uvw[0]) || !model_fine(uvw[1]) || !model_fine(uvw[2]) || std::isnan(lam)) return;
	const uint32_t L = ch.levels();
	const float top = (float)((int)L - 1);
	const float lc = lam < 0.0f ? 0.0f : lam > top ? top : lam;
	int l0;
	double g = 0.0;
	if (smp.mip_filter == 0)
	{
		volatile double sum = (double)lc + 0.5;
		l0 = (int)std::ceil(sum) - 1;
	}
	else
	{
		l0 = (int)std::floor((double)lc);
		g = (double)lc - (double)l0;
	}
	const bool slope = smp.mip_filter == 1 && lam >= 0.0f && lam < top;
	const Terms t0 = model_level_terms(ch, l0, smp, uvw[0], uvw[1], uvw[2], a, channels);
	*level_mask |= 1u << l0;
	Terms t1 = { { 0.0, 0.0, 0.0 }, 0.0 };
	if (g != 0.0 || (slope && want_lod))
	{
		t1 = model_level_terms(ch, l0 + 1, smp, uvw[0], uvw[1], uvw[2], a, channels);
		*level_mask |= 1u << (l0 + 1);
		if (g == 0.0) g_extra++;
	}
	for (int k = 0; k < 3; k++)
	{
		if (g != 0.0)
		{
			volatile double w0 = 1.0 - g;
			volatile double p0 = w0 * t0.d[k], p1 = g * t1.d[k];
			volatile double sum = p0 + p1;
			out[k] = stored(sum);
		}
		else out[k] = stored(t0.d[k]);
	}
	if (slope && want_lod)
	{
		volatile double d = t1.s - t0.s;
		out[3] = stored(d);
	}
}

struct Grid { uint32_t ox, oy; std::vector<float> uvw; std::vector<float> lod; bool has_lod; float bias; bool want_lod; };       // uvw: ox * oy triples, row by row

/* An upstream value the tensor type holds: its bits and its widening to binary32. */
static float upstream_value(uint32_t type, uint32_t kind, uint8_t* bits)
{
	float f = (rnd_unit() - 0.5f) * 8.0f;
	if (kind == 1) f = __builtin_nanf("");
	if (kind == 2) f = __builtin_inff();
	if (kind == 3) f = -__builtin_inff();
	uint32_t u;
	memcpy(&u, &f, 4);
	if (type == 0) { memcpy(bits, &u, 4); return f; }
	if (type == 2)
	{
		const uint16_t h = (uint16_t)(u >> 16);
		memcpy(bits, &h, 2);
		u &= 0xFFFF0000u;
		memcpy(&f, &u, 4);
		return f;
	}
	const uint16_t h = (uint16_t)model_bits(f, 1.0f, 0.0f, 1);
	memcpy(bits, &h, 2);
	uint8_t texel[8] = { 0 };
	memcpy(texel, &h, 2);
	return (float)source_value(texel, 1, 0);
}

/* One table of all `wanted` grids over one chain (entries first_entry .. of a call whose other entries are left null). */
static void check_table(const char* chain_tag, const Chain& ch, const std::vector<Grid>& wanted, DecodeBatch& batch, SampleTile& tile, const Format& f,
                        const DecodeLodSampler& smp, uint32_t turn)
{
	char tag[256];
	snprintf(tag, sizeof(tag), "%s -> filter %u address %u %u %u mip %u type %u layout %u channels %u", chain_tag, smp.filter, smp.address_x, smp.address_y, smp.address_z,
	         smp.mip_filter, f.type, f.layout, f.channels);
	const size_t eb = f.type == 0 ? 4 : 2;
	const bool planar = f.layout == 0;
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = f.type; format.layout = f.layout; format.channels = f.channels;
	const float scales[4] = { 0.017124754f, -0.5f, 3.0f, 1.0f / 255.0f }, biases[4] = { -2.1179039f, 0.25f, 100.0f, 0.0f };
	for (int c = 0; c < 4; c++) { format.scale[c] = scales[c]; format.bias[c] = biases[c]; }
	g_triples_seen |= 1ull << (smp.address_x * 16u + smp.address_y * 4u + smp.address_z);

	// (the chain is entries 1 .. L of the call: entry 0 is another image, which no grid may touch)
	const uint32_t first_entry = 1, L = ch.levels();
	std::vector<DecodeImage> images(1 + L);
	std::vector<const uint8_t*> streams(1 + L, nullptr);
	memset(static_cast<void*>(&images[0]), 0, sizeof(DecodeImage));
	for (uint32_t l = 0; l < L; l++) { images[1 + l] = ch.images[l]; streams[1 + l] = ch.blocks[l].data(); }

	const size_t guard = 16;        // floats
	const uint32_t count = (uint32_t)wanted.size();
	std::vector<DecodeLodGradLaunch> grids(count);
	std::vector<std::vector<uint8_t>> ups(count);
	std::vector<std::vector<float>> coords(count), lods(count), up_values(count);
	std::vector<std::vector<uint32_t>> gcs(count), gls(count);
	unsigned long long want_total = 0;
	for (uint32_t i = 0; i < count; i++)
	{
		const Grid& w = wanted[i];
		const uint32_t mix = (i * 7u + turn * 3u + 1u) * 11u;
		const bool padded = (mix & 1u) != 0u, coords_padded = (mix & 2u) != 0u, lod_padded = (mix & 4u) != 0u, gc_padded = (mix & 8u) != 0u, gl_padded = (mix & 16u) != 0u;
		const size_t row = (size_t)w.ox * (planar ? 1 : f.channels) + (padded ? 3 : 0);
		const size_t plane = planar ? row * w.oy + (padded ? 5 : 0) : 0;
		const size_t elements = planar ? plane * f.channels : row * w.oy;
		// grad_out: NaNs of the type everywhere, then the points' values (the first grids of a table hold a NaN and the infinities)
		ups[i].assign(elements * eb, 0xFF);
		up_values[i].assign((size_t)w.ox * w.oy * 4u, 0.0f);
		for (uint32_t j = 0; j < w.oy; j++)
			for (uint32_t x = 0; x < w.ox; x++)
				for (uint32_t c = 0; c < f.channels; c++)
				{
					const size_t p = (size_t)j * w.ox + x;
					const uint32_t kind = i < 2u && p % 37u == 5u ? 1u + (uint32_t)(p / 37u) % 3u : 0u;
					const size_t at = planar ? c * plane + j * row + x : j * row + (size_t)x * f.channels + c;
					up_values[i][p * 4u + c] = upstream_value(f.type, c == (p & 3u) % f.channels ? kind : 0u, ups[i].data() + at * eb);
				}
		// (odd paddings: the pitch of triples need not be even)
		const size_t crow = 3u * (size_t)w.ox + (coords_padded ? 5 : 0), lrow = (size_t)w.ox + (lod_padded ? 5 : 0);
		coords[i].assign(crow * w.oy, __builtin_nanf(""));
		lods[i].assign(lrow * w.oy, __builtin_nanf(""));
		for (uint32_t j = 0; j < w.oy; j++)
		{
			memcpy(coords[i].data() + j * crow, w.uvw.data() + (size_t)j * 3u * w.ox, 3u * (size_t)w.ox * sizeof(float));
			if (w.has_lod) memcpy(lods[i].data() + j * lrow, w.lod.data() + (size_t)j * w.ox, (size_t)w.ox * sizeof(float));
		}
		const size_t gcrow = 3u * (size_t)w.ox + (gc_padded ? 1 : 0), glrow = (size_t)w.ox + (gl_padded ? 7 : 0);
		// (grad_coords starts on an odd float: aligned to 4 bytes and no more)
		gcs[i].assign(guard + 1u + gcrow * w.oy + guard, 0xA5A5A5A5u);
		gls[i].assign(guard + glrow * w.oy + guard, 0xA5A5A5A5u);
		DecodeLodGradLaunch& g = grids[i];
		memset(&g, 0, sizeof(g));
		g.lod.first_entry = first_entry; g.lod.level_count = L;
		g.lod.out_x = w.ox; g.lod.out_y = w.oy;
		g.lod.d_coords = coords[i].data(); g.lod.coord_row_pitch = crow;
		g.lod.d_lod = w.has_lod ? lods[i].data() : nullptr; g.lod.lod_row_pitch = lrow;
		g.lod.lod_bias = w.bias;
		g.lod.d_out = ups[i].data();
		g.lod.row_pitch = row; g.lod.plane_pitch = plane;
		g.d_grad_coords = reinterpret_cast<float*>(gcs[i].data() + guard + 1u); g.grad_coord_row_pitch = gcrow;
		g.d_grad_lod = w.want_lod ? reinterpret_cast<float*>(gls[i].data() + guard) : nullptr; g.grad_lod_row_pitch = glrow;
		const uint32_t th = w.oy >= 5 ? 8u : w.oy >= 3 ? 4u : w.oy, tw = 64u / th;
		want_total += (unsigned long long)((w.ox + tw - 1u) / tw) * ((w.oy + th - 1u) / th);
	}
	std::vector<uint8_t> table(decode_volume_grad_bytes(grids.data(), count));
	const uint32_t total = decode_volume_grad_build(table.data(), images.data(), streams.data(), format, smp, grids.data(), count);
	const std::vector<uint8_t> table_before = table;
	const std::vector<std::vector<uint8_t>> blocks_before = ch.blocks, ups_before = ups;
	const std::vector<std::vector<float>> coords_before = coords, lods_before = lods;

	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const uint8_t* records = table.data() + image_set_records_offset(count);
	g_checked++;
	if (head->count != count || head->total != total || total != want_total) fail("the table's totals", tag, -1, (long)total);
	memset(static_cast<void*>(&tile), 0xCD, sizeof(SampleTile));
	std::vector<std::vector<LodTileCount>> did(count);
	for (uint32_t r = 0; r < head->total; r++)
	{
		const uint32_t g = image_set_find(first, head->count, r);
		const DecodeVolumeGradRecord rec = image_set_record<DecodeVolumeGradRecord>(reinterpret_cast<const uint32_t*>(records + (size_t)g * sizeof(DecodeVolumeGradRecord)));
		const LevelsOfGrid levels = { table.data() + rec.vol.levels };
		g_shapes_seen |= 1u << rec.vol.tw_log2;
		const LodTileCount n = with_build(rec.vol.fmt.type, rec.vol.fmt.layout, [&](auto t, auto l)
		{
			return decode_volume_grad_tile<decltype(t)::value, decltype(l)::value>(rec, levels, r - first[g], batch, tile);
		});
		if (n.passes > L || n.blocks > (uint32_t)VOLUME_TILE_BLOCKS * n.passes || n.batches * (uint32_t)DECODE_BATCH < n.blocks)
			fail("a tile's passes, batches and blocks", tag, g, (long)n.blocks);
		did[g].push_back(n);
		g_passes += n.passes; g_tiles++;
	}
	if (ch.blocks != blocks_before || table != table_before) fail("an input changed", tag, -1, 0);
	for (uint32_t i = 0; i < count; i++)
		if (memcmp(coords[i].data(), coords_before[i].data(), coords[i].size() * sizeof(float)) != 0 || memcmp(lods[i].data(), lods_before[i].data(), lods[i].size() * sizeof(float)) != 0 ||
		    ups[i] != ups_before[i])
			fail("the coordinates, the levels of detail or the upstream gradient changed", tag, i, 0);

	for (uint32_t i = 0; i < count; i++)
	{
		const DecodeLodGradLaunch& g = grids[i];
		const Grid& w = wanted[i];
		std::vector<uint32_t> want_gc(gcs[i].size(), 0xA5A5A5A5u), want_gl(gls[i].size(), 0xA5A5A5A5u);
		const uint32_t th = w.oy >= 5 ? 8u : w.oy >= 3 ? 4u : w.oy, tw = 64u / th, tiles_x = (w.ox + tw - 1u) / tw;
		std::vector<uint32_t> masks(did[i].size(), 0u);
		for (uint32_t j = 0; j < w.oy; j++)
			for (uint32_t x = 0; x < w.ox; x++)
			{
				const float* uvw = g.lod.d_coords + j * g.lod.coord_row_pitch + 3u * x;
				const float lod = g.lod.d_lod ? g.lod.d_lod[j * g.lod.lod_row_pitch + x] : 0.0f;
				double a[4];
				for (uint32_t c = 0; c < f.channels; c++)
				{
					volatile double p = (double)up_values[i][((size_t)j * w.ox + x) * 4u + c] * (double)format.scale[c];
					a[c] = p;
				}
				uint32_t out[4];
				model_point(ch, smp, uvw, lod, w.bias, a, f.channels, w.want_lod, out, &masks[(size_t)(j / th) * tiles_x + x / tw]);
				for (uint32_t k = 0; k < 3u; k++) want_gc[guard + 1u + j * g.grad_coord_row_pitch + 3u * x + k] = out[k];
				if (w.want_lod) want_gl[guard + j * g.grad_lod_row_pitch + x] = out[3];
			}
		for (size_t t = 0; t < did[i].size(); t++)
			if (did[i][t].level_mask != masks[t] || did[i][t].passes != (uint32_t)__builtin_popcount(masks[t])) fail("a tile's level passes are not the levels its points need", tag, i, (long)t);
		if (gcs[i] != want_gc)
		{
			size_t at = 0;
			while (gcs[i][at] == want_gc[at]) at++;
			fail(at < guard + 1u || at >= gcs[i].size() - guard ? "a guard float of grad_coords was written" : "grad_coords differs from the model (or padding was written)", tag, i,
			     (long)at - (long)guard - 1);
		}
		if (gls[i] != want_gl)
		{
			size_t at = 0;
			while (gls[i][at] == want_gl[at]) at++;
			fail(!w.want_lod ? "grad_lod was written though it is not wanted" : "grad_lod differs from the model (or padding or a guard was written)", tag, i, (long)at - (long)guard);
		}
	}
}

/* The full chain of a dim_x x dim_y x dim_z volume; dtype 3: levels of U8, F16, F32 in turn. */
static Chain make_chain(int bx, int by, int bz, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, int profile, uint32_t dtype, const DecodeTables* tabs, DecodeBatch& batch)
{
	Chain ch;
	for (uint32_t l = 0; ; l++)
	{
		const uint32_t w = dim_x >> l ? dim_x >> l : 1u, h = dim_y >> l ? dim_y >> l : 1u, d = dim_z >> l ? dim_z >> l : 1u;
		DecodeImage img = make_image(bx, by, bz, w, h, d, profile, dtype == 3 ? l % 3u : dtype, RGBA, tabs);
		ch.blocks.emplace_back();
		ch.whole.emplace_back();
		random_blocks(ch.blocks.back(), (size_t)img.blocks_x * img.blocks_y * img.blocks_z);
		decode_whole(img, ch.blocks.back(), ch.whole.back(), batch);
		ch.images.push_back(img);
		if (w == 1 && h == 1 && d == 1) break;
	}
	return ch;
}

static Grid random_grid(uint32_t ox, uint32_t oy, float lo, float hi, float l0, float l1, bool has_lod = true, float bias = 0.0f, bool want_lod = true)
{
	Grid g = { ox, oy, {}, {}, has_lod, bias, want_lod };
	for (uint32_t k = 0; k < ox * oy; k++)
	{
		for (int c = 0; c < 3; c++) g.uvw.push_back(lo + (hi - lo) * rnd_unit());
		g.lod.push_back(l0 + (l1 - l0) * rnd_unit());
	}
	return g;
}

static void check(int bx, int by, int bz, int profile, uint32_t dtype, uint32_t config)
{
	const uint32_t dim_x = 20u, dim_y = 14u, dim_z = 9u;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%dx%d %ux%ux%u profile %d type %u", bx, by, bz, dim_x, dim_y, dim_z, profile, dtype);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
	std::vector<DecodeBatch> batch(1);
	std::vector<SampleTile> tile(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	const Chain ch = make_chain(bx, by, bz, dim_x, dim_y, dim_z, profile, dtype, tabs.data(), batch[0]);
	const float top = (float)(ch.levels() - 1u), inf = __builtin_inff(), nan = __builtin_nanf("");

	std::vector<Grid> grids;
	grids.push_back(random_grid(33, 9, -0.25f, 1.25f, -1.0f, top + 1.5f));                          // anywhere, any level; 8 x 8 tiles
	grids.push_back(random_grid(13, 5, -0.25f, 1.25f, -1.0f, top + 1.5f, true, 0.0f, false));       // grad_lod NULL
	{
		// integer lambda: grad_lod is the right derivative and reads l0 + 1 at weight zero
		Grid g = random_grid(21, 4, 0.0f, 1.0f, 0.0f, 0.0f);
		for (size_t k = 0; k < g.lod.size(); k++) g.lod[k] = (float)(rnd() % ch.levels());
		grids.push_back(g);
		g.want_lod = false;                                                                       // ... and with grad_lod NULL does not
		g.ox = 42; g.oy = 2;
		grids.push_back(g);
	}
	{
		// the texel centres of level 1 (10 x 7 x 4): f = 0 on all three axes, then on each axis alone; the right-hand neighbours are read
		const uint32_t w = dim_x >> 1, h = dim_y >> 1, d = dim_z >> 1;
		Grid g = { 19, 4, {}, {}, true, 0.0f, true };
		for (uint32_t j = 0; j < g.oy; j++)
			for (uint32_t i = 0; i < g.ox; i++)
			{
				const float centre[3] = { ((float)(i * 3u % w) + 0.5f) / (float)w, ((float)(i * 5u % h) + 0.5f) / (float)h, ((float)(i * 7u % d) + 0.5f) / (float)d };
				for (uint32_t c = 0; c < 3u; c++) g.uvw.push_back(j == 0u || j == c + 1u ? centre[c] : rnd_unit());
				g.lod.push_back(1.0f);
			}
		grids.push_back(g);
	}
	grids.push_back(random_grid(35, 2, 0.0f, 1.0f, 0.0f, top, false, 1.5f));                        // 32 x 2 tiles; lod NULL: the bias alone
	grids.push_back(random_grid(70, 1, -3.0f, 3.0f, 0.0f, top + 1.0f, true, -0.75f));               // 64 x 1; REPEAT and MIRROR over several periods; a bias
	grids.push_back(random_grid(1, 1, 0.0f, 1.0f, 0.0f, top));
	{
		// the special values of u, v, w and lambda: every value on two axes at once, the third turning through the list
		const float big = 16384.0f, next = __builtin_nextafterf(big, inf);
		const float s[] = { 0.5f, 0.0f, -0.0f, 1.0f, 0.99999994f, 1e-30f, -0.25f, nan, inf, -inf, big, next, -big, -next, 1.0f / 28.0f, 1.5f };
		const float lam[] = { -1.0f, 0.0f, -0.0f, 0.5f, 1.0f, 1.5f, top, top + 3.0f, inf, -inf, nan, 0.49999997f, 0.50000006f, 1e-30f, top - 0.25f, top - 1.0f };
		const uint32_t n = sizeof(s) / sizeof(s[0]), m = sizeof(lam) / sizeof(lam[0]);
		Grid g = { n, n, {}, {}, true, 0.0f, true };
		for (uint32_t j = 0; j < n; j++)
			for (uint32_t i = 0; i < n; i++)
			{
				const float p[3] = { s[i], s[j], s[(i * 3u + j * 5u + config) % n] };
				for (uint32_t c = 0; c < 3u; c++) g.uvw.push_back(p[(c + config) % 3u]);
				g.lod.push_back(lam[(j * 5u + i + config) % m]);
			}
		grids.push_back(g);
	}

	// (every build: three types x two layouts; channels 1 to 4)
	const Format formats[6] = { { 1, 0, 3 }, { 2, 1, 4 }, { 0, 1, 1 }, { 0, 0, 4 }, { 1, 1, 2 }, { 2, 0, 1 } };
	for (uint32_t mip = 0; mip < 2; mip++)
		for (uint32_t filter = 0; filter < 2; filter++)
			for (uint32_t f = 0; f < 6; f++)
			{
				const uint32_t t = config * 24u + mip * 12u + filter * 6u + f;
				// (a base-4 counter with the table: 64 consecutive tables meet every triple)
				const DecodeLodSampler smp = { filter, t & 3u, (t >> 2) & 3u, mip, ((t >> 4) + (t >> 6)) & 3u };
				check_table(tag, ch, grids, batch[0], tile[0], formats[f], smp, t);
			}
}

/* The table of a hand-computed case (4x4x3): entries 0 .. 2 are a chain of 100 x 60 x 20 U8, 50 x 30 x 10 F16 and 25 x 15 x 5 F32.  One line. */
static int tables()
{
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], 4, 4, 3);
	const DecodeImage images[3] = { make_image(4, 4, 3, 100, 60, 20, 0, 0, RGBA, tabs.data()), make_image(4, 4, 3, 50, 30, 10, 0, 1, RGBA, tabs.data()),
	                                make_image(4, 4, 3, 25, 15, 5, 0, 2, RGBA, tabs.data()) };
	static uint16_t up[16];
	static float uvw[3], lod[1], gc[3], gl[1];
	DecodeTensorFormat format;
	memset(&format, 0, sizeof(format));
	format.type = 2; format.layout = 0; format.channels = 2;
	const DecodeLodSampler smp = { 1, 3, 1, 1, 2 };
	std::vector<DecodeLodGradLaunch> grids(2);
	memset(static_cast<void*>(grids.data()), 0, 2 * sizeof(DecodeLodGradLaunch));
	grids[0].lod.first_entry = 0; grids[0].lod.level_count = 3; grids[0].lod.out_x = 100; grids[0].lod.out_y = 1;
	grids[0].lod.d_coords = uvw; grids[0].lod.coord_row_pitch = 300; grids[0].lod.d_lod = lod; grids[0].lod.lod_row_pitch = 100; grids[0].lod.lod_bias = 0.5f;
	grids[0].lod.d_out = up; grids[0].lod.row_pitch = 100; grids[0].lod.plane_pitch = 100;
	grids[0].d_grad_coords = gc; grids[0].grad_coord_row_pitch = 301; grids[0].d_grad_lod = gl; grids[0].grad_lod_row_pitch = 101;
	grids[1] = grids[0];
	grids[1].lod.first_entry = 1; grids[1].lod.level_count = 2; grids[1].lod.out_x = 20; grids[1].lod.out_y = 17;
	grids[1].lod.coord_row_pitch = 60; grids[1].lod.d_lod = nullptr; grids[1].lod.lod_row_pitch = 20; grids[1].lod.row_pitch = 20; grids[1].lod.plane_pitch = 340;
	grids[1].grad_coord_row_pitch = 60; grids[1].d_grad_lod = nullptr; grids[1].grad_lod_row_pitch = 20;
	const std::vector<const uint8_t*> streams(3, nullptr);
	std::vector<uint8_t> table(decode_volume_grad_bytes(grids.data(), 2));
	const uint32_t total = decode_volume_grad_build(table.data(), images, streams.data(), format, smp, grids.data(), 2);
	const ImageSetTable* head = reinterpret_cast<const ImageSetTable*>(table.data());
	const uint32_t* first = reinterpret_cast<const uint32_t*>(table.data() + image_set_first_offset());
	const DecodeVolumeGradRecord* rec = reinterpret_cast<const DecodeVolumeGradRecord*>(table.data() + image_set_records_offset(head->count));
	printf("table: bytes %zu levels_at %zu level_bytes %zu count %u total %u returned %u first %u %u records", table.size(), decode_volume_grad_levels_offset(head->count),
	       sizeof(DecodeLodLevel), head->count, head->total, total, first[0], first[1]);
	for (uint32_t i = 0; i < head->count; i++)
	{
		const DecodeLodLevel* lv = reinterpret_cast<const DecodeLodLevel*>(table.data() + rec[i].vol.levels);
		printf(" [levels %zu level_count %u out_x %u out_y %u row %zu plane %zu has_up %u has_uvw %u uvw_row %zu address_x %u address_y %u address_z %u filter %u mip %u tw_log2 %u"
		       " tiles_x %u level0_z %u has_gc %u gc_row %zu has_gl %u gl_row %zu]",
		       rec[i].vol.levels, rec[i].vol.level_count, rec[i].vol.out_x, rec[i].vol.out_y, rec[i].vol.row, rec[i].vol.fmt.plane, rec[i].vol.out == up ? 1u : 0u,
		       rec[i].vol.coords == uvw ? 1u : 0u, rec[i].vol.coord_row, rec[i].vol.address_x, rec[i].vol.address_y, rec[i].vol.address_z, rec[i].vol.filter, rec[i].vol.mip_filter,
		       rec[i].vol.tw_log2, rec[i].vol.tiles_x, lv[0].img.dim_z, rec[i].grad_coords == gc ? 1u : 0u, rec[i].grad_coord_row, rec[i].grad_lod == gl ? 1u : 0u, rec[i].grad_lod_row);
	}
	printf("\n");
	return 0;
}

int main(int argc, char** argv)
{
	if (argc > 1 && strcmp(argv[1], "tables") == 0) return tables();
	const int footprints[3][3] = { { 4, 4, 1 }, { 3, 3, 3 }, { 5, 5, 4 } };
	// (profile, data type of the levels): LDR U8, HDR F16, HDR F32, HDR mixed
	const int chains[4][2] = { { 0, 0 }, { 3, 1 }, { 3, 2 }, { 3, 3 } };
	uint32_t config = 0;
	for (const int* f : footprints)
		for (const int* c : chains) check(f[0], f[1], f[2], c[0], (uint32_t)c[1], config++);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	printf("address mode triples met: %d of 64\n", __builtin_popcountll(g_triples_seen));
	printf("tile shapes met: %d\n", __builtin_popcount(g_shapes_seen));
	printf("%llu tiles, %llu level passes\n", g_tiles, g_passes);
	printf("points that read level l0 + 1 at weight zero: %llu\n", g_extra);
	if (g_extra == 0) { fprintf(stderr, "no point read level l0 + 1 at weight zero\n"); return 1; }
	return g_bad == 0 ? 0 : 1;
}
