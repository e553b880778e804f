// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: the fused block quality routine (wave_quality.h: the batched decoder with the comparing texel sink)
// against the path it replaces -- decode_row_batch into an image, then metric_texel_terms / metric_hdr_terms over it -- on
// the host, as plain sequential code under the sanitizers.  Random 16-byte patterns (most of them error blocks or odd but
// legal modes) mixed with constant-colour blocks (UNORM16 and FP16), footprints 4x4, 6x6, 12x12, 3x3x3 and 6x6x6, the three
// decode types against originals of every type, an identity and two other swizzles, the four profiles.  Required: every
// texel's terms bit equal, the per-block and total sums within 1e-12 relative, the peak equal, nothing written past the
// per-block records.
//   g++ -std=c++17 -O1 -DASTC_WAVE_EMU=1 -ffp-contract=off -fsanitize=address,undefined -I astc-encoder_amd/csrc
//       tests/harness/block_quality_check.cpp -o block_quality_check
#define ASTC_VARIANT v_check
#define ASTC_ENABLE_HDR 1
#include "backend.h"
#include "wave_quality.h"
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

using namespace astcd;

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (uint32_t)(g_x >> 16); }

static long g_checked = 0, g_bad = 0;

static bool close_enough(double a, double b) { return fabs(a - b) <= 1e-12 * fmax(fabs(a), fabs(b)); }

static void fail(const char* what, const char* tag, long at, double a, double b)
{
	if (++g_bad <= 20) fprintf(stderr, "%s: %s at %ld: %.17g vs %.17g\n", tag, what, at, a, b);
}

template <bool HDR>
static void check(int bx, int by, int bz, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, int profile, uint32_t otype, uint32_t dtype, const uint32_t swz[4])
{
	constexpr int NT = HDR ? 16 : 8;
	const int fstop_lo = -1, fstop_hi = 1;
	char tag[128];
	snprintf(tag, sizeof(tag), "%dx%dx%d %ux%ux%u profile %d original %u decode %u swizzle %u%u%u%u%s", bx, by, bz, dim_x, dim_y, dim_z, profile, otype, dtype,
	         swz[0], swz[1], swz[2], swz[3], HDR ? " hdr" : "");
	DecodeImage img;
	memset(&img, 0, sizeof(img));
	img.dim_x = dim_x; img.dim_y = dim_y; img.dim_z = dim_z;
	img.data_type = dtype;
	for (int i = 0; i < 4; i++) img.swz[i] = swz[i];
	img.block_x = bx; img.block_y = by; img.block_z = bz;
	img.blocks_x = (dim_x + bx - 1) / bx; img.blocks_y = (dim_y + by - 1) / by; img.blocks_z = (dim_z + bz - 1) / bz;
	img.profile = (uint32_t)profile;
	decode_image_prepare(img);
	std::vector<DecodeTables> tabs(1);
	decode_tables_build(tabs[0], bx, by, bz);
	img.tabs = tabs.data();
	const size_t nblocks = (size_t)img.blocks_x * img.blocks_y * img.blocks_z, texels = (size_t)dim_x * dim_y * dim_z;

	// the stream
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
	// the original: every bit pattern of its type (NaNs, infinities and negative values among the halves and floats)
	const size_t obytes = texels * (otype == 0 ? 4 : otype == 1 ? 8 : 16);
	std::vector<uint8_t> orig(obytes);
	for (size_t i = 0; i < obytes; i++) orig[i] = (uint8_t)rnd();
	if (otype == 2)
		for (size_t i = 0; i < texels * 4; i++)
			if (rnd() & 1u) { const float v = (float)(rnd() % 4096u) / 1024.0f; memcpy(orig.data() + i * 4, &v, 4); }
	const std::vector<uint8_t> orig_before = orig, blocks_before = blocks;

	// decode, then compare: the path the fused routine replaces
	std::vector<uint8_t> decoded(texels * (dtype == 0 ? 4 : dtype == 1 ? 8 : 16), 0xA5);
	img.data = decoded.data();
	std::vector<DecodeBatch> batch(1);
	memset(static_cast<void*>(batch.data()), 0xCD, sizeof(DecodeBatch));
	for (uint32_t z = 0; z < img.blocks_z; z++)
		for (uint32_t y = 0; y < img.blocks_y; y++)
			for (uint32_t x0 = 0; x0 < img.blocks_x; x0 += DECODE_BATCH)
				decode_row_batch(img, blocks.data(), x0, y, z, i_min(DECODE_BATCH, (int)(img.blocks_x - x0)), batch[0]);
	std::vector<float> want(texels * NT);
	std::vector<double> want_block(nblocks * 4, 0.0);
	double want_sum[NT] = {};
	float want_peak = 0.0f;
	for (size_t t = 0; t < texels; t++)
	{
		float c1[4], c2[4];
		float* e = want.data() + t * NT;
		const float m = metric_texel_terms(orig.data(), otype, decoded.data(), dtype, t, nullptr, e, c1, c2);
		if (HDR) metric_hdr_terms(c1, c2, fstop_lo, fstop_hi, e + (HDR ? 8 : 0));
		want_peak = m > want_peak ? m : want_peak;
		for (int k = 0; k < NT; k++) want_sum[k] += (double)e[k];
		const uint32_t x = (uint32_t)(t % dim_x), y = (uint32_t)(t / dim_x % dim_y), z = (uint32_t)(t / ((size_t)dim_x * dim_y));
		const size_t b = ((size_t)(z / bz) * img.blocks_y + y / by) * img.blocks_x + x / bx;
		for (int k = 0; k < 4; k++) want_block[b * 4 + k] += (double)e[k];
	}

	// the fused routine, run by run as the kernel takes them
	img.data = nullptr;
	std::vector<uint32_t> trace_bits(texels * NT, 0xFFFFFFFFu);     // (no term is this NaN: an unvisited texel shows)
	const double guard = -12345.0;
	std::vector<double> got_block(nblocks * 4 + 8, guard);
	const uint32_t runs_x = (img.blocks_x + DECODE_BATCH - 1) / DECODE_BATCH;
	const size_t runs = (size_t)runs_x * img.blocks_y * img.blocks_z;
	std::vector<double> partials(runs * METRIC_SUMS_HDR, guard);
	std::unique_ptr<QualitySink<HDR>> sink(new QualitySink<HDR>);
	std::vector<QualityScratch> scratch(1);
	memset(static_cast<void*>(scratch.data()), 0xCD, sizeof(QualityScratch));
	size_t run = 0;
	for (uint32_t z = 0; z < img.blocks_z; z++)
		for (uint32_t y = 0; y < img.blocks_y; y++)
			for (uint32_t x0 = 0; x0 < img.blocks_x; x0 += DECODE_BATCH, run++)
			{
				sink->begin(orig.data(), otype, fstop_lo, fstop_hi, true, scratch.data());
				sink->trace = reinterpret_cast<float*>(trace_bits.data());
				quality_row_batch<HDR>(img, blocks.data(), x0, y, z, i_min(DECODE_BATCH, (int)(img.blocks_x - x0)), batch[0], *sink,
				                       got_block.data() + 4, partials.data() + run, runs);
			}

	g_checked++;
	if (orig != orig_before || blocks != blocks_before) fail("an input changed", tag, 0, 0, 0);
	if (memcmp(trace_bits.data(), want.data(), texels * NT * 4) != 0)
	{
		for (size_t i = 0; i < texels * NT; i++)
		{
			uint32_t w;
			memcpy(&w, &want[i], 4);
			if (w != trace_bits[i]) { float g; memcpy(&g, &trace_bits[i], 4); fail("term", tag, (long)i, (double)g, (double)want[i]); break; }
		}
	}
	for (int i = 0; i < 4; i++)
		if (got_block[i] != guard || got_block[4 + nblocks * 4 + i] != guard) fail("a write outside the block records", tag, i, 0, 0);
	for (size_t i = 0; i < nblocks * 4; i++)
		if (!close_enough(got_block[4 + i], want_block[i])) fail("block sum", tag, (long)i, got_block[4 + i], want_block[i]);
	double got_sum[METRIC_SUMS_HDR] = {};
	for (size_t r = 0; r < runs; r++)
		for (int k = 0; k < METRIC_SUMS_HDR; k++)
		{
			const double p = partials[(size_t)k * runs + r];
			const bool written = k < 9 || (HDR && k >= METRIC_HDR_FIRST);
			if (!written) { if (p != guard) fail("a partial that is not the kernel's", tag, k, p, guard); continue; }
			got_sum[k] = k == QUALITY_PEAK ? (p > got_sum[k] ? p : got_sum[k]) : got_sum[k] + p;
		}
	for (int k = 0; k < 8; k++) if (!close_enough(got_sum[k], want_sum[k])) fail("sum", tag, k, got_sum[k], want_sum[k]);
	if (HDR) for (int k = 0; k < 8; k++) if (!close_enough(got_sum[METRIC_HDR_FIRST + k], want_sum[8 + k])) fail("hdr sum", tag, k, got_sum[METRIC_HDR_FIRST + k], want_sum[8 + k]);
	if (got_sum[QUALITY_PEAK] != (double)want_peak) fail("peak", tag, 0, got_sum[QUALITY_PEAK], (double)want_peak);
	// ... and the per-block records add up to the totals
	for (int k = 0; k < 4; k++)
	{
		double s = 0.0;
		for (size_t b = 0; b < nblocks; b++) s += got_block[4 + b * 4 + k];
		if (!close_enough(s, got_sum[k])) fail("blocks against the total", tag, k, s, got_sum[k]);
	}
}

int main()
{
	const int footprints[5][3] = { { 4, 4, 1 }, { 6, 6, 1 }, { 12, 12, 1 }, { 3, 3, 3 }, { 6, 6, 6 } };
	const uint32_t swizzles[3][4] = { { 0, 1, 2, 3 }, { 2, 1, 0, 3 }, { 1, 1, 1, 0 } };
	const uint32_t z_swizzle[4] = { 0, 3, 6, 5 };        // (a normal map's: r, a, the reconstructed z, 1)
	for (const int* f : footprints)
	{
		// 34 blocks per row (a full run and one of two blocks), the last block partial in every axis; two block rows / layers
		const uint32_t dim_x = 34u * f[0] - (uint32_t)f[0] / 2u, dim_y = 2u * f[1] - 1u, dim_z = f[2] == 1 ? (f[0] == 6 ? 2u : 1u) : (uint32_t)f[2] + 1u;
		for (int profile = 0; profile < 4; profile++)
			for (uint32_t dtype = 0; dtype < 3; dtype++)
				for (int s = 0; s < 4; s++)
				{
					const uint32_t* swz = s < 3 ? swizzles[s] : z_swizzle;
					const uint32_t otype = (uint32_t)(profile + dtype + s) % 3u;
					if (profile >= 2 && s != 2) check<true>(f[0], f[1], f[2], dim_x, dim_y, dim_z, profile, otype, dtype, swz);
					else check<false>(f[0], f[1], f[2], dim_x, dim_y, dim_z, profile, otype, dtype, swz);
				}
	}
	// one block, and a single column of a second one
	const uint32_t rgba[4] = { 0, 1, 2, 3 };
	check<false>(6, 6, 1, 1, 1, 1, 0, 0, 0, rgba);
	check<false>(6, 6, 1, 7, 6, 1, 0, 0, 0, rgba);
	check<true>(4, 4, 4, 9, 6, 5, 3, 1, 1, rgba);
	printf("%ld configurations, %ld mismatches\n", g_checked, g_bad);
	return g_bad == 0 ? 0 : 1;
}
