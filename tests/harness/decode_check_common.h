// SPDX-License-Identifier: Apache-2.0
// Test infrastructure: what the harnesses of the windowed and the sampled decoders share (decode_region_check.cpp,
// decode_tensor_check.cpp, decode_scaled_check.cpp, decode_sample_check.cpp and, through decode_lod_check_common.h, those of the
// level-of-detail samplers): the random numbers, the count of checks and mismatches, a prepared DecodeImage, the pieces of the
// tensor model (include/astcenc_amd.h) that every tensor call ends in -- a stored texel's component widened, and the scaled,
// shifted value's bits by integer arithmetic -- and what the samplers' harnesses are made of: the dispatch on a tensor type and
// layout, random streams, an image decoded whole, files of floats read and of bytes written.
// Included after the harness has defined ASTC_VARIANT and included the decode_*.h it checks; DECODE_CHECK_ITEM, defined before,
// names what a mismatch is counted in ("region" unless a harness says "grid").
#pragma once
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace astcd;

#ifndef DECODE_CHECK_ITEM
#define DECODE_CHECK_ITEM "region"
#endif

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
inline uint32_t rnd() { g_x ^= g_x << 13; g_x ^= g_x >> 7; g_x ^= g_x << 17; return (uint32_t)(g_x >> 16); }
inline float rnd_unit() { return (float)(rnd() & 0xFFFFFFu) / 16777216.0f; }

static long g_checked = 0, g_bad = 0;

inline void fail(const char* what, const char* tag, long item, long at)
{
	if (++g_bad <= 20) fprintf(stderr, "%s: %s (" DECODE_CHECK_ITEM " %ld, at %ld)\n", tag, what, item, at);
}

inline DecodeImage make_image(int bx, int by, int bz, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, int profile, uint32_t dtype, const uint32_t swz[4],
                              const DecodeTables* tabs)
{
	DecodeImage img;
	memset(&img, 0, sizeof(img));
	img.dim_x = dim_x; img.dim_y = dim_y; img.dim_z = dim_z;
	img.data_type = dtype;
	for (int i = 0; i < 4; i++) img.swz[i] = swz[i];
	img.block_x = bx; img.block_y = by; img.block_z = bz;
	img.blocks_x = (dim_x + bx - 1) / bx; img.blocks_y = (dim_y + by - 1) / by; img.blocks_z = (dim_z + bz - 1) / bz;
	img.profile = (uint32_t)profile;
	decode_image_prepare(img);
	img.tabs = tabs;
	return img;
}

/* (a 2D footprint, the identity swizzle) */
inline DecodeImage make_image(int bx, int by, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, int profile, uint32_t dtype, const DecodeTables* tabs)
{
	const uint32_t rgba[4] = { 0, 1, 2, 3 };
	return make_image(bx, by, 1, dim_x, dim_y, dim_z, profile, dtype, rgba, tabs);
}

/* The model, one operation at a time: component c of a decoded texel (what the decoder writes for the whole image), widened to
 * binary64 -- exact for all three data types, so a harness whose model starts from binary32 narrows it back without loss ... */
inline double source_value(const uint8_t* texel, uint32_t dtype, uint32_t c)
{
	if (dtype == 0) return (double)texel[c];
	if (dtype == 1)
	{
		uint16_t h;
		memcpy(&h, texel + 2 * c, 2);
		// exact widening, written out: sign, exponent, mantissa
		const uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
		double v;
		if (e == 31) v = m ? __builtin_nan("") : __builtin_inf();
		else if (e != 0) v = __builtin_ldexp((double)(m | 0x400u), (int)e - 25);
		else v = __builtin_ldexp((double)m, -24);
		return (h & 0x8000u) ? -v : v;
	}
	float f;
	memcpy(&f, texel + 4 * c, 4);
	return (double)f;
}

/* ... scaled and shifted with two roundings, and the bits it is stored as (type 0 F32, 1 F16, 2 BF16). */
inline uint32_t model_bits(float s, float scale, float bias, uint32_t type)
{
	volatile float t = s * scale;
	volatile float yv = t + bias;
	const float y = yv;
	uint32_t u;
	memcpy(&u, &y, 4);
	const bool nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
	if (type == 0) return nan ? 0x7FC00000u : u;
	if (type == 2) return nan ? 0x7FC0u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
	if (nan) return 0x7E00u;
	// binary16, round to nearest even, from the integer fields
	const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7FFFFFFFu;
	if (a >= 0x7F800000u) return sign | 0x7C00u;
	const int e = (int)(a >> 23) - 127;
	if (e > 15) return sign | 0x7C00u;
	uint64_t m = (a & 0x7FFFFFu) | (a >> 23 ? 0x800000u : 0u);       // 24-bit significand, value m * 2^(e - 23) (subnormal floats: e = -126 by the next line)
	const int ee = a >> 23 ? e : -126;
	// result in units of 2^-24 (the binary16 subnormal step) when below 2^-14, else normal with 10 fraction bits
	int shift = ee >= -14 ? 13 : 13 + (-14 - ee);
	if (shift > 40) return sign;
	const uint64_t q = m >> shift, rem = m & (((uint64_t)1 << shift) - 1u), half = (uint64_t)1 << (shift - 1);
	uint64_t r = q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
	// r holds the implicit bit at 1 << 10 for normals: adding the biased exponent - 1 folds a mantissa carry into the exponent
	const uint32_t out = ee >= -14 ? (uint32_t)(((uint64_t)(ee + 14) << 10) + r) : (uint32_t)r;
	return out >= 0x7C00u ? sign | 0x7C00u : sign | out;
}

struct Format { uint32_t type, layout, channels; };

/* fn(type, layout) with the tensor type and layout as constants: the kernels' one build per type and layout. */
template <class Fn>
static auto with_build(uint32_t type, uint32_t layout, Fn fn)
{
	switch (type * 2u + layout)
	{
	case 0: return fn(std::integral_constant<uint32_t, 0>(), std::integral_constant<uint32_t, 0>());
	case 1: return fn(std::integral_constant<uint32_t, 0>(), std::integral_constant<uint32_t, 1>());
	case 2: return fn(std::integral_constant<uint32_t, 1>(), std::integral_constant<uint32_t, 0>());
	case 3: return fn(std::integral_constant<uint32_t, 1>(), std::integral_constant<uint32_t, 1>());
	case 4: return fn(std::integral_constant<uint32_t, 2>(), std::integral_constant<uint32_t, 0>());
	default: return fn(std::integral_constant<uint32_t, 2>(), std::integral_constant<uint32_t, 1>());
	}
}

/* Random 16-byte patterns with constant-colour blocks (UNORM16 and FP16) and reserved-mode blocks among them; only_reserved:
 * reserved-mode blocks only. */
inline void random_blocks(std::vector<uint8_t>& blocks, size_t nblocks, int only_reserved = 0)
{
	blocks.resize(nblocks * 16);
	for (size_t b = 0; b < nblocks; b++)
	{
		uint8_t* p = blocks.data() + b * 16;
		for (int i = 0; i < 16; i++) p[i] = (uint8_t)rnd();
		const uint32_t kind = only_reserved ? 3u : rnd() % 16u;
		if (kind < 3)
		{
			// constant colour without an extent: 0x1FC, the FP16 flag, the reserved bits and the extent all ones
			p[0] = 0xFC; p[1] = kind == 2 ? 0xFF : 0xFD;
			for (int i = 2; i < 8; i++) p[i] = 0xFF;
			if (kind == 2) for (int i = 0; i < 4; i++) { const uint16_t h = (uint16_t)(rnd() % 0x7C00u); memcpy(p + 8 + 2 * i, &h, 2); }
		}
		else if (kind == 3) memset(p, 0, 16);       // a reserved block mode: an error block
	}
}

/* The whole image, as the decoder writes it. */
inline void decode_whole(DecodeImage& img, const std::vector<uint8_t>& blocks, std::vector<uint8_t>& whole, DecodeBatch& batch)
{
	const size_t tb = img.data_type == 0 ? 4 : img.data_type == 1 ? 8 : 16;
	whole.assign((size_t)img.dim_x * img.dim_y * img.dim_z * tb, 0x5A);
	img.data = whole.data();
	for (uint32_t z = 0; z < img.blocks_z; z++)
		for (uint32_t y = 0; y < img.blocks_y; y++)
			for (uint32_t x0 = 0; x0 < img.blocks_x; x0 += DECODE_BATCH)
				decode_row_batch(img, blocks.data(), x0, y, z, i_min(DECODE_BATCH, (int)(img.blocks_x - x0)), batch);
	img.data = nullptr;
}

/* A file of binary32 values into v (its size says how many), and bytes out to a file. */
inline bool read_floats(const char* path, std::vector<float>& v)
{
	FILE* fp = fopen(path, "rb");
	if (!fp) return false;
	const bool ok = fread(v.data(), sizeof(float), v.size(), fp) == v.size();
	fclose(fp);
	return ok;
}

inline bool write_bytes(const std::string& path, const std::vector<uint8_t>& v)
{
	FILE* fp = fopen(path.c_str(), "wb");
	if (!fp) return false;
	const bool ok = fwrite(v.data(), 1, v.size(), fp) == v.size();
	return fclose(fp) == 0 && ok;
}
