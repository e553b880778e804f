// SPDX-License-Identifier: Apache-2.0
// The filter of mip chain generation (astcenc_amd_generate_mip_chain_device, include/astcenc_amd.h): the taps of a destination
// texel along one axis, the per-texel arithmetic of every data type, and the chain's level dimensions.  Everything here is
// exactly reproducible -- integer arithmetic for linear U8, float64 in a fixed order for sRGB and float data, explicit
// round-to-nearest-even conversions -- so that the numpy models (tests/mip_model.py, tests/mip_model_3d.py) match it bit for
// bit.  The arithmetic is written once, over three axes (mip_texel_u8_3d, mip_texel_float_3d): a volume's z axis
// (astcenc_amd_generate_mip_chain_volume_device) has the taps of x and y.  A 2D texel (mip_texel_u8, mip_texel_float) is a
// texel of depth 1, whose z taps mip_axis_taps(1, 0) -- one tap of weight 1 over a denominator of 1 -- make every step of the
// z axis exact, so that the result is the 2D arithmetic of include/astcenc_amd.h.
//
// No includes and no HIP types: kernel_mips.hip builds its kernels on these functions and tests/test_mip_chain_cpu.py
// compiles the header with g++.
#pragma once

#if defined(__HIPCC__)
#define ASTC_MIP_FN __host__ __device__ inline
#define ASTC_MIP_UNROLL _Pragma("unroll")
#else
#define ASTC_MIP_FN inline
#define ASTC_MIP_UNROLL
#endif

namespace astcd {

constexpr unsigned int MIP_MAX_LEVELS = 32;          // = ASTCENC_AMD_MAX_MIP_LEVELS: a 2^32 - 1 wide image has 32 levels
constexpr unsigned int MIP_LEVEL_ALIGN = 256;        // every generated level starts on this byte boundary

/* Levels of the full chain of a dim_x x dim_y image, down to 1 x 1: floor(log2(max(dim_x, dim_y))) + 1. */
ASTC_MIP_FN unsigned int mip_full_levels(unsigned int dim_x, unsigned int dim_y)
{
	unsigned int m = dim_x > dim_y ? dim_x : dim_y, n = 1;
	while (m > 1) { m >>= 1; n++; }
	return n;
}

/* ... of a dim_x x dim_y x dim_z volume (every axis halves): floor(log2(max(dim_x, dim_y, dim_z))) + 1. */
ASTC_MIP_FN unsigned int mip_full_levels_3d(unsigned int dim_x, unsigned int dim_y, unsigned int dim_z)
{
	return mip_full_levels(dim_x > dim_y ? dim_x : dim_y, dim_z);
}

/* A level's size along one axis: max(1, dim >> level). */
ASTC_MIP_FN unsigned int mip_level_dim(unsigned int dim, unsigned int level)
{
	const unsigned int d = level >= 32 ? 0u : dim >> level;
	return d ? d : 1u;
}

/* The taps of destination texel j along an axis whose source has s texels:
 *   s == 1          texel 0, weight 1, denominator 1
 *   s even          texels 2j, 2j+1, weights (1, 1), denominator 2
 *   s = 2n+1 > 1    texels 2j, 2j+1, 2j+2, weights (n-j, n, j+1), denominator 2n+1 (the exact area coverage of texel j) */
struct MipTaps {
	unsigned int first, count;
	unsigned int w[3];
	unsigned int den;
};

ASTC_MIP_FN MipTaps mip_axis_taps(unsigned int s, unsigned int j)
{
	MipTaps t;
	if (s <= 1)
	{
		t.first = 0; t.count = 1; t.w[0] = 1; t.w[1] = 0; t.w[2] = 0; t.den = 1;
	}
	else if ((s & 1u) == 0)
	{
		t.first = 2 * j; t.count = 2; t.w[0] = 1; t.w[1] = 1; t.w[2] = 0; t.den = 2;
	}
	else
	{
		const unsigned int n = s >> 1;
		t.first = 2 * j; t.count = 3; t.w[0] = n - j; t.w[1] = n; t.w[2] = j + 1; t.den = s;
	}
	return t;
}

/* The mean of integer texels: sum / den rounded to the nearest integer, ties up.  (sum <= 255 * den; den = the product of the
 * axis denominators, at most the level's texel count, so 2 * sum + den stays far below 2^64.) */
ASTC_MIP_FN unsigned int mip_round_mean(unsigned long long sum, unsigned long long den)
{
	return (unsigned int)((2ull * sum + den) / (2ull * den));
}

/* sRGB encode of a linear mean: the number of codes c in 1..255 with mean >= thr[c - 1], thr[c - 1] = EOTF((c - 0.5) / 255)
 * (an ascending table, so a binary search). */
ASTC_MIP_FN unsigned int mip_srgb_encode(double mean, const double* thr)
{
	unsigned int lo = 0, hi = 255;       // the answer lies in [lo, hi]
	while (lo < hi)
	{
		const unsigned int mid = (lo + hi + 1) >> 1;
		if (mean >= thr[mid - 1]) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

/* The sRGB tables, float64, built on the host: lin[c] = EOTF(c / 255) for c = 0..255 at out[0..255], then
 * thr[c - 1] = EOTF((c - 0.5) / 255) for c = 1..255 at out[256..510].  pow: the C library's (the header includes nothing). */
constexpr unsigned int MIP_SRGB_TABLE_DOUBLES = 256 + 255;
template <typename Pow>
inline void mip_srgb_tables_build(double* out, Pow pow)
{
	auto eotf = [&](double x) { return x <= 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4); };
	for (int c = 0; c < 256; c++) out[c] = eotf((double)c / 255.0);
	for (int c = 1; c < 256; c++) out[256 + c - 1] = eotf(((double)c - 0.5) / 255.0);
}

ASTC_MIP_FN unsigned int mip_float_bits(float f) { unsigned int u; __builtin_memcpy(&u, &f, 4); return u; }
ASTC_MIP_FN float mip_bits_float(unsigned int u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

/* IEEE binary16 <-> binary32, round to nearest even (subnormals kept; NaN stays a quiet NaN). */
ASTC_MIP_FN unsigned short mip_half_from_float(float f)
{
	const unsigned int x = mip_float_bits(f);
	const unsigned int sign = (x >> 16) & 0x8000u;
	const unsigned int ax = x & 0x7FFFFFFFu;
	if (ax > 0x7F800000u) return (unsigned short)(sign | 0x7E00u | ((ax >> 13) & 0x3FFu));
	if (ax >= 0x477FF000u) return (unsigned short)(sign | 0x7C00u);       // >= 65520: rounds to infinity
	if (ax >= 0x38800000u)                                                // a normal half (>= 2^-14)
	{
		const unsigned int m = ax - 0x38000000u;                           // exponent rebiased from 127 to 15
		return (unsigned short)(sign | ((m + 0x0FFFu + ((m >> 13) & 1u)) >> 13));
	}
	if (ax <= 0x33000000u) return (unsigned short)sign;                   // <= 2^-25: rounds to zero
	const unsigned int mant = (ax & 0x7FFFFFu) | 0x800000u;               // a subnormal half: units of 2^-24
	const unsigned int shift = 126u - (ax >> 23);                         // 14 .. 24
	unsigned int q = mant >> shift;
	const unsigned int rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
	if (rem > half || (rem == half && (q & 1u))) q++;
	return (unsigned short)(sign | q);
}

ASTC_MIP_FN float mip_float_from_half(unsigned short h)
{
	const unsigned int sign = ((unsigned int)h & 0x8000u) << 16;
	const unsigned int e = ((unsigned int)h >> 10) & 0x1Fu, m = (unsigned int)h & 0x3FFu;
	if (e == 0)
	{
		const float v = (float)m * 5.9604644775390625e-8f;                 // m * 2^-24, exact
		return sign ? -v : v;
	}
	if (e == 31) return mip_bits_float(sign | 0x7F800000u | (m << 13));
	return mip_bits_float(sign | ((e + 112u) << 23) | (m << 13));
}

/* (The tap loops run a fixed three trips with an early exit: the weights are then indexed by constants, which keeps them in
 * registers on the device.)
 *
 * One destination texel of float data (F16 / F32 sources, stored as float channels): for each z tap in increasing slice and
 * each y tap in increasing row, row = w_x0 * v0 + w_x1 * v1 (+ w_x2 * v2); per slice acc = w_y0 * row0 + w_y1 * row1 (+ ...);
 * vol = w_z0 * acc0 + w_z1 * acc1 (+ ...); all in float64 (each sum starts at its first product), then
 * vol / ((den_x * den_y) * den_z) in float64, rounded to float32.  load(x, y, z, float v[4]) reads a source texel.  With the
 * z taps of depth 1, vol = 1.0 * acc and the denominator is (den_x * den_y) * 1.0, both exact. */
template <typename Load>
ASTC_MIP_FN void mip_texel_float_3d(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, float out[4])
{
	double vol[4] = { 0.0, 0.0, 0.0, 0.0 };
	ASTC_MIP_UNROLL
	for (unsigned int kz = 0; kz < 3; kz++)
	{
		if (kz >= tz.count) break;
		double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
		ASTC_MIP_UNROLL
		for (unsigned int ky = 0; ky < 3; ky++)
		{
			if (ky >= ty.count) break;
			double row[4] = { 0.0, 0.0, 0.0, 0.0 };
			ASTC_MIP_UNROLL
			for (unsigned int kx = 0; kx < 3; kx++)
			{
				if (kx >= tx.count) break;
				float v[4];
				load(tx.first + kx, ty.first + ky, tz.first + kz, v);
				for (int c = 0; c < 4; c++)
				{
					const double p = (double)tx.w[kx] * (double)v[c];
					row[c] = kx == 0 ? p : row[c] + p;
				}
			}
			for (int c = 0; c < 4; c++)
			{
				const double q = (double)ty.w[ky] * row[c];
				acc[c] = ky == 0 ? q : acc[c] + q;
			}
		}
		for (int c = 0; c < 4; c++)
		{
			const double r = (double)tz.w[kz] * acc[c];
			vol[c] = kz == 0 ? r : vol[c] + r;
		}
	}
	const double den = ((double)tx.den * (double)ty.den) * (double)tz.den;
	for (int c = 0; c < 4; c++) out[c] = (float)(vol[c] / den);
}

/* One destination texel of RGBA8 data: load(x, y, z) reads a source texel (packed, R in the low byte).  lin == null: every
 * channel linear, weight w_x * w_y * w_z, denominator den_x * den_y * den_z (at most the source level's texel count), the exact
 * rational mean rounded to nearest, ties up.  Otherwise (sRGB): channels 0-2 are decoded through lin[256] (the sRGB EOTF of
 * c / 255), averaged as mip_texel_float_3d averages and encoded with mip_srgb_encode(thr); channel 3 is linear. */
template <typename Load>
ASTC_MIP_FN unsigned int mip_texel_u8_3d(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, const double* lin,
                                         const double* thr)
{
	unsigned long long sum[4] = { 0, 0, 0, 0 };
	double vol[3] = { 0.0, 0.0, 0.0 };
	ASTC_MIP_UNROLL
	for (unsigned int kz = 0; kz < 3; kz++)
	{
		if (kz >= tz.count) break;
		double acc[3] = { 0.0, 0.0, 0.0 };
		ASTC_MIP_UNROLL
		for (unsigned int ky = 0; ky < 3; ky++)
		{
			if (ky >= ty.count) break;
			double row[3] = { 0.0, 0.0, 0.0 };
			ASTC_MIP_UNROLL
			for (unsigned int kx = 0; kx < 3; kx++)
			{
				if (kx >= tx.count) break;
				const unsigned int p = load(tx.first + kx, ty.first + ky, tz.first + kz);
				const unsigned long long w = (unsigned long long)tx.w[kx] * ty.w[ky] * tz.w[kz];
				for (int c = 0; c < 4; c++) sum[c] += w * ((p >> (8 * c)) & 0xFFu);
				if (lin)
					for (int c = 0; c < 3; c++)
					{
						const double v = (double)tx.w[kx] * lin[(p >> (8 * c)) & 0xFFu];
						row[c] = kx == 0 ? v : row[c] + v;
					}
			}
			if (lin)
				for (int c = 0; c < 3; c++)
				{
					const double q = (double)ty.w[ky] * row[c];
					acc[c] = ky == 0 ? q : acc[c] + q;
				}
		}
		if (lin)
			for (int c = 0; c < 3; c++)
			{
				const double r = (double)tz.w[kz] * acc[c];
				vol[c] = kz == 0 ? r : vol[c] + r;
			}
	}
	const unsigned long long den = (unsigned long long)tx.den * ty.den * tz.den;
	unsigned int out = mip_round_mean(sum[3], den) << 24;
	if (lin)
	{
		const double dden = ((double)tx.den * (double)ty.den) * (double)tz.den;
		for (int c = 0; c < 3; c++) out |= mip_srgb_encode(vol[c] / dden, thr) << (8 * c);
	}
	else
		for (int c = 0; c < 3; c++) out |= mip_round_mean(sum[c], den) << (8 * c);
	return out;
}

/* A 2D texel: the texel of depth 1 (z taps mip_axis_taps(1, 0)), its source texels read by load(x, y, float v[4]) /
 * load(x, y) -> packed texel. */
template <typename Load>
ASTC_MIP_FN void mip_texel_float(const MipTaps& tx, const MipTaps& ty, Load load, float out[4])
{
	mip_texel_float_3d(tx, ty, mip_axis_taps(1, 0), [&](unsigned int x, unsigned int y, unsigned int, float v[4]) { load(x, y, v); }, out);
}

template <typename Load>
ASTC_MIP_FN unsigned int mip_texel_u8(const MipTaps& tx, const MipTaps& ty, Load load, const double* lin, const double* thr)
{
	return mip_texel_u8_3d(tx, ty, mip_axis_taps(1, 0), [&](unsigned int x, unsigned int y, unsigned int) { return load(x, y); }, lin, thr);
}

} // namespace astcd
