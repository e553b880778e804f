// SPDX-License-Identifier: Apache-2.0
// Alpha-weighted colour filtering of mip chain generation (astcenc_amd_generate_mip_chain_weighted_device with
// ASTCENC_AMD_MIP_WEIGHT_ALPHA, include/astcenc_amd.h): channels 0-2 of a destination texel are the mean of the source colours
// weighted by tap weight x alpha, so that the colour under transparent texels does not bleed into visible ones.  Channel 3 is
// the plain filter's, bit for bit, and a footprint without any positive alpha weight keeps the plain filter's colour too.
//
// "Plain" is the arithmetic of mip_filter.h (box) and mip_resample.h (windowed) for the same filter, kind and type; the sums
// here are the same taps in the same order, each sum starting at its first product, one rounded IEEE operation at a time.
// tests/mip_weighted_model.py reproduces all of it bit for bit.
//
// No HIP types and nothing but the two sibling headers: kernel_mip_weighted.hip and kernel_mip_filter.hip build their kernels
// on these functions and tests/test_mip_weighted_cpu.py compiles the header with g++.
#pragma once

#include "mip_resample.h"

namespace astcd {

// = enum astcenc_amd_mip_weight
enum MipWeight { MIP_WEIGHT_NONE = 0, MIP_WEIGHT_ALPHA = 1 };

/* The box filter's float64 sums of N values per source texel (the row / acc / vol order of mip_texel_float_3d, no division):
 * values(x, y, z, double v[N]) gives a source texel's values. */
template <int N, typename Values>
ASTC_MIP_FN void mip_box_sums(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Values values, double vol[N])
{
	for (int c = 0; c < N; c++) vol[c] = 0.0;
	ASTC_MIP_UNROLL
	for (unsigned int kz = 0; kz < 3; kz++)
	{
		if (kz >= tz.count) break;
		double acc[N];
		for (int c = 0; c < N; c++) acc[c] = 0.0;
		ASTC_MIP_UNROLL
		for (unsigned int ky = 0; ky < 3; ky++)
		{
			if (ky >= ty.count) break;
			double row[N];
			for (int c = 0; c < N; c++) row[c] = 0.0;
			ASTC_MIP_UNROLL
			for (unsigned int kx = 0; kx < 3; kx++)
			{
				if (kx >= tx.count) break;
				double v[N];
				values(tx.first + kx, ty.first + ky, tz.first + kz, v);
				for (int c = 0; c < N; c++)
				{
					const double p = (double)tx.w[kx] * v[c];
					row[c] = kx == 0 ? p : row[c] + p;
				}
			}
			for (int c = 0; c < N; c++)
			{
				const double q = (double)ty.w[ky] * row[c];
				acc[c] = ky == 0 ? q : acc[c] + q;
			}
		}
		for (int c = 0; c < N; c++)
		{
			const double r = (double)tz.w[kz] * acc[c];
			vol[c] = kz == 0 ? r : vol[c] + r;
		}
	}
}

/* One destination texel of float data, box filter.  Values of a source texel (c0, c1, c2, a): the four channels as float64 and
 * (double)a * (double)c (exact in float64); vol[0..3] are the plain sums, volA = vol[3], volP_c = vol[4 + c].  Channel 3 and,
 * unless volA > 0.0 (a zero, a negative or a NaN volA), channels 0-2 are the plain filter's (float)(vol[c] / den); otherwise
 * channel c is (float)(volP_c / volA).  Nothing else is special: infinities and negative alphas follow IEEE. */
template <typename Load>
ASTC_MIP_FN void mip_texel_float_3d_weighted(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, float out[4])
{
	double vol[7];
	mip_box_sums<7>(tx, ty, tz, [&](unsigned int x, unsigned int y, unsigned int z, double v[7]) {
		float f[4];
		load(x, y, z, f);
		for (int c = 0; c < 4; c++) v[c] = (double)f[c];
		for (int c = 0; c < 3; c++) v[4 + c] = v[3] * v[c];
	}, vol);
	const double den = ((double)tx.den * (double)ty.den) * (double)tz.den;
	for (int c = 0; c < 4; c++) out[c] = (float)(vol[c] / den);
	if (vol[3] > 0.0)
		for (int c = 0; c < 3; c++) out[c] = (float)(vol[4 + c] / vol[3]);
}

/* One destination texel of RGBA8 data, box filter.  W = w_x * w_y * w_z per tap, SA = sum W a and SP_c = sum W a c, exact
 * integers.  Channel 3 is the plain filter's; with SA == 0 so are channels 0-2.  With SA > 0:
 *   linear (lin == null): (2 SP_c + SA) / (2 SA) floored, the exact weighted mean rounded to nearest, ties up (at most 255);
 *   sRGB: the value of a tap is (double)a * lin[c], volP_c the plain float64 sums of it, and the code is
 *   mip_srgb_encode(volP_c / (double)SA).
 * (2 SP_c + SA <= 130305 den, below 2^17 den, den = the product of the axis denominators: 64-bit integers hold while
 * den < 2^47, and a level of that many texels cannot exist in device memory.) */
template <typename Load>
ASTC_MIP_FN unsigned int mip_texel_u8_3d_weighted(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, const double* lin,
                                                  const double* thr)
{
	unsigned long long sum[4] = { 0, 0, 0, 0 }, sa = 0, sp[3] = { 0, 0, 0 };
	ASTC_MIP_UNROLL
	for (unsigned int kz = 0; kz < 3; kz++)
	{
		if (kz >= tz.count) break;
		ASTC_MIP_UNROLL
		for (unsigned int ky = 0; ky < 3; ky++)
		{
			if (ky >= ty.count) break;
			ASTC_MIP_UNROLL
			for (unsigned int kx = 0; kx < 3; kx++)
			{
				if (kx >= tx.count) break;
				const unsigned int p = load(tx.first + kx, ty.first + ky, tz.first + kz);
				const unsigned long long w = (unsigned long long)tx.w[kx] * ty.w[ky] * tz.w[kz];
				for (int c = 0; c < 4; c++) sum[c] += w * ((p >> (8 * c)) & 0xFFu);
				const unsigned long long wa = w * (p >> 24);
				sa += wa;
				for (int c = 0; c < 3; c++) sp[c] += wa * ((p >> (8 * c)) & 0xFFu);
			}
		}
	}
	const unsigned long long den = (unsigned long long)tx.den * ty.den * tz.den;
	unsigned int out = mip_round_mean(sum[3], den) << 24;
	if (lin)
	{
		// vol[0..2]: the plain sums of lin[c]; vol[3..5]: those of (double)a * lin[c]
		double vol[6];
		mip_box_sums<6>(tx, ty, tz, [&](unsigned int x, unsigned int y, unsigned int z, double v[6]) {
			const unsigned int p = load(x, y, z);
			const double a = (double)(p >> 24);
			for (int c = 0; c < 3; c++)
			{
				v[c] = lin[(p >> (8 * c)) & 0xFFu];
				v[3 + c] = a * v[c];
			}
		}, vol);
		const double dden = ((double)tx.den * (double)ty.den) * (double)tz.den;
		for (int c = 0; c < 3; c++)
			out |= mip_srgb_encode(sa > 0 ? vol[3 + c] / (double)sa : vol[c] / dden, thr) << (8 * c);
	}
	else
		for (int c = 0; c < 3; c++)
			out |= (sa > 0 ? (unsigned int)((2ull * sp[c] + sa) / (2ull * sa)) : mip_round_mean(sum[c], den)) << (8 * c);
	return out;
}

/* A 2D texel: the texel of depth 1. */
template <typename Load>
ASTC_MIP_FN void mip_texel_float_weighted(const MipTaps& tx, const MipTaps& ty, Load load, float out[4])
{
	mip_texel_float_3d_weighted(tx, ty, mip_axis_taps(1, 0), [&](unsigned int x, unsigned int y, unsigned int, float v[4]) { load(x, y, v); }, out);
}

template <typename Load>
ASTC_MIP_FN unsigned int mip_texel_u8_weighted(const MipTaps& tx, const MipTaps& ty, Load load, const double* lin, const double* thr)
{
	return mip_texel_u8_3d_weighted(tx, ty, mip_axis_taps(1, 0), [&](unsigned int x, unsigned int y, unsigned int) { return load(x, y); }, lin, thr);
}

/* The windowed filters (mip_resample.h).  A source texel has seven float64 values: v[0..3] the plain ones
 * (mip_resample_load_*), v[4 + c] the alpha-weighted colour: (double)(a * c) for linear U8 (the integer product),
 * (double)a * lin[c] for sRGB, (double)a * (double)c for floats.  The seven separable sums run as the plain four do
 * (mip_resample_accumulate7); volA = vol[3], volP_c = vol[4 + c]. */
constexpr int MIP_WEIGHTED_VALUES = 7;

ASTC_MIP_FN void mip_resample_load_u8_weighted(unsigned int p, const double* lin, double v[7])
{
	mip_resample_load_u8(p, lin, v);
	const unsigned int a = p >> 24;
	for (int c = 0; c < 3; c++)
		v[4 + c] = lin ? (double)a * v[c] : (double)(a * ((p >> (8 * c)) & 0xFFu));
}

ASTC_MIP_FN void mip_resample_load_float_weighted(const float f[4], double v[7])
{
	mip_resample_load_float(f, v);
	for (int c = 0; c < 3; c++) v[4 + c] = v[3] * v[c];
}

ASTC_MIP_FN void mip_resample_accumulate7(double sum[7], double w, const double v[7], unsigned int k)
{
	for (int c = 0; c < 7; c++)
	{
		const double p = w * v[c];
		sum[c] = k == 0 ? p : sum[c] + p;
	}
}

/* The stored results: the plain ones of vol[0..3]; where volA > 0.0, channels 0-2 from m = volP_c / volA instead: linear U8
 * clamp(floor(m + 0.5), 0, 255), clamped in float64 before the conversion (a tiny volA from negative lobes can make m huge);
 * sRGB mip_srgb_encode(m); floats (float)m. */
ASTC_MIP_FN unsigned int mip_resample_out_u8_weighted(const double vol[7], const double* thr)
{
	unsigned int out = mip_resample_out_u8(vol, thr);
	if (vol[3] > 0.0)
	{
		out &= 0xFF000000u;
		for (int c = 0; c < 3; c++)
		{
			const double m = vol[4 + c] / vol[3];
			unsigned int code;
			if (thr)
				code = mip_srgb_encode(m, thr);
			else
			{
				const double q = __builtin_floor(m + 0.5);
				code = q < 0.0 ? 0u : q > 255.0 ? 255u : (unsigned int)q;
			}
			out |= code << (8 * c);
		}
	}
	return out;
}

ASTC_MIP_FN void mip_resample_out_float_weighted(const double vol[7], float out[4])
{
	mip_resample_out_float(vol, out);
	if (vol[3] > 0.0)
		for (int c = 0; c < 3; c++) out[c] = (float)(vol[4 + c] / vol[3]);
}

/* One destination texel, the reference form (mip_resample_texel with seven values): load(x, y, z, double v[7]). */
template <typename Load>
inline void mip_resample_texel_weighted(const MipResampleTaps& tx, const MipResampleTaps& ty, const MipResampleTaps& tz, Load load, double vol[7])
{
	for (unsigned int kz = 0; kz < tz.count; kz++)
	{
		const unsigned int z = mip_resample_source(tz.first + kz, tz.s, tz.edge);
		double acc[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
		for (unsigned int ky = 0; ky < ty.count; ky++)
		{
			const unsigned int y = mip_resample_source(ty.first + ky, ty.s, ty.edge);
			double row[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
			for (unsigned int kx = 0; kx < tx.count; kx++)
			{
				double v[7];
				load(mip_resample_source(tx.first + kx, tx.s, tx.edge), y, z, v);
				mip_resample_accumulate7(row, tx.w[kx], v, kx);
			}
			mip_resample_accumulate7(acc, ty.w[ky], row, ky);
		}
		mip_resample_accumulate7(vol, tz.w[kz], acc, kz);
	}
}

/* ... and of a cube face with MIP_EDGE_CUBE (mip_resample_texel_cube with seven values): load(face, x, y, double v[7]). */
template <typename Load>
inline void mip_resample_texel_cube_weighted(unsigned int face, const MipResampleTaps& tx, const MipResampleTaps& ty, Load load, double vol[7])
{
	double acc[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
	for (unsigned int ky = 0; ky < ty.count; ky++)
	{
		double row[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
		for (unsigned int kx = 0; kx < tx.count; kx++)
		{
			const MipCubeTexel t = mip_cube_source(face, tx.first + kx, ty.first + ky, tx.s);
			double v[7];
			load(t.face, t.x, t.y, v);
			mip_resample_accumulate7(row, tx.w[kx], v, kx);
		}
		mip_resample_accumulate7(acc, ty.w[ky], row, ky);
	}
	mip_resample_accumulate7(vol, 1.0, acc, 0);
}

} // namespace astcd
