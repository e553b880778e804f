// SPDX-License-Identifier: Apache-2.0
// Resizing to any size with the mip filters (astcenc_amd_resize_image_device, include/astcenc_amd.h): the taps of a destination
// texel along an axis whose s source texels make d, for the box (exact area coverage, integers) and the windowed filters (the
// function, normalisation and edges of mip_resample.h with the centre and the scale of a general ratio), the sums of one
// destination texel, and the integer arithmetic of astcenc_amd_resize_dims.  At d = max(1, s >> 1) the taps are those of
// mip_axis_taps / mip_resample_taps, every weight equal, and the sums and results are the chain's own: the float64 row / acc /
// vol order of mip_resample.h, exact integers where the box filter of mip_filter.h has them, the alpha weighting of
// mip_weighted.h.  tests/resize_model.py reproduces all of it bit for bit.
//
// Nothing but the sibling headers and no HIP types: kernel_resize.hip builds its kernels on these functions and
// tests/test_resize_cpu.py compiles the header with g++.
#pragma once

#include "mip_weighted.h"

namespace astcd {

ASTC_MIP_FN unsigned int mip_resize_gcd(unsigned int a, unsigned int b)
{
	while (b) { const unsigned int t = a % b; a = b; b = t; }
	return a;
}

/* An axis copies (one tap of weight 1.0 on texel 0 or on texel j) when its source has one texel or its size stays. */
ASTC_MIP_FN bool mip_resize_passes(unsigned int s, unsigned int d) { return s <= 1 || d == s; }

/* The box taps of destination texel j: with g = gcd(s, d), s' = s / g and d' = d / g, destination j covers [j s', (j + 1) s')
 * and source i covers [i d', (i + 1) d'); the taps are the sources with a non-empty overlap, in increasing i, the weight is the
 * overlap's length and the denominator is s'.  Returns the count and the first source; weight(k) gives tap k's. */
struct MipResizeBox {
	unsigned long long lo, hi;        // the destination's interval
	unsigned long long first;
	unsigned int count, dp, den;
};

ASTC_MIP_FN MipResizeBox mip_resize_box(unsigned int s, unsigned int d, unsigned int j)
{
	const unsigned int g = mip_resize_gcd(s, d);
	MipResizeBox b;
	b.den = s / g; b.dp = d / g;
	b.lo = (unsigned long long)j * b.den; b.hi = b.lo + b.den;
	b.first = b.lo / b.dp;
	b.count = (unsigned int)((b.hi - 1ull) / b.dp - b.first) + 1u;
	return b;
}

ASTC_MIP_FN unsigned int mip_resize_box_weight(const MipResizeBox& b, unsigned int k)
{
	const unsigned long long a = (b.first + k) * b.dp, e = a + b.dp;
	return (unsigned int)((e < b.hi ? e : b.hi) - (a > b.lo ? a : b.lo));
}

/* The windowed taps of destination texel j: r = (double)s / (double)d, scale = r when d < s and 1.0 otherwise (no widening when
 * enlarging), c = (double)((2j + 1) * s) / (double)(2d) (the product in 64-bit integers); the taps are every integer i with
 * |t| < S, t = (((double)i + 0.5) - c) / scale.  t does not decrease with i, so they are one run of integers: its first index
 * goes to *first and its length is returned.  (The tap next to c has |t| <= 0.5, so there is always one.) */
ASTC_MIP_FN double mip_resize_t(long long i, double c, double scale)
{
	const double t = (((double)i + 0.5) - c) / scale;
	return t < 0.0 ? -t : t;
}

ASTC_MIP_FN unsigned long long mip_resize_range(int kind, unsigned int s, unsigned int d, unsigned int j, long long* first)
{
	const double r = (double)s / (double)d;
	const double scale = d < s ? r : 1.0;
	const double c = (double)((2ull * j + 1ull) * (unsigned long long)s) / (double)(2ull * d);
	const double S = (double)mip_resample_support(kind);
	long long lo = (long long)__builtin_floor(c - S * scale) - 2, hi = (long long)__builtin_floor(c + S * scale) + 2;
	while (!(mip_resize_t(lo, c, scale) < S)) lo++;
	while (!(mip_resize_t(hi, c, scale) < S)) hi--;
	*first = lo;
	return (unsigned long long)(hi - lo) + 1ull;
}

/* ... and their weights, w[0 .. count): f(|t|) / sum, sum = f_first + f_first+1 + ... in increasing i (mip_resample_eval). */
template <typename Sin>
inline void mip_resize_weights(int kind, unsigned int s, unsigned int d, unsigned int j, Sin sin, long long first, unsigned long long count, double* w)
{
	const double r = (double)s / (double)d;
	const double scale = d < s ? r : 1.0;
	const double c = (double)((2ull * j + 1ull) * (unsigned long long)s) / (double)(2ull * d);
	double sum = 0.0;
	for (unsigned long long k = 0; k < count; k++)
	{
		const double f = mip_resample_eval(kind, mip_resize_t(first + (long long)k, c, scale), sin);
		w[k] = f;
		sum = k == 0 ? f : sum + f;
	}
	for (unsigned long long k = 0; k < count; k++) w[k] = w[k] / sum;
}

/* The taps of destination texel j for any filter: the count and *first; *den the axis denominator (1 unless the box). */
ASTC_MIP_FN unsigned long long mip_resize_tap_count(int kind, unsigned int s, unsigned int d, unsigned int j, long long* first, unsigned int* den)
{
	*den = 1;
	if (mip_resize_passes(s, d))
	{
		*first = s <= 1 ? 0 : (long long)j;
		return 1;
	}
	if (kind == MIP_FILTER_BOX)
	{
		const MipResizeBox b = mip_resize_box(s, d, j);
		*first = (long long)b.first; *den = b.den;
		return b.count;
	}
	return mip_resize_range(kind, s, d, j, first);
}

/* ... and the weights as float64 (the box's integers are exact in it), w[0 .. count). */
template <typename Sin>
inline void mip_resize_tap_weights(int kind, unsigned int s, unsigned int d, unsigned int j, Sin sin, long long first, unsigned long long count, double* w)
{
	if (mip_resize_passes(s, d)) w[0] = 1.0;
	else if (kind == MIP_FILTER_BOX)
	{
		const MipResizeBox b = mip_resize_box(s, d, j);
		for (unsigned int k = 0; k < b.count; k++) w[k] = (double)mip_resize_box_weight(b, k);
	}
	else mip_resize_weights(kind, s, d, j, sin, first, count, w);
}

/* The rows of an axis repeat with a period where the arithmetic above is exact: destination j then has the taps of
 * j mod period moved by (j / period) * shift.  The box: period d / g, shift s / g (integers).  A windowed kind: the centres
 * must be exact in float64, which they are for an integer ratio s / d (period 1, shift s / d: c = (2j + 1) (s / d) / 2) and
 * for an enlargement by a power of two (period d / s, shift 1: c = (2j + 1) / (2 d / s)), while (2j + 1) s stays below 2^53.
 * Anything else: period d, shift 0. */
ASTC_MIP_FN void mip_resize_period(int kind, unsigned int s, unsigned int d, unsigned int* period, unsigned int* shift)
{
	*period = d; *shift = 0;
	if (s <= 1) { *period = 1; return; }
	if (d == s) { *period = 1; *shift = 1; return; }
	if (kind == MIP_FILTER_BOX)
	{
		const unsigned int g = mip_resize_gcd(s, d);
		*period = d / g; *shift = s / g;
		return;
	}
	if (2ull * d * (unsigned long long)s > (1ull << 53)) return;
	if (s % d == 0) { *period = 1; *shift = s / d; }
	else if (d % s == 0 && ((d / s) & (d / s - 1u)) == 0) { *period = d / s; *shift = 1; }
}

/* The values of a texel and the sums.  A texel has N = 4 values (the channels) or, with WEIGHT_ALPHA, 7 (then the channels
 * times alpha, mip_weighted.h), each one 64-bit slot.  The slots named by the bits of INTS hold exact unsigned integers, the
 * others float64: the box filter keeps every channel of linear U8 data and the alpha channel of sRGB data in integers
 * (mip_filter.h), everything else is float64 (mip_resize_ints). */
union MipResizeSlot {
	double f;
	unsigned long long u;
};

enum MipResizeType { MIP_RESIZE_U8 = 0, MIP_RESIZE_U8_SRGB = 1, MIP_RESIZE_FLOAT = 2 };

ASTC_MIP_FN constexpr unsigned int mip_resize_ints(int type, bool box, bool weighted)
{
	return !box || type == MIP_RESIZE_FLOAT ? 0u : type == MIP_RESIZE_U8_SRGB ? 0x08u : weighted ? 0x7Fu : 0x0Fu;
}

template <int N, unsigned int INTS>
ASTC_MIP_FN void mip_resize_load_u8(unsigned int p, const double* lin, MipResizeSlot v[N])
{
	const unsigned int a = p >> 24;
	for (int c = 0; c < 4; c++)
	{
		const unsigned int code = (p >> (8 * c)) & 0xFFu;
		if (INTS >> c & 1u) v[c].u = code;
		else v[c].f = lin && c < 3 ? lin[code] : (double)code;
	}
	for (int c = 4; c < N; c++)
	{
		const unsigned int code = (p >> (8 * (c - 4))) & 0xFFu;
		if (INTS >> c & 1u) v[c].u = a * code;
		else v[c].f = lin ? (double)a * lin[code] : (double)(a * code);
	}
}

template <int N>
ASTC_MIP_FN void mip_resize_load_float(const float f[4], MipResizeSlot v[N])
{
	for (int c = 0; c < 4; c++) v[c].f = (double)f[c];
	for (int c = 4; c < N; c++) v[c].f = v[3].f * v[c - 4].f;
}

/* One step of a sum (mip_resample_accumulate): sum = w * v at tap 0 of the sum, else sum + w * v; an integer slot takes the
 * weight as the integer it is. */
template <int N, unsigned int INTS>
ASTC_MIP_FN void mip_resize_accumulate(MipResizeSlot sum[N], double w, const MipResizeSlot v[N], bool first)
{
	for (int c = 0; c < N; c++)
	{
		if (INTS >> c & 1u)
		{
			const unsigned long long p = (unsigned long long)w * v[c].u;
			sum[c].u = first ? p : sum[c].u + p;
		}
		else
		{
			const double p = w * v[c].f;
			sum[c].f = first ? p : sum[c].f + p;
		}
	}
}

/* sum / den rounded to nearest, ties up: mip_round_mean without its doubled numerator, (2 sum + den) / (2 den) =
 * sum / den + (2 (sum mod den) >= den), so that sums up to 2^63 hold. */
ASTC_MIP_FN unsigned int mip_resize_round_mean(unsigned long long sum, unsigned long long den)
{
	const unsigned long long q = sum / den, r = sum - q * den;
	return (unsigned int)(q + (r >= den - r ? 1u : 0u));
}

/* The stored results of vol.  den = den_x * den_y * den_z and dden = ((double)den_x * (double)den_y) * (double)den_z (both 1
 * for a windowed kind). */
template <int N, bool BOX>
ASTC_MIP_FN unsigned int mip_resize_out_u8(const MipResizeSlot vol[N], const double* thr, unsigned long long den, double dden)
{
	if (!BOX)
	{
		double v[N];
		for (int c = 0; c < N; c++) v[c] = vol[c].f;
		if (N == 7) return mip_resample_out_u8_weighted(v, thr);
		return mip_resample_out_u8(v, thr);
	}
	unsigned int out = mip_resize_round_mean(vol[3].u, den) << 24;
	const unsigned long long sa = vol[3].u;
	for (int c = 0; c < 3; c++)
	{
		unsigned int code;
		if (thr) code = mip_srgb_encode(N == 7 && sa > 0 ? vol[N == 7 ? 4 + c : c].f / (double)sa : vol[c].f / dden, thr);
		else if (N == 7 && sa > 0) code = mip_resize_round_mean(vol[N == 7 ? 4 + c : c].u, sa);
		else code = mip_resize_round_mean(vol[c].u, den);
		out |= code << (8 * c);
	}
	return out;
}

template <int N, bool BOX>
ASTC_MIP_FN void mip_resize_out_float(const MipResizeSlot vol[N], double dden, float out[4])
{
	for (int c = 0; c < 4; c++) out[c] = (float)(BOX ? vol[c].f / dden : vol[c].f);
	if (N == 7 && vol[3].f > 0.0)
		for (int c = 0; c < 3; c++) out[c] = (float)(vol[N == 7 ? 4 + c : c].f / vol[3].f);
}

/* One destination texel, the reference form (mip_resample_texel): for each z tap and each y tap in increasing order
 * row = sum_x w_x v, per slice acc = sum_y w_y row, then vol = sum_z w_z acc.  load(x, y, z, MipResizeSlot v[N]) gives a source
 * texel's values, the indices already mapped by mip_resample_source (the box and a copied axis never leave the source). */
template <int N, unsigned int INTS, typename Load>
inline void mip_resize_texel(const MipResampleTaps& tx, const MipResampleTaps& ty, const MipResampleTaps& tz, Load load, MipResizeSlot vol[N])
{
	for (unsigned int kz = 0; kz < tz.count; kz++)
	{
		const unsigned int z = mip_resample_source(tz.first + kz, tz.s, tz.edge);
		MipResizeSlot acc[N];
		for (unsigned int ky = 0; ky < ty.count; ky++)
		{
			const unsigned int y = mip_resample_source(ty.first + ky, ty.s, ty.edge);
			MipResizeSlot row[N];
			for (unsigned int kx = 0; kx < tx.count; kx++)
			{
				MipResizeSlot v[N];
				load(mip_resample_source(tx.first + kx, tx.s, tx.edge), y, z, v);
				mip_resize_accumulate<N, INTS>(row, tx.w[kx], v, kx == 0);
			}
			mip_resize_accumulate<N, INTS>(acc, ty.w[ky], row, ky == 0);
		}
		mip_resize_accumulate<N, INTS>(vol, tz.w[kz], acc, kz == 0);
	}
}

/* astcenc_amd_resize_dims (include/astcenc_amd.h), integers only.  pow2: 0 none, 1 nearest, 2 next, 3 previous.  false: a zero
 * dimension, an unknown mode or a result above 2^31. */
ASTC_MIP_FN unsigned long long mip_resize_pow2(unsigned long long v, unsigned int pow2)
{
	unsigned long long prev = 1;
	while (prev * 2ull <= v) prev *= 2ull;
	if (pow2 == 3 || prev == v) return prev;
	if (pow2 == 2) return prev * 2ull;
	return v - prev < 2ull * prev - v ? prev : prev * 2ull;
}

ASTC_MIP_FN bool mip_resize_dims(unsigned int x, unsigned int y, unsigned int max_dim, unsigned int pow2, unsigned int* out_x, unsigned int* out_y)
{
	if (x == 0 || y == 0 || pow2 > 3) return false;
	unsigned long long v[2] = { x, y };
	const unsigned long long L = x > y ? x : y;
	if (max_dim != 0 && L > max_dim)
		for (int a = 0; a < 2; a++)
		{
			if (v[a] == L) v[a] = max_dim;
			else
			{
				v[a] = (v[a] * max_dim + L / 2ull) / L;
				if (v[a] == 0) v[a] = 1;
			}
		}
	if (pow2 != 0)
		for (int a = 0; a < 2; a++)
		{
			const unsigned long long p = mip_resize_pow2(v[a], pow2);
			v[a] = max_dim != 0 && p > max_dim ? mip_resize_pow2(v[a], 3) : p;
		}
	if (v[0] > (1ull << 31) || v[1] > (1ull << 31)) return false;
	*out_x = (unsigned int)v[0]; *out_y = (unsigned int)v[1];
	return true;
}

} // namespace astcd
