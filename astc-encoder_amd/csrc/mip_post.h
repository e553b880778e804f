// SPDX-License-Identifier: Apache-2.0
// The post-passes of a mip chain (astcenc_amd_generate_mip_chain_ex_device, include/astcenc_amd.h): normal-map
// renormalisation of channels 0-2 and alpha-test coverage preservation of channel 3, applied to levels 1 .. n-1 after the
// whole chain has been generated.  This header holds the per-texel arithmetic and the host-derived constants; the kernels that
// count, select and apply are in kernel_mip_post.hip.  Every float operation is float64, one IEEE operation at a time (the
// library builds with -ffp-contract=off), with a true division and a correctly rounded sqrt, so that the numpy model
// (tests/mip_options_model.py) matches it bit for bit.
//
// No includes: it is read after mip_filter.h (its half conversions and ASTC_MIP_FN), by kernel_mip_post.hip, by the host
// checks (astcenc_set.cpp) and by tests/test_mip_options_cpu.py, which compiles both headers with g++.
#pragma once

namespace astcd {

constexpr unsigned int MIP_POST_NORMALIZE = 0x1u;        // = ASTCENC_AMD_MIP_NORMALIZE
constexpr unsigned int MIP_POST_ALPHA_COVERAGE = 0x2u;   // = ASTCENC_AMD_MIP_ALPHA_COVERAGE

/* ---- NORMALIZE: channels 0-2 hold (n + 1) / 2 of a unit normal n ---- */

/* A texel's three decoded components v (double) -> the unit vector out; false (nothing to write) when len2 is 0 or not finite. */
ASTC_MIP_FN bool mip_normalize3(const double v[3], double out[3])
{
	const double len2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
	if (!(len2 > 0.0) || !(len2 < __builtin_inf())) return false;     // (also NaN)
	const double len = __builtin_sqrt(len2);
	for (int c = 0; c < 3; c++) out[c] = v[c] / len;
	return true;
}

/* RGBA8: v = (2 code - 255) / 255, code = clamp(floor((n + 1) * 127.5 + 0.5), 0, 255); channel 3 kept.  len2 is never 0:
 * 2 code - 255 is odd. */
ASTC_MIP_FN unsigned int mip_normalize_u8(unsigned int texel)
{
	double v[3], n[3];
	for (int c = 0; c < 3; c++) v[c] = (double)(2 * (int)((texel >> (8 * c)) & 0xFFu) - 255) / 255.0;
	if (!mip_normalize3(v, n)) return texel;
	unsigned int out = texel & 0xFF000000u;
	for (int c = 0; c < 3; c++)
	{
		const double q = __builtin_floor((n[c] + 1.0) * 127.5 + 0.5);
		const unsigned int code = q <= 0.0 ? 0u : q >= 255.0 ? 255u : (unsigned int)q;
		out |= code << (8 * c);
	}
	return out;
}

/* F16 / F32 channels 0-2 (as floats, in place): v = 2 x - 1, out = (float)((n + 1) * 0.5).  Returns false when the texel stays
 * as it is (its stored bits are then kept, for F16 too); an F16 texel takes mip_half_from_float of the new floats. */
ASTC_MIP_FN bool mip_normalize_float(float x[3])
{
	double v[3], n[3];
	for (int c = 0; c < 3; c++) v[c] = 2.0 * (double)x[c] - 1.0;
	if (!mip_normalize3(v, n)) return false;
	for (int c = 0; c < 3; c++) x[c] = (float)((n[c] + 1.0) * 0.5);
	return true;
}

/* ---- ALPHA_COVERAGE: keep level 0's share of texels that pass the alpha test ---- */

/* RGBA8: a code is covered when code >= t, t = the smallest integer in 1..255 with (double)t >= (double)cutoff * 255. */
ASTC_MIP_FN unsigned int mip_cover_u8_threshold(float cutoff)
{
	const double c = (double)cutoff * 255.0;
	unsigned int t = 1;
	while (t < 255 && (double)t < c) t++;
	return t;
}

/* F16 / F32: hi / lo = the smallest / largest value of the output type that is >= / < cutoff (cutoff in (0, 1]). */
ASTC_MIP_FN void mip_cover_bounds(float cutoff, bool half, float& hi, float& lo)
{
	if (!half)
	{
		hi = cutoff;
		lo = mip_bits_float(mip_float_bits(cutoff) - 1u);                  // (positive: one step toward zero)
		return;
	}
	unsigned short h = mip_half_from_float(cutoff);
	if (mip_float_from_half(h) < cutoff) h++;
	hi = mip_float_from_half(h);
	lo = mip_float_from_half((unsigned short)(h - 1u));
}

/* Is an alpha covered: U8 code >= t; float (double)a >= (double)cutoff (NaN never). */
ASTC_MIP_FN bool mip_covered_u8(unsigned int code, unsigned int t) { return code >= t; }
ASTC_MIP_FN bool mip_covered_float(float a, float cutoff) { return (double)a >= (double)cutoff; }

/* The target count of a surface of n texels whose level-0 surface of n0 texels has c0 covered: floor((2 c0 n + n0) / (2 n0)),
 * exactly (the product needs 128 bits; the quotient is at most n). */
ASTC_MIP_FN unsigned long long mip_cover_target(unsigned long long c0, unsigned long long n, unsigned long long n0)
{
	const unsigned __int128 num = (unsigned __int128)c0 * n * 2u + n0;
	const unsigned long long den = 2ull * n0;                           // (n0 < 2^62: the chain's bytes fit size_t)
	unsigned long long rem = 0, q = 0;
	for (int i = 127; i >= 0; i--)
	{
		rem = (rem << 1) | (unsigned long long)((num >> i) & 1u);
		if (rem >= den)
		{
			rem -= den;
			q |= 1ull << (i & 63);                                         // (only i < 64 can set a bit: q <= n)
		}
	}
	return q;
}

/* The order-preserving keys the k-th largest alpha is selected by (radix digits from the top, 8 bits each): U8 the code,
 * F16 / F32 the bit pattern mapped so that unsigned order is numeric order, every NaN mapped to 0, below everything. */
ASTC_MIP_FN unsigned int mip_key_f32(float a)
{
	const unsigned int u = mip_float_bits(a);
	if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ASTC_MIP_FN float mip_key_f32_value(unsigned int k) { return mip_bits_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
ASTC_MIP_FN unsigned int mip_key_f16(unsigned short h)
{
	const unsigned int u = h;
	if ((u & 0x7FFFu) > 0x7C00u) return 0u;
	return (u & 0x8000u) ? (~u & 0xFFFFu) : (u | 0x8000u);
}
ASTC_MIP_FN float mip_key_f16_value(unsigned int k)
{
	return mip_float_from_half((unsigned short)((k & 0x8000u) ? (k & 0x7FFFu) : (~k & 0xFFFFu)));
}

/* U8 remap with the threshold alpha ak (> 0): q = floor((2 a t + ak) / (2 ak)); a >= ak: min(255, q), else min(t - 1, q). */
ASTC_MIP_FN unsigned int mip_cover_remap_u8(unsigned int a, unsigned int ak, unsigned int t)
{
	const unsigned int q = (2u * a * t + ak) / (2u * ak);
	const unsigned int cap = a >= ak ? 255u : t - 1u;
	return q < cap ? q : cap;
}

/* Float remap with the threshold alpha ak (finite, > 0): r = (a * cutoff) / ak in float64, rounded to float32 (then to half
 * for F16: `half`); a >= ak: max(hi, min(r, 1)), else min(r, lo).  A NaN alpha is returned unchanged.  The result is a float
 * that the output type holds exactly. */
ASTC_MIP_FN float mip_cover_remap_float(float a, float ak, float cutoff, float hi, float lo, bool half)
{
	if (a != a) return a;
	float r = (float)(((double)a * (double)cutoff) / (double)ak);
	if (half) r = mip_float_from_half(mip_half_from_float(r));
	if ((double)a >= (double)ak)
	{
		r = r < 1.0f ? r : 1.0f;
		return r > hi ? r : hi;
	}
	return r < lo ? r : lo;
}

} // namespace astcd
