// SPDX-License-Identifier: Apache-2.0
// The windowed filters of mip chain generation (astcenc_amd_generate_mip_chain_filtered_device, include/astcenc_amd.h):
// MITCHELL, LANCZOS3 and KAISER.  The taps of a destination texel along one axis and their weights are computed on the host,
// once per call, by mip_resample_taps (IEEE + - * /, sqrt and the C library's sin, which the caller passes in: the header
// includes nothing); the device only multiplies and adds them in float64, in the order of mip_resample_accumulate, and rounds
// with mip_resample_out_*.  tests/mip_filter_model.py reproduces all of it bit for bit with Python floats (math.sin is the same
// C library function).
//
// No includes and no HIP types: kernel_mip_filter.hip and kernel_mip_cube.hip build their kernels on these functions and
// tests/test_mip_filter_cpu.py and tests/test_mip_cube_cpu.py compile the header with g++.
#pragma once

#include "mip_filter.h"

namespace astcd {

// = enum astcenc_amd_mip_filter_kind / astcenc_amd_mip_edge
enum MipFilterKind { MIP_FILTER_BOX = 0, MIP_FILTER_MITCHELL = 1, MIP_FILTER_LANCZOS3 = 2, MIP_FILTER_KAISER = 3 };
enum MipFilterEdge { MIP_EDGE_CLAMP = 0, MIP_EDGE_WRAP = 1, MIP_EDGE_CUBE = 2 };
constexpr unsigned int MIP_RESAMPLE_MAX_TAPS = 17;      // s = 3 with support 3

/* The support S of a windowed filter: taps have |t| < S. */
ASTC_MIP_FN int mip_resample_support(int kind) { return kind == MIP_FILTER_MITCHELL ? 2 : 3; }

/* I0 by its power series, a fixed 25 terms: q2 = (x * 0.5) * (x * 0.5); term_0 = sum_0 = 1.0; for k = 1 .. 24
 * term_k = (term_{k-1} * q2) / (double)(k * k), sum_k = sum_{k-1} + term_k. */
inline double mip_resample_i0(double x)
{
	const double q = x * 0.5;
	const double q2 = q * q;
	double term = 1.0, sum = 1.0;
	for (int k = 1; k <= 24; k++)
	{
		term = term * q2 / (double)(k * k);
		sum = sum + term;
	}
	return sum;
}

/* sinc(x) = sin(pi x) / (pi x), px = 3.141592653589793 * x evaluated once; sinc(0) = 1. */
template <typename Sin>
inline double mip_resample_sinc(double x, Sin sin)
{
	if (x == 0.0) return 1.0;
	const double px = 3.141592653589793 * x;
	return sin(px) / px;
}

/* f(a), a = |t| < support:
 *   MITCHELL (B = C = 1/3), a2 = a * a, a3 = a2 * a:
 *     a < 1: ((7.0 * a3 - 12.0 * a2) + 16.0 / 3.0) / 6.0
 *     else:  ((((-7.0 / 3.0) * a3 + 12.0 * a2) - 20.0 * a) + 32.0 / 3.0) / 6.0
 *   LANCZOS3: sinc(a) * sinc(a / 3.0)
 *   KAISER:   q = a / 3.0; (sinc(a) * I0(4.0 * sqrt(1.0 - q * q))) / I0(4.0) */
template <typename Sin>
inline double mip_resample_eval(int kind, double a, Sin sin)
{
	if (kind == MIP_FILTER_MITCHELL)
	{
		const double a2 = a * a, a3 = a2 * a;
		if (a < 1.0) return ((7.0 * a3 - 12.0 * a2) + 16.0 / 3.0) / 6.0;
		return ((((-7.0 / 3.0) * a3 + 12.0 * a2) - 20.0 * a) + 32.0 / 3.0) / 6.0;
	}
	if (kind == MIP_FILTER_LANCZOS3) return mip_resample_sinc(a, sin) * mip_resample_sinc(a / 3.0, sin);
	const double q = a / 3.0;
	return (mip_resample_sinc(a, sin) * mip_resample_i0(4.0 * __builtin_sqrt(1.0 - q * q))) / mip_resample_i0(4.0);
}

/* The taps of destination texel j along an axis whose source has s texels (d = max(1, s >> 1)): writes the integer index of the
 * first tap to *first, the weights to w[0 .. count) and returns count.  Tap k sits at integer i = first + k, read from source
 * texel mip_resample_source(i, s, edge).
 *   s == 1: one tap, i = 0, weight 1.0;
 *   else: r = (double)s / (double)d, c = (double)((2j + 1) * s) / (double)(2d) (the product in 64-bit integers); the taps are
 *   every integer i with |t| < S, t = (((double)i + 0.5) - c) / r, in increasing i; f is evaluated on |t|; the weights are
 *   f_i / sum, sum = f_first + f_first+1 + ... in increasing i. */
template <typename Sin>
inline unsigned int mip_resample_taps(int kind, unsigned int s, unsigned int j, Sin sin, long long* first, double* w)
{
	if (s <= 1)
	{
		*first = 0; w[0] = 1.0;
		return 1;
	}
	*first = 0;
	const unsigned int d = s >> 1;
	const double r = (double)s / (double)d;
	const double c = (double)((2ull * j + 1ull) * (unsigned long long)s) / (double)(2ull * d);
	const double S = (double)mip_resample_support(kind);
	// candidates around the centre (the window spans 2 S r < 2 S * 3 texels); the test below picks the taps exactly
	const long long lo = (long long)(c - S * r) - 3, hi = (long long)(c + S * r) + 3;
	unsigned int n = 0;
	double sum = 0.0;
	for (long long i = lo; i <= hi; i++)
	{
		const double t = (((double)i + 0.5) - c) / r;
		const double a = t < 0.0 ? -t : t;
		if (!(a < S)) continue;
		if (n == 0) *first = i;
		const double f = mip_resample_eval(kind, a, sin);
		w[n] = f;
		sum = n == 0 ? f : sum + f;
		n++;
	}
	for (unsigned int k = 0; k < n; k++) w[k] = w[k] / sum;
	return n;
}

/* The source texel of tap index i (any integer, here within 9 of [0, s)): CLAMP clamp(i, 0, s - 1), WRAP the non-negative
 * i mod s.  (CUBE maps x and y together, mip_cube_source; an axis on its own clamps.) */
ASTC_MIP_FN unsigned int mip_resample_source(long long i, unsigned int s, unsigned int edge)
{
	if (i >= 0 && i < (long long)s) return (unsigned int)i;
	if (edge == MIP_EDGE_WRAP)
	{
		long long m = i % (long long)s;
		return (unsigned int)(m < 0 ? m + (long long)s : m);
	}
	return i < 0 ? 0u : s - 1u;
}

/* MIP_EDGE_CUBE (include/astcenc_amd.h, "Cube edges"): the texel that tap (ix, iy) of face `face` reads in a cube of s x s
 * faces, faces in the order +X, -X, +Y, -Y, +Z, -Z.  Both indices inside [0, s): the texel itself.  Both outside: the face's
 * own corner texel.  One outside, on side 0 (x < 0), 1 (x >= s), 2 (y < 0) or 3 (y >= s): with p the index that is inside,
 * k the overshoot (index - s or -1 - index) and kk = min(k, s - 1), the neighbour's texel at depth kk from the shared edge.
 * Unfolding the neighbour with the face frames of the GL table (P' = sg s A + (s - (2 kk + 1)) M_f + W, x' = (P' . S_f' + s - 1)
 * / 2, y' likewise) makes each of x' and y' one of p, s - 1 - p, kk, s - 1 - kk, so the 24 (face, side) pairs fit a table of
 * bytes: bits 0-2 the neighbour, bits 3-4 the form of x', bits 5-6 that of y' (bit 0 of a form: mirrored, s - 1 - v; bit 1:
 * v = kk instead of p).  tests/mip_cube_model.py works the frames out in full and tests/test_mip_cube_cpu.py compares.
 * (decode_cube.h maps the taps of the cube sampler through this function too: its indices lie in [-1, s].) */
struct MipCubeTexel {
	unsigned int face, x, y;
};

ASTC_MIP_FN MipCubeTexel mip_cube_source(unsigned int face, long long ix, long long iy, unsigned int s)
{
	const long long n = (long long)s;
	const bool in_x = ix >= 0 && ix < n, in_y = iy >= 0 && iy < n;
	MipCubeTexel t;
	t.face = face;
	if (in_x == in_y)
	{
		t.x = in_x ? (unsigned int)ix : ix < 0 ? 0u : s - 1u;
		t.y = in_y ? (unsigned int)iy : iy < 0 ? 0u : s - 1u;
		return t;
	}
	const long long out = in_x ? iy : ix;
	const unsigned int side = (in_x ? 2u : 0u) + (out < 0 ? 0u : 1u);
	const unsigned int p = (unsigned int)(in_x ? ix : iy);
	const long long k = out < 0 ? -1 - out : out - n;
	const unsigned int kk = k < n - 1 ? (unsigned int)k : s - 1u;
	// entry face * 4 + side, eight to a word, entry 0 in the low byte
	const unsigned int e = face * 4u + side;
	const unsigned long long word = e < 8u ? 0x3312141D1B3A151Cull : e < 16u ? 0x6D646069444D4841ull : 0x6B4A111843621019ull;
	const unsigned int code = (unsigned int)(word >> (8u * (e & 7u))) & 0xFFu;
	const unsigned int fx = (code >> 3) & 3u, fy = (code >> 5) & 3u;
	const unsigned int vx = fx & 2u ? kk : p, vy = fy & 2u ? kk : p;
	t.face = code & 7u;
	t.x = fx & 1u ? s - 1u - vx : vx;
	t.y = fy & 1u ? s - 1u - vy : vy;
	return t;
}

/* The float64 channel values of a stored texel: U8 (double)code, or lin[code] for channels 0-2 of sRGB data (lin = the sRGB
 * table of mip_srgb_tables_build, null for linear); F16 the half's value; F32 the float's. */
ASTC_MIP_FN void mip_resample_load_u8(unsigned int p, const double* lin, double v[4])
{
	for (int c = 0; c < 4; c++)
	{
		const unsigned int code = (p >> (8 * c)) & 0xFFu;
		v[c] = lin && c < 3 ? lin[code] : (double)code;
	}
}

ASTC_MIP_FN void mip_resample_load_float(const float f[4], double v[4])
{
	for (int c = 0; c < 4; c++) v[c] = (double)f[c];
}

/* One step of every sum of the filter: sum = w * v when k == 0 (a sum starts at its first product), else sum + w * v, each
 * operation rounded on its own. */
ASTC_MIP_FN void mip_resample_accumulate(double sum[4], double w, const double v[4], unsigned int k)
{
	for (int c = 0; c < 4; c++)
	{
		const double p = w * v[c];
		sum[c] = k == 0 ? p : sum[c] + p;
	}
}

/* The stored results of vol: U8 clamp(floor(vol + 0.5), 0, 255), or mip_srgb_encode(vol, thr) for channels 0-2 of sRGB data
 * (thr null: linear); F32 (float)vol; F16 that float to half (both round to nearest even).  Float data is not clamped. */
ASTC_MIP_FN unsigned int mip_resample_out_u8(const double vol[4], const double* thr)
{
	unsigned int out = 0;
	for (int c = 0; c < 4; c++)
	{
		unsigned int code;
		if (thr && c < 3)
			code = mip_srgb_encode(vol[c], thr);
		else
		{
			const double q = __builtin_floor(vol[c] + 0.5);
			code = q < 0.0 ? 0u : q > 255.0 ? 255u : (unsigned int)q;
		}
		out |= code << (8 * c);
	}
	return out;
}

ASTC_MIP_FN void mip_resample_out_float(const double vol[4], float out[4])
{
	for (int c = 0; c < 4; c++) out[c] = (float)vol[c];
}

/* One destination texel, the reference form of the arithmetic (the kernels share row sums between texels, which changes no
 * bit): for each z tap in increasing order and each y tap in increasing order row = sum_x w_x v, per slice acc = sum_y w_y row,
 * then vol = sum_z w_z acc, every sum starting at its first product.  Taps (first index, count, weights) per axis; load(x, y,
 * z, double v[4]) reads a source texel's values (mip_resample_load_*), the indices already mapped by mip_resample_source. */
struct MipResampleTaps {
	long long first;
	unsigned int count, s, edge;
	const double* w;
};

template <typename Load>
inline void mip_resample_texel(const MipResampleTaps& tx, const MipResampleTaps& ty, const MipResampleTaps& tz, Load load, double vol[4])
{
	for (unsigned int kz = 0; kz < tz.count; kz++)
	{
		const unsigned int z = mip_resample_source(tz.first + kz, tz.s, tz.edge);
		double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
		for (unsigned int ky = 0; ky < ty.count; ky++)
		{
			const unsigned int y = mip_resample_source(ty.first + ky, ty.s, ty.edge);
			double row[4] = { 0.0, 0.0, 0.0, 0.0 };
			for (unsigned int kx = 0; kx < tx.count; kx++)
			{
				double v[4];
				load(mip_resample_source(tx.first + kx, tx.s, tx.edge), y, z, v);
				mip_resample_accumulate(row, tx.w[kx], v, kx);
			}
			mip_resample_accumulate(acc, ty.w[ky], row, ky);
		}
		mip_resample_accumulate(vol, tz.w[kz], acc, kz);
	}
}

/* ... of face `face` of a cube with MIP_EDGE_CUBE (tx.s == ty.s, no z filter: a layer reads its own cube): the same sums, each
 * tap read from mip_cube_source; load(face, x, y, double v[4]).  Taps that land on the same texel are not merged. */
template <typename Load>
inline void mip_resample_texel_cube(unsigned int face, const MipResampleTaps& tx, const MipResampleTaps& ty, Load load, double vol[4])
{
	double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
	for (unsigned int ky = 0; ky < ty.count; ky++)
	{
		double row[4] = { 0.0, 0.0, 0.0, 0.0 };
		for (unsigned int kx = 0; kx < tx.count; kx++)
		{
			const MipCubeTexel t = mip_cube_source(face, tx.first + kx, ty.first + ky, tx.s);
			double v[4];
			load(t.face, t.x, t.y, v);
			mip_resample_accumulate(row, tx.w[kx], v, kx);
		}
		mip_resample_accumulate(acc, ty.w[ky], row, ky);
	}
	mip_resample_accumulate(vol, 1.0, acc, 0);
}

} // namespace astcd
