// SPDX-License-Identifier: Apache-2.0
// Mip chain generation with alpha-weighted colour (astcenc_amd_generate_mip_chain_weighted_device with
// ASTCENC_AMD_MIP_WEIGHT_ALPHA): the arithmetic of mip_weighted.h in kernels of their own, astc_mipw_*, so that the plain
// kernels stay as they are.
//
// Box filter: the six kernel shapes and the launch rules of kernel_mips.hip (mip_kernels.h) -- even levels with 16-byte loads
// and one 16-byte store per lane, the tap loop for any other level, the LDS tail for the rest of the chain, and their volume
// forms.  They move exactly the bytes of the plain kernels.  The even RGBA8 kernels are the ones that matter for speed.  Per
// destination texel they add SA = sum a and SP_c = sum a c over the footprint (4 or 8 texels, all of weight 1) and three exact
// divisions (2 SP_c + SA) / (2 SA): the numerator is below 2^20 and the divisor at most 4080, so one v_rcp_f32 per texel, a
// multiply per channel and a +-1 integer correction give the exact quotient; there is no float64 and no 64-bit integer on that
// path.  A footprint with SA == 0 keeps the plain kernel's SIMD-halves mean, by a select rather than a branch.
//
// Windowed filters: the two shapes of kernel_mip_filter.hip over the same table of taps (mip_filter_kernels.h), at the end of
// the file.
#include "mip_kernels.h"
#include "mip_filter_kernels.h"

namespace astcd {

/* One destination texel with the taps (tx, ty), its source texels read by load(x, y) -> stored texel. */
template <int K, typename Load>
__device__ inline typename MipTexel<K>::T mipw_texel(const MipTaps& tx, const MipTaps& ty, Load load, const double* srgb)
{
	if constexpr (K == MIP_U8 || K == MIP_U8_SRGB)
	{
		return mip_texel_u8_weighted(tx, ty, load, K == MIP_U8_SRGB ? srgb : nullptr, K == MIP_U8_SRGB ? srgb + 256 : nullptr);
	}
	else
	{
		float out[4];
		mip_texel_float_weighted(tx, ty, [&](unsigned int x, unsigned int y, float v[4]) { mip_unpack<K>(load(x, y), v); }, out);
		if constexpr (K == MIP_F16) return mip_pack_f16(out);
		else return make_float4(out[0], out[1], out[2], out[3]);
	}
}

/* ... and in a volume: load(x, y, z). */
template <int K, typename Load>
__device__ inline typename MipTexel<K>::T mipw_texel_3d(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, const double* srgb)
{
	if constexpr (K == MIP_U8 || K == MIP_U8_SRGB)
	{
		return mip_texel_u8_3d_weighted(tx, ty, tz, load, K == MIP_U8_SRGB ? srgb : nullptr, K == MIP_U8_SRGB ? srgb + 256 : nullptr);
	}
	else
	{
		float out[4];
		mip_texel_float_3d_weighted(tx, ty, tz, [&](unsigned int x, unsigned int y, unsigned int z, float v[4]) { mip_unpack<K>(load(x, y, z), v); }, out);
		if constexpr (K == MIP_F16) return mip_pack_f16(out);
		else return make_float4(out[0], out[1], out[2], out[3]);
	}
}

/* One linear RGBA8 texel of an even level from its N = 4 or 8 source texels (all of weight 1): the rounded plain mean
 * (s + N / 2) / N in two 16-bit SIMD halves, as the plain kernels make it, and with SA > 0 channels 0-2 replaced by
 * (2 SP_c + SA) / (2 SA).  num = 2 SP_c + SA <= 2 * 8 * 255 * 255 + 2040 < 2^20 is exact in float, den = 2 SA <= 4080, the
 * quotient is at most 255: (float)num * rcp((float)den) is within 1e-3 of it, so its floor is the quotient or one beside it,
 * which the remainder tells. */
template <int N>
__device__ inline uint32_t mipw_even_u8(const uint32_t (&q)[N])
{
	constexpr uint32_t HALF = (uint32_t)(N / 2) * 0x00010001u;
	constexpr int SHIFT = N == 4 ? 2 : 3;
	uint32_t lo = HALF, hi = HALF, sa = 0, sp[3] = { 0, 0, 0 };
	#pragma unroll
	for (int i = 0; i < N; i++)
	{
		lo += q[i] & 0x00FF00FFu;
		hi += (q[i] >> 8) & 0x00FF00FFu;
		const uint32_t a = q[i] >> 24;
		sa += a;
		#pragma unroll
		for (int c = 0; c < 3; c++) sp[c] += a * ((q[i] >> (8 * c)) & 0xFFu);
	}
	const uint32_t plain = ((lo >> SHIFT) & 0x00FF00FFu) | (((hi >> SHIFT) & 0x00FF00FFu) << 8);
	const uint32_t den = sa ? 2u * sa : 1u;
	const float r = __builtin_amdgcn_rcpf((float)den);
	uint32_t out = plain & 0xFF000000u;
	#pragma unroll
	for (int c = 0; c < 3; c++)
	{
		const uint32_t num = 2u * sp[c] + sa;
		uint32_t v = (uint32_t)((float)num * r);
		const int32_t rem = (int32_t)(num - v * den);
		v = rem < 0 ? v - 1u : rem >= (int32_t)den ? v + 1u : v;
		out |= v << (8 * c);
	}
	return sa ? out : plain;
}

/* Even source axes: astc_downsample_even's loads and store. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mipw_even(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, size_t dst_pitch, uint32_t units_x,
               size_t units, const double* __restrict__ srgb)
{
	const size_t stride = (size_t)gridDim.x * MIP_THREADS;
	for (size_t u = (size_t)blockIdx.x * MIP_THREADS + threadIdx.x; u < units; u += stride)
	{
		uint32_t ux; size_t y;
		mip_unit_xy(u, units_x, ux, y);
		const uint4* r0 = reinterpret_cast<const uint4*>(src + 2 * y * src_pitch + (size_t)ux * 32);
		const uint4* r1 = reinterpret_cast<const uint4*>(src + (2 * y + 1) * src_pitch + (size_t)ux * 32);
		const uint4 a0 = r0[0], a1 = r0[1], b0 = r1[0], b1 = r1[1];
		uint4 out;
		if constexpr (K == MIP_U8)
		{
			const uint32_t ra[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
			const uint32_t rb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
			uint32_t o[4];
			#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const uint32_t q[4] = { ra[2 * k], ra[2 * k + 1], rb[2 * k], rb[2 * k + 1] };
				o[k] = mipw_even_u8<4>(q);
			}
			out = make_uint4(o[0], o[1], o[2], o[3]);
		}
		else
		{
			// the tap loop of the header over the loaded texels (taps of an even axis, in the lane's own coordinates)
			typedef typename MipTexel<K>::T T;
			constexpr int PER = 32 / (int)sizeof(T);            // source texels per 32-byte row piece
			T row0[PER], row1[PER];
			__builtin_memcpy(&row0[0], &a0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row0) + 16, &a1, 16);
			__builtin_memcpy(&row1[0], &b0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row1) + 16, &b1, 16);
			T res[PER / 2];
			#pragma unroll
			for (int k = 0; k < PER / 2; k++)
			{
				const MipTaps t = mip_axis_taps(2, 0);
				res[k] = mipw_texel<K>(t, t, [&](unsigned int x, unsigned int yy) { return yy ? row1[2 * k + x] : row0[2 * k + x]; }, srgb);
			}
			__builtin_memcpy(&out, res, 16);
		}
		*reinterpret_cast<uint4*>(dst + y * dst_pitch + (size_t)ux * 16) = out;
	}
}

/* Stores a lane's 16 / sizeof(T) texels from x0 on at texel `at` of dst: one 16-byte store when they are all there and the
 * address allows it, texel stores otherwise. */
template <typename T>
__device__ inline void mipw_store_unit(uint8_t* dst, size_t at, uint32_t x0, uint32_t dx, const T* res)
{
	constexpr uint32_t TPL = 16 / (uint32_t)sizeof(T);
	T* out = reinterpret_cast<T*>(dst) + at;
	if (x0 + TPL <= dx && ((at * sizeof(T)) & 15u) == 0)
	{
		uint4 v;
		__builtin_memcpy(&v, res, 16);
		*reinterpret_cast<uint4*>(out) = v;
	}
	else
	{
		for (uint32_t k = 0; k < TPL && x0 + k < dx; k++) out[k] = res[k];
	}
}

/* Any level: astc_downsample_level's units (the rows of all layers in one range) through the weighted tap loop. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mipw_level(const void* __restrict__ src, uint32_t sx, uint32_t sy, uint8_t* __restrict__ dst, uint32_t dx, uint32_t dy,
                uint32_t units_x, size_t units, const double* __restrict__ srgb)
{
	typedef typename MipTexel<K>::T T;
	constexpr uint32_t TPL = 16 / (uint32_t)sizeof(T);
	const size_t stride = (size_t)gridDim.x * MIP_THREADS;
	for (size_t u = (size_t)blockIdx.x * MIP_THREADS + threadIdx.x; u < units; u += stride)
	{
		uint32_t ux; size_t r;
		mip_unit_xy(u, units_x, ux, r);
		size_t layer; uint32_t y;
		mip_row_layer(r, dy, layer, y);
		const size_t base = layer * sx * sy;
		const MipTaps ty = mip_axis_taps(sy, y);
		const uint32_t x0 = ux * TPL;
		T res[TPL];
		#pragma unroll
		for (uint32_t k = 0; k < TPL; k++)
		{
			if (x0 + k >= dx) break;
			const MipTaps tx = mip_axis_taps(sx, x0 + k);
			res[k] = mipw_texel<K>(tx, ty, [&](unsigned int x, unsigned int yy) { return mip_load_global<K>(src, base + (size_t)yy * sx + x); }, srgb);
		}
		mipw_store_unit<T>(dst, r * dx + x0, x0, dx, res);
	}
}

/* The rest of the chain in one workgroup per layer: astc_downsample_tail with the weighted texel. */
template <int K>
__global__ void __launch_bounds__(MIP_TAIL_THREADS)
astc_mipw_tail(MipTailArgs a, uint32_t layers, const double* __restrict__ srgb)
{
	typedef typename MipTexel<K>::T T;
	__shared__ T buf[2][MIP_TAIL_DST_TEXELS];
	for (uint32_t layer = blockIdx.x; layer < layers; layer += gridDim.x)
	{
		uint32_t sx = a.sx, sy = a.sy;
		const T* src = reinterpret_cast<const T*>(a.src) + (size_t)layer * sx * sy;
		for (uint32_t k = 0; k < a.levels; k++)
		{
			const uint32_t dx = sx > 1 ? sx >> 1 : 1u, dy = sy > 1 ? sy >> 1 : 1u;
			T* out = buf[k & 1];
			const T* in = buf[(k & 1) ^ 1];
			T* g = reinterpret_cast<T*>(a.dst[k]) + (size_t)layer * dx * dy;
			for (uint32_t t = threadIdx.x; t < dx * dy; t += MIP_TAIL_THREADS)
			{
				const uint32_t y = t / dx, x = t - y * dx;
				const MipTaps tx = mip_axis_taps(sx, x), ty = mip_axis_taps(sy, y);
				T v;
				if (k == 0)
					v = mipw_texel<K>(tx, ty, [&](unsigned int xx, unsigned int yy) { return mip_load_global<K>(src, (size_t)yy * sx + xx); }, srgb);
				else
					v = mipw_texel<K>(tx, ty, [&](unsigned int xx, unsigned int yy) { return in[yy * sx + xx]; }, srgb);
				out[t] = v;
				g[t] = v;
			}
			__syncthreads();
			sx = dx; sy = dy;
		}
	}
}

/* Volumes, all three source axes even: astc_mip3d_even's loads and store. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mipw_even3d(const uint8_t* __restrict__ src, size_t src_pitch, uint32_t sy, uint8_t* __restrict__ dst, size_t dst_pitch, uint32_t dy,
                 uint32_t units_x, size_t units, const double* __restrict__ srgb)
{
	const size_t stride = (size_t)gridDim.x * MIP_THREADS;
	const size_t slice_pitch = (size_t)sy * src_pitch;
	for (size_t u = (size_t)blockIdx.x * MIP_THREADS + threadIdx.x; u < units; u += stride)
	{
		uint32_t ux; size_t r;
		mip_unit_xy(u, units_x, ux, r);
		size_t z; uint32_t y;
		mip_row_layer(r, dy, z, y);
		const uint8_t* p = src + 2 * z * slice_pitch + (size_t)(2 * y) * src_pitch + (size_t)ux * 32;
		const uint4* r00 = reinterpret_cast<const uint4*>(p);
		const uint4* r01 = reinterpret_cast<const uint4*>(p + src_pitch);
		const uint4* r10 = reinterpret_cast<const uint4*>(p + slice_pitch);
		const uint4* r11 = reinterpret_cast<const uint4*>(p + slice_pitch + src_pitch);
		const uint4 a0 = r00[0], a1 = r00[1], b0 = r01[0], b1 = r01[1], c0 = r10[0], c1 = r10[1], d0 = r11[0], d1 = r11[1];
		uint4 out;
		if constexpr (K == MIP_U8)
		{
			const uint32_t ra[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
			const uint32_t rb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
			const uint32_t rc[8] = { c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w };
			const uint32_t rd[8] = { d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w };
			uint32_t o[4];
			#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const uint32_t q[8] = { ra[2 * k], ra[2 * k + 1], rb[2 * k], rb[2 * k + 1], rc[2 * k], rc[2 * k + 1], rd[2 * k], rd[2 * k + 1] };
				o[k] = mipw_even_u8<8>(q);
			}
			out = make_uint4(o[0], o[1], o[2], o[3]);
		}
		else
		{
			typedef typename MipTexel<K>::T T;
			constexpr int PER = 32 / (int)sizeof(T);
			T row[4][PER];                                       // [slice * 2 + row]
			__builtin_memcpy(&row[0][0], &a0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row[0]) + 16, &a1, 16);
			__builtin_memcpy(&row[1][0], &b0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row[1]) + 16, &b1, 16);
			__builtin_memcpy(&row[2][0], &c0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row[2]) + 16, &c1, 16);
			__builtin_memcpy(&row[3][0], &d0, 16); __builtin_memcpy(reinterpret_cast<uint8_t*>(row[3]) + 16, &d1, 16);
			T res[PER / 2];
			#pragma unroll
			for (int k = 0; k < PER / 2; k++)
			{
				const MipTaps t = mip_axis_taps(2, 0);
				res[k] = mipw_texel_3d<K>(t, t, t, [&](unsigned int x, unsigned int yy, unsigned int zz) { return row[zz * 2 + yy][2 * k + x]; }, srgb);
			}
			__builtin_memcpy(&out, res, 16);
		}
		*reinterpret_cast<uint4*>(dst + r * dst_pitch + (size_t)ux * 16) = out;
	}
}

/* Volumes, any shape: astc_mip3d_level's units through the weighted tap loop. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mipw_level3d(const void* __restrict__ src, uint32_t sx, uint32_t sy, uint32_t sz, uint8_t* __restrict__ dst, uint32_t dx, uint32_t dy,
                  uint32_t units_x, size_t units, const double* __restrict__ srgb)
{
	typedef typename MipTexel<K>::T T;
	constexpr uint32_t TPL = 16 / (uint32_t)sizeof(T);
	const size_t stride = (size_t)gridDim.x * MIP_THREADS;
	for (size_t u = (size_t)blockIdx.x * MIP_THREADS + threadIdx.x; u < units; u += stride)
	{
		uint32_t ux; size_t r;
		mip_unit_xy(u, units_x, ux, r);
		size_t z; uint32_t y;
		mip_row_layer(r, dy, z, y);
		const MipTaps ty = mip_axis_taps(sy, y), tz = mip_axis_taps(sz, (uint32_t)z);
		const uint32_t x0 = ux * TPL;
		T res[TPL];
		#pragma unroll
		for (uint32_t k = 0; k < TPL; k++)
		{
			if (x0 + k >= dx) break;
			const MipTaps tx = mip_axis_taps(sx, x0 + k);
			res[k] = mipw_texel_3d<K>(tx, ty, tz, [&](unsigned int x, unsigned int yy, unsigned int zz) {
				return mip_load_global<K>(src, ((size_t)zz * sy + yy) * sx + x); }, srgb);
		}
		mipw_store_unit<T>(dst, r * dx + x0, x0, dx, res);
	}
}

/* Volumes: the rest of the chain in one workgroup, astc_mip3d_tail with the weighted texel. */
template <int K>
__global__ void __launch_bounds__(MIP_TAIL_THREADS)
astc_mipw_tail3d(Mip3dTailArgs a, const double* __restrict__ srgb)
{
	typedef typename MipTexel<K>::T T;
	__shared__ T buf[2][MIP_TAIL_DST_TEXELS];
	uint32_t sx = a.sx, sy = a.sy, sz = a.sz;
	for (uint32_t k = 0; k < a.levels; k++)
	{
		const uint32_t dx = sx > 1 ? sx >> 1 : 1u, dy = sy > 1 ? sy >> 1 : 1u, dz = sz > 1 ? sz >> 1 : 1u;
		T* out = buf[k & 1];
		const T* in = buf[(k & 1) ^ 1];
		T* g = reinterpret_cast<T*>(a.dst[k]);
		for (uint32_t t = threadIdx.x; t < dx * dy * dz; t += MIP_TAIL_THREADS)
		{
			const uint32_t zy = t / dx, x = t - zy * dx, z = zy / dy, y = zy - z * dy;
			const MipTaps tx = mip_axis_taps(sx, x), ty = mip_axis_taps(sy, y), tz = mip_axis_taps(sz, z);
			T v;
			if (k == 0)
				v = mipw_texel_3d<K>(tx, ty, tz, [&](unsigned int xx, unsigned int yy, unsigned int zz) {
					return mip_load_global<K>(a.src, ((size_t)zz * sy + yy) * sx + xx); }, srgb);
			else
				v = mipw_texel_3d<K>(tx, ty, tz, [&](unsigned int xx, unsigned int yy, unsigned int zz) { return in[(zz * sy + yy) * sx + xx]; }, srgb);
			out[t] = v;
			g[t] = v;
		}
		__syncthreads();
		sx = dx; sy = dy; sz = dz;
	}
}

template <int K>
static int mipw_launch_kind(const MipChainJob& job, const double* srgb, hipStream_t stream)
{
	const MipKernels ks = { astc_mipw_even<K>, astc_mipw_level<K>, astc_mipw_tail<K>, astc_mipw_even3d<K>, astc_mipw_level3d<K>, astc_mipw_tail3d<K> };
	return mip_launch_chain<K>(job, srgb, stream, ks);
}

int astc_mip_weighted_launch(const MipChainJob& job, const void* d_srgb, void* stream)
{
	if (job.level_count < 2) return 0;
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? mipw_launch_kind<MIP_U8_SRGB>(job, srgb, s) : mipw_launch_kind<MIP_U8>(job, srgb, s);
	case 1: return mipw_launch_kind<MIP_F16>(job, srgb, s);
	default: return mipw_launch_kind<MIP_F32>(job, srgb, s);
	}
}

/* The windowed filters (kernel_mip_filter.hip's two shapes over the same table) with seven sums per texel: the plain four, whose
 * alpha sum is volA, and volP_0..2, so that a texel whose volA > 0.0 fails has its plain colour at hand.  Seven float64 values
 * in the plain 32 x 16 tile would need 84 KiB of LDS; the weighted tile is MIP_RSW_TX = 16 wide instead (42 KiB, one destination
 * texel per thread).  A narrower tile costs no arithmetic: a row sum depends only on (source row, destination x), and the rows
 * a tile stages depend on its height alone, which stays MIP_RS_TY. */
namespace {

/* The weighted tile: mip_rs_tile with seven values per source texel and MIP_RSW_TX columns (tile index: x, then y, then slice,
 * with the tile's own tiles_x). */

struct MipRswShared {
	double rows[MIP_RS_ROWS][MIP_RSW_TX][MIP_WEIGHTED_VALUES];
	double srgb[MIP_SRGB_TABLE_DOUBLES];
};

__device__ inline uint32_t mip_rsw_tiles_x(const MipRsLevel& L) { return (L.dx + MIP_RSW_TX - 1) / MIP_RSW_TX; }

template <int K>
__device__ void mip_rsw_tile(const uint8_t* table, const MipRsLevel& L, size_t tile, MipRswShared& sh)
{
	const uint32_t tiles_x = mip_rsw_tiles_x(L), tiles_xy = tiles_x * L.tiles_y;
	const uint32_t slice = (uint32_t)(tile / tiles_xy), txy = (uint32_t)(tile - (size_t)slice * tiles_xy);
	const uint32_t ty_i = txy / tiles_x, tx_i = txy - ty_i * tiles_x;
	const uint32_t x0 = tx_i * MIP_RSW_TX, y0 = ty_i * MIP_RS_TY;
	const uint32_t ylast = (y0 + MIP_RS_TY < L.dy ? y0 + MIP_RS_TY : L.dy) - 1;
	const MipRsTaps t_lo = mip_rs_taps(table, L.ax[1], y0), t_hi = mip_rs_taps(table, L.ax[1], ylast);
	const long long ylo = t_lo.first;
	const uint32_t nrows = (uint32_t)(t_hi.first + t_hi.count - ylo);
	const MipRsTaps tz = L.array ? MipRsTaps{ (long long)slice, 1u, nullptr } : mip_rs_taps(table, L.ax[2], slice);
	const double* lin = K == MIP_RS_U8_SRGB ? sh.srgb : nullptr;
	const uint32_t c = threadIdx.x % MIP_RSW_TX, x = x0 + c, y = y0 + threadIdx.x / MIP_RSW_TX;
	const bool mine = x < L.dx && y < L.dy;

	double vol[7] = {};
	for (uint32_t kz = 0; kz < tz.count; kz++)
	{
		const uint32_t zs = L.array ? slice : mip_resample_source(tz.first + kz, L.sz, L.ax[2].edge);
		const double wz = L.array ? 1.0 : tz.w[kz];
		// x pass: a thread's column is the same for every row it takes (MIP_RS_THREADS is a multiple of MIP_RSW_TX)
		if (x < L.dx)
		{
			const MipRsTaps tx = mip_rs_taps(table, L.ax[0], x);
			for (uint32_t r = threadIdx.x / MIP_RSW_TX; r < nrows; r += MIP_RS_THREADS / MIP_RSW_TX)
			{
				const uint32_t ys = mip_resample_source(ylo + r, L.sy, L.ax[1].edge);
				const size_t base = ((size_t)zs * L.sy + ys) * L.sx;
				double sum[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
				for (uint32_t k = 0; k < tx.count; k++)
				{
					double v[7];
					mip_rsw_load<K>(L.src, base + mip_resample_source(tx.first + k, L.sx, L.ax[0].edge), lin, v);
					mip_resample_accumulate7(sum, tx.w[k], v, k);
				}
				for (int ch = 0; ch < 7; ch++) sh.rows[r][c][ch] = sum[ch];
			}
		}
		__syncthreads();
		// y pass from LDS, then this z tap's share of vol
		if (mine)
		{
			const MipRsTaps ty = mip_rs_taps(table, L.ax[1], y);
			double acc[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
			for (uint32_t k = 0; k < ty.count; k++)
			{
				const uint32_t r = (uint32_t)(ty.first + k - ylo);
				double row[7];
				for (int ch = 0; ch < 7; ch++) row[ch] = sh.rows[r][c][ch];
				mip_resample_accumulate7(acc, ty.w[k], row, k);
			}
			mip_resample_accumulate7(vol, wz, acc, kz);
		}
		__syncthreads();
	}
	if (mine) mip_rsw_store<K>(L.dst, ((size_t)slice * L.dy + y) * L.dx + x, vol, sh.srgb + 256);
}

template <int K>
__device__ inline void mip_rsw_srgb_to_lds(const double* srgb, MipRswShared& sh)
{
	if constexpr (K == MIP_RS_U8_SRGB)
		for (uint32_t i = threadIdx.x; i < MIP_SRGB_TABLE_DOUBLES; i += MIP_RS_THREADS) sh.srgb[i] = srgb[i];
	__syncthreads();
}

} // namespace

/* astc_mipfilter_level / _tail with the weighted tile. */
template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipw_filter_level(const uint8_t* table, uint32_t level, const double* srgb)
{
	__shared__ MipRswShared sh;
	mip_rsw_srgb_to_lds<K>(srgb, sh);
	const MipRsLevel& L = reinterpret_cast<const MipRsLevel*>(table)[level];
	const size_t tiles = (size_t)mip_rsw_tiles_x(L) * L.tiles_y * L.dz;
	for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) mip_rsw_tile<K>(table, L, t, sh);
}

template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipw_filter_tail(const uint8_t* table, uint32_t first, uint32_t levels, uint32_t layers, const double* srgb)
{
	__shared__ MipRswShared sh;
	mip_rsw_srgb_to_lds<K>(srgb, sh);
	for (uint32_t layer = blockIdx.x; layer < layers; layer += gridDim.x)
		for (uint32_t lv = first; lv < levels; lv++)
		{
			const MipRsLevel& L = reinterpret_cast<const MipRsLevel*>(table)[lv];
			const size_t per = (size_t)mip_rsw_tiles_x(L) * L.tiles_y;
			const size_t t0 = L.array ? (size_t)layer * per : 0, t1 = L.array ? t0 + per : per * L.dz;
			for (size_t t = t0; t < t1; t++) mip_rsw_tile<K>(table, L, t, sh);
			__syncthreads();
		}
}

template <int K>
static int mipw_filter_launch_kind(const MipChainJob& job, const uint8_t* d_table, const double* srgb, hipStream_t stream)
{
	return mip_rs_launch_chain(job, d_table, srgb, stream, astc_mipw_filter_tail<K>, astc_mipw_filter_level<K>, MIP_RSW_TX);
}

int astc_mip_filter_weighted_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream)
{
	if (job.level_count < 2) return 0;
	const uint8_t* t = static_cast<const uint8_t*>(d_table);
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? mipw_filter_launch_kind<MIP_RS_U8_SRGB>(job, t, srgb, s) : mipw_filter_launch_kind<MIP_RS_U8>(job, t, srgb, s);
	case 1: return mipw_filter_launch_kind<MIP_RS_F16>(job, t, srgb, s);
	default: return mipw_filter_launch_kind<MIP_RS_F32>(job, t, srgb, s);
	}
}

} // namespace astcd
