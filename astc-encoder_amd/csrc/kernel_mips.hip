// SPDX-License-Identifier: Apache-2.0
// Mip chain generation (astcenc_amd_generate_mip_chain_device): every level made from the one above it with the filter of
// mip_filter.h.  Memory-bound, so the launches are shaped by their traffic:
//   - a large level is one launch; a lane makes 16 bytes of output (4 RGBA8, 2 F16 or 1 F32 texels) and stores them at once.
//     When both source axes are even and a source row is a whole number of 32-byte pieces, the lane reads its 2 x 2 footprints
//     with four 16-byte loads (astc_downsample_even); any other level takes the tap loop of the header (astc_downsample_level);
//   - once a source level has at most MIP_TAIL_TEXELS texels, one workgroup makes every remaining level in one launch
//     (astc_downsample_tail): each level lives in LDS, where the next one reads it, and is written out once.
// Texture arrays and cube maps (ASTCENC_AMD_MIP_ARRAY) run the same launches over all layers: a layer's rows follow the
// previous layer's, so the even path is unchanged, the tap loop finds the layer from its row, and the tail runs one
// workgroup per layer.  Volumes (ASTCENC_AMD_MIP_VOLUME) whose source level has more than one slice take the 3D kernels
// astc_mip3d_even / _level / _tail, the same shapes with a z axis; a level whose source depth is 1 takes the 2D kernels with
// one layer, their texels being the 3D filter's of depth 1.  A 2D image is the volume of depth 1, so every level of it does.
// Linear RGBA8 is integer arithmetic only; float64 is used for sRGB channels and float data, as the filter demands.
#include "mip_kernels.h"
#include <cmath>

namespace astcd {

/* One destination texel with the taps (tx, ty), its source texels read by load(x, y) -> stored texel. */
template <int K, typename Load>
__device__ inline typename MipTexel<K>::T mip_texel(const MipTaps& tx, const MipTaps& ty, Load load, const double* srgb)
{
	if constexpr (K == MIP_U8 || K == MIP_U8_SRGB)
	{
		return mip_texel_u8(tx, ty, load, K == MIP_U8_SRGB ? srgb : nullptr, K == MIP_U8_SRGB ? srgb + 256 : nullptr);
	}
	else
	{
		float out[4];
		mip_texel_float(tx, ty, [&](unsigned int x, unsigned int y, float v[4]) { mip_unpack<K>(load(x, y), v); }, out);
		if constexpr (K == MIP_F16) return mip_pack_f16(out);
		else return make_float4(out[0], out[1], out[2], out[3]);
	}
}

/* ... and in a volume: load(x, y, z). */
template <int K, typename Load>
__device__ inline typename MipTexel<K>::T mip_texel_3d(const MipTaps& tx, const MipTaps& ty, const MipTaps& tz, Load load, const double* srgb)
{
	if constexpr (K == MIP_U8 || K == MIP_U8_SRGB)
	{
		return mip_texel_u8_3d(tx, ty, tz, load, K == MIP_U8_SRGB ? srgb : nullptr, K == MIP_U8_SRGB ? srgb + 256 : nullptr);
	}
	else
	{
		float out[4];
		mip_texel_float_3d(tx, ty, tz, [&](unsigned int x, unsigned int y, unsigned int z, float v[4]) { mip_unpack<K>(load(x, y, z), v); }, out);
		if constexpr (K == MIP_F16) return mip_pack_f16(out);
		else return make_float4(out[0], out[1], out[2], out[3]);
	}
}

/* Even source axes: a lane's 16 bytes of output from two source rows of 32 bytes each (four 16-byte loads).  Launched only when
 * the source is 16-byte aligned and its row pitch a multiple of 32 bytes, so every load is aligned and units_x = sx_bytes / 32. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_downsample_even(const uint8_t* __restrict__ src, size_t src_pitch, uint8_t* __restrict__ dst, size_t dst_pitch, uint32_t units_x,
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
			// four texels, each the rounded mean (s + 2) >> 2 of its 2 x 2 footprint: the channels in two 16-bit SIMD halves
			const uint32_t ra[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
			const uint32_t rb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
			uint32_t o[4];
			#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const uint32_t p0 = ra[2 * k], p1 = ra[2 * k + 1], p2 = rb[2 * k], p3 = rb[2 * k + 1];
				const uint32_t lo = (p0 & 0x00FF00FFu) + (p1 & 0x00FF00FFu) + (p2 & 0x00FF00FFu) + (p3 & 0x00FF00FFu) + 0x00020002u;
				const uint32_t hi = ((p0 >> 8) & 0x00FF00FFu) + ((p1 >> 8) & 0x00FF00FFu) + ((p2 >> 8) & 0x00FF00FFu) + ((p3 >> 8) & 0x00FF00FFu) + 0x00020002u;
				o[k] = ((lo >> 2) & 0x00FF00FFu) | (((hi >> 2) & 0x00FF00FFu) << 8);
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
				res[k] = mip_texel<K>(t, t, [&](unsigned int x, unsigned int yy) { return yy ? row1[2 * k + x] : row0[2 * k + x]; }, srgb);
			}
			__builtin_memcpy(&out, res, 16);
		}
		*reinterpret_cast<uint4*>(dst + y * dst_pitch + (size_t)ux * 16) = out;
	}
}

/* Any level: a lane makes the 16 / sizeof(T) destination texels from x = ux * that on, through the tap loop of the header;
 * one 16-byte store when they are all there and the address allows it, texel stores otherwise.  The rows of all layers in
 * one range: row r is row r mod dy of layer r / dy. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_downsample_level(const void* __restrict__ src, uint32_t sx, uint32_t sy, uint8_t* __restrict__ dst, uint32_t dx, uint32_t dy,
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
			res[k] = mip_texel<K>(tx, ty, [&](unsigned int x, unsigned int yy) { return mip_load_global<K>(src, base + (size_t)yy * sx + x); }, srgb);
		}
		const size_t at = r * dx + x0;
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
}

/* The rest of the chain in one workgroup per layer: level k + 1 is made from level k (k = 0: `src` in global memory, then the
 * LDS copy of the level before), kept in LDS for the next one and written to dst[k].  Layer l's levels follow the l levels
 * of the layers before it; a workgroup takes layers blockIdx.x, + gridDim.x, ... */
template <int K>
__global__ void __launch_bounds__(MIP_TAIL_THREADS)
astc_downsample_tail(MipTailArgs a, uint32_t layers, const double* __restrict__ srgb)
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
					v = mip_texel<K>(tx, ty, [&](unsigned int xx, unsigned int yy) { return mip_load_global<K>(src, (size_t)yy * sx + xx); }, srgb);
				else
					v = mip_texel<K>(tx, ty, [&](unsigned int xx, unsigned int yy) { return in[yy * sx + xx]; }, srgb);
				out[t] = v;
				g[t] = v;
			}
			__syncthreads();
			sx = dx; sy = dy;
		}
	}
}

/* Volumes, all three source axes even: a lane's 16 bytes of output from two slices x two rows of 32 bytes each (eight 16-byte
 * loads).  As astc_downsample_even: launched only when the source is 16-byte aligned and its row pitch a multiple of 32 bytes.
 * The destination rows of all slices in one range: row r is row r mod dy of slice r / dy. */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mip3d_even(const uint8_t* __restrict__ src, size_t src_pitch, uint32_t sy, uint8_t* __restrict__ dst, size_t dst_pitch, uint32_t dy,
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
			// four texels, each the rounded mean (s + 4) >> 3 of its 2 x 2 x 2 footprint: the channels in two 16-bit SIMD
			// halves (8 * 255 + 4 fits in 16 bits)
			const uint32_t ra[8] = { a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w };
			const uint32_t rb[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
			const uint32_t rc[8] = { c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w };
			const uint32_t rd[8] = { d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w };
			uint32_t o[4];
			#pragma unroll
			for (int k = 0; k < 4; k++)
			{
				const uint32_t q[8] = { ra[2 * k], ra[2 * k + 1], rb[2 * k], rb[2 * k + 1], rc[2 * k], rc[2 * k + 1], rd[2 * k], rd[2 * k + 1] };
				uint32_t lo = 0x00040004u, hi = 0x00040004u;
				#pragma unroll
				for (int i = 0; i < 8; i++)
				{
					lo += q[i] & 0x00FF00FFu;
					hi += (q[i] >> 8) & 0x00FF00FFu;
				}
				o[k] = ((lo >> 3) & 0x00FF00FFu) | (((hi >> 3) & 0x00FF00FFu) << 8);
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
				res[k] = mip_texel_3d<K>(t, t, t, [&](unsigned int x, unsigned int yy, unsigned int zz) { return row[zz * 2 + yy][2 * k + x]; }, srgb);
			}
			__builtin_memcpy(&out, res, 16);
		}
		*reinterpret_cast<uint4*>(dst + r * dst_pitch + (size_t)ux * 16) = out;
	}
}

/* Volumes, any shape: astc_downsample_level with a z axis (3 x 3 x 3 taps at most). */
template <int K>
__global__ void __launch_bounds__(MIP_THREADS)
astc_mip3d_level(const void* __restrict__ src, uint32_t sx, uint32_t sy, uint32_t sz, uint8_t* __restrict__ dst, uint32_t dx, uint32_t dy,
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
			res[k] = mip_texel_3d<K>(tx, ty, tz, [&](unsigned int x, unsigned int yy, unsigned int zz) {
				return mip_load_global<K>(src, ((size_t)zz * sy + yy) * sx + x); }, srgb);
		}
		const size_t at = r * dx + x0;
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
}

/* Volumes: the rest of the chain in one workgroup once a source level has at most MIP_TAIL_TEXELS texels (a destination has
 * at most half its source's texels, so the 2D tail's buffers hold every level). */
template <int K>
__global__ void __launch_bounds__(MIP_TAIL_THREADS)
astc_mip3d_tail(Mip3dTailArgs a, const double* __restrict__ srgb)
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
				v = mip_texel_3d<K>(tx, ty, tz, [&](unsigned int xx, unsigned int yy, unsigned int zz) {
					return mip_load_global<K>(a.src, ((size_t)zz * sy + yy) * sx + xx); }, srgb);
			else
				v = mip_texel_3d<K>(tx, ty, tz, [&](unsigned int xx, unsigned int yy, unsigned int zz) { return in[(zz * sy + yy) * sx + xx]; }, srgb);
			out[t] = v;
			g[t] = v;
		}
		__syncthreads();
		sx = dx; sy = dy; sz = dz;
	}
}


template <int K>
static int mip_launch_kind(const MipChainJob& job, const double* srgb, hipStream_t stream)
{
	const MipKernels ks = { astc_downsample_even<K>, astc_downsample_level<K>, astc_downsample_tail<K>,
	                        astc_mip3d_even<K>, astc_mip3d_level<K>, astc_mip3d_tail<K> };
	return mip_launch_chain<K>(job, srgb, stream, ks);
}

int astc_mip_launch(const MipChainJob& job, const void* d_srgb, void* stream)
{
	if (job.level_count < 2) return 0;
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? mip_launch_kind<MIP_U8_SRGB>(job, srgb, s) : mip_launch_kind<MIP_U8>(job, srgb, s);
	case 1: return mip_launch_kind<MIP_F16>(job, srgb, s);
	default: return mip_launch_kind<MIP_F32>(job, srgb, s);
	}
}

size_t astc_mip_srgb_table_bytes() { return MIP_SRGB_TABLE_DOUBLES * sizeof(double); }

void astc_mip_srgb_tables_build(void* out)
{
	mip_srgb_tables_build(static_cast<double*>(out), [](double x, double y) { return ::pow(x, y); });
}

} // namespace astcd
