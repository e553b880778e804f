// SPDX-License-Identifier: Apache-2.0
// What the box filter's kernels share (kernel_mips.hip: the plain filter of mip_filter.h; kernel_mip_weighted.hip: the
// alpha-weighted one of mip_weighted.h): the kinds of data and how a stored texel is loaded and unpacked, the index arithmetic
// of a lane's unit, and the launch rules of a chain -- which of the six kernel shapes makes which level.
// Both files give mip_launch_chain their own kernels of those shapes.
#pragma once
#include "backend.h"
#include "mip_filter.h"
#include <hip/hip_runtime.h>
#include <cstring>

namespace astcd {

// the kinds of data a level holds: which arithmetic of mip_filter.h runs
enum MipKind { MIP_U8 = 0, MIP_U8_SRGB = 1, MIP_F16 = 2, MIP_F32 = 3 };
constexpr uint32_t MIP_TAIL_TEXELS = 4096;      // a source level this small: the rest of the chain in one workgroup
constexpr uint32_t MIP_TAIL_DST_TEXELS = 2048;  // ... whose destinations have at most half as many texels (LDS buffer size)
constexpr uint32_t MIP_TAIL_THREADS = 1024;
constexpr uint32_t MIP_THREADS = 256;
constexpr uint32_t MIP_MAX_GROUPS = 1u << 20;

template <int K> struct MipTexel;                           // a texel as it is stored
template <> struct MipTexel<MIP_U8> { typedef uint32_t T; };
template <> struct MipTexel<MIP_U8_SRGB> { typedef uint32_t T; };
template <> struct MipTexel<MIP_F16> { typedef uint2 T; };
template <> struct MipTexel<MIP_F32> { typedef float4 T; };

/* Unit u of a level (units_x per row) -> its row and the unit within the row; 32-bit division while the index fits. */
__device__ inline void mip_unit_xy(size_t u, uint32_t units_x, uint32_t& ux, size_t& y)
{
	if (u <= 0xFFFFFFFFull)
	{
		const uint32_t q = (uint32_t)u / units_x;
		y = q; ux = (uint32_t)u - q * units_x;
	}
	else
	{
		y = u / units_x; ux = (uint32_t)(u - y * units_x);
	}
}

/* The float channels of a stored texel, and back. */
template <int K> __device__ inline void mip_unpack(const typename MipTexel<K>::T& t, float v[4]);
template <> __device__ inline void mip_unpack<MIP_F16>(const uint2& t, float v[4])
{
	v[0] = mip_float_from_half((unsigned short)(t.x & 0xFFFFu)); v[1] = mip_float_from_half((unsigned short)(t.x >> 16));
	v[2] = mip_float_from_half((unsigned short)(t.y & 0xFFFFu)); v[3] = mip_float_from_half((unsigned short)(t.y >> 16));
}
template <> __device__ inline void mip_unpack<MIP_F32>(const float4& t, float v[4]) { v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
__device__ inline uint2 mip_pack_f16(const float v[4])
{
	return make_uint2((uint32_t)mip_half_from_float(v[0]) | ((uint32_t)mip_half_from_float(v[1]) << 16),
	                  (uint32_t)mip_half_from_float(v[2]) | ((uint32_t)mip_half_from_float(v[3]) << 16));
}

/* A source texel from global memory with the loads the compressor uses on a caller's image (wave_load.h): one dword for RGBA8,
 * component loads otherwise, so a source needs only the alignment of its components. */
template <int K> __device__ inline typename MipTexel<K>::T mip_load_global(const void* src, size_t i);
template <> __device__ inline uint32_t mip_load_global<MIP_U8>(const void* src, size_t i) { return static_cast<const uint32_t*>(src)[i]; }
template <> __device__ inline uint32_t mip_load_global<MIP_U8_SRGB>(const void* src, size_t i) { return static_cast<const uint32_t*>(src)[i]; }
template <> __device__ inline uint2 mip_load_global<MIP_F16>(const void* src, size_t i)
{
	const uint16_t* p = static_cast<const uint16_t*>(src) + 4 * i;
	return make_uint2((uint32_t)p[0] | ((uint32_t)p[1] << 16), (uint32_t)p[2] | ((uint32_t)p[3] << 16));
}
template <> __device__ inline float4 mip_load_global<MIP_F32>(const void* src, size_t i)
{
	const float* p = static_cast<const float*>(src) + 4 * i;
	return make_float4(p[0], p[1], p[2], p[3]);
}

/* Row r of a layered level (rows_per_layer rows per layer) -> its layer and its row within the layer. */
__device__ inline void mip_row_layer(size_t r, uint32_t rows_per_layer, size_t& layer, uint32_t& y)
{
	if (r <= 0xFFFFFFFFull)
	{
		const uint32_t q = (uint32_t)r / rows_per_layer;
		layer = q; y = (uint32_t)r - q * rows_per_layer;
	}
	else
	{
		layer = r / rows_per_layer; y = (uint32_t)(r - layer * rows_per_layer);
	}
}

/* The arguments of the tail kernels: level k + 1 of the rest of the chain goes to dst[k]. */
struct MipTailArgs {
	const void* src;
	uint32_t sx, sy, levels;
	uint8_t* dst[MIP_MAX_LEVELS];
};

struct Mip3dTailArgs {
	const void* src;
	uint32_t sx, sy, sz, levels;
	uint8_t* dst[MIP_MAX_LEVELS];
};

/* The six kernels of one kind of data: 2D even / any level / tail, and their volume forms. */
struct MipKernels {
	void (*even)(const uint8_t*, size_t, uint8_t*, size_t, uint32_t, size_t, const double*);
	void (*level)(const void*, uint32_t, uint32_t, uint8_t*, uint32_t, uint32_t, uint32_t, size_t, const double*);
	void (*tail)(MipTailArgs, uint32_t, const double*);
	void (*even3d)(const uint8_t*, size_t, uint32_t, uint8_t*, size_t, uint32_t, uint32_t, size_t, const double*);
	void (*level3d)(const void*, uint32_t, uint32_t, uint32_t, uint8_t*, uint32_t, uint32_t, uint32_t, size_t, const double*);
	void (*tail3d)(Mip3dTailArgs, const double*);
};

/* Queues levels 1 .. n-1 of `job`, its texels of kind K, with the kernels `ks`. */
template <int K>
static int mip_launch_chain(const MipChainJob& job, const double* srgb, hipStream_t stream, const MipKernels& ks)
{
	typedef typename MipTexel<K>::T T;
	uint8_t* level_at[MIP_MAX_LEVELS];      // (level 0 is only read)
	level_at[0] = static_cast<uint8_t*>(const_cast<void*>(job.device_image));
	for (uint32_t i = 1; i < job.level_count; i++) level_at[i] = job.device_levels + job.texels_offset[i];
	const bool volume = job.kind == 1;
	uint32_t sx = job.dim_x, sy = job.dim_y, sz = job.dim_z;
	for (uint32_t level = 1; level < job.level_count; level++)
	{
		const void* src = level_at[level - 1];
		const uint32_t dx = sx > 1 ? sx >> 1 : 1u, dy = sy > 1 ? sy >> 1 : 1u;
		uint8_t* dst = level_at[level];
		const size_t src_pitch = (size_t)sx * sizeof(T);
		const bool aligned = (src_pitch & 31u) == 0 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
		if (volume && sz > 1)
		{
			const uint32_t dz = sz >> 1;
			if ((size_t)sx * sy * sz <= MIP_TAIL_TEXELS)
			{
				Mip3dTailArgs a;
				memset(&a, 0, sizeof(a));
				a.src = src; a.sx = sx; a.sy = sy; a.sz = sz; a.levels = job.level_count - level;
				for (uint32_t k = 0; k < a.levels; k++) a.dst[k] = level_at[level + k];
				hipLaunchKernelGGL(ks.tail3d, dim3(1), dim3(MIP_TAIL_THREADS), 0, stream, a, srgb);
				break;
			}
			const bool even = (sx & 1u) == 0 && (sy & 1u) == 0 && (sz & 1u) == 0 && aligned;
			const uint32_t units_x = even ? (uint32_t)(src_pitch / 32) : (uint32_t)((dx + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
			const size_t units = (size_t)units_x * dy * dz;
			size_t groups = (units + MIP_THREADS - 1) / MIP_THREADS;
			if (groups > MIP_MAX_GROUPS) groups = MIP_MAX_GROUPS;
			if (even)
				hipLaunchKernelGGL(ks.even3d, dim3((uint32_t)groups), dim3(MIP_THREADS), 0, stream,
				                   static_cast<const uint8_t*>(src), src_pitch, sy, dst, (size_t)dx * sizeof(T), dy, units_x, units, srgb);
			else
				hipLaunchKernelGGL(ks.level3d, dim3((uint32_t)groups), dim3(MIP_THREADS), 0, stream,
				                   src, sx, sy, sz, dst, dx, dy, units_x, units, srgb);
			sx = dx; sy = dy; sz = dz;
			continue;
		}
		// 2D layers: the layers of an array, or one (a 2D image, a volume level of depth 1)
		const uint32_t layers = volume ? 1u : sz;
		if ((size_t)sx * sy <= MIP_TAIL_TEXELS)
		{
			MipTailArgs a;
			memset(&a, 0, sizeof(a));
			a.src = src; a.sx = sx; a.sy = sy; a.levels = job.level_count - level;
			for (uint32_t k = 0; k < a.levels; k++) a.dst[k] = level_at[level + k];
			const uint32_t groups = layers < MIP_MAX_GROUPS ? layers : MIP_MAX_GROUPS;
			hipLaunchKernelGGL(ks.tail, dim3(groups), dim3(MIP_TAIL_THREADS), 0, stream, a, layers, srgb);
			break;
		}
		// (even sizes: a layer is an even number of rows, so the rows of all layers pair up as those of one tall image)
		const bool even = (sx & 1u) == 0 && (sy & 1u) == 0 && aligned;
		const uint32_t units_x = even ? (uint32_t)(src_pitch / 32) : (uint32_t)((dx + 16 / sizeof(T) - 1) / (16 / sizeof(T)));
		const size_t units = (size_t)units_x * dy * layers;
		size_t groups = (units + MIP_THREADS - 1) / MIP_THREADS;
		if (groups > MIP_MAX_GROUPS) groups = MIP_MAX_GROUPS;
		if (even)
			hipLaunchKernelGGL(ks.even, dim3((uint32_t)groups), dim3(MIP_THREADS), 0, stream,
			                   static_cast<const uint8_t*>(src), src_pitch, dst, (size_t)dx * sizeof(T), units_x, units, srgb);
		else
			hipLaunchKernelGGL(ks.level, dim3((uint32_t)groups), dim3(MIP_THREADS), 0, stream,
			                   src, sx, sy, dst, dx, dy, units_x, units, srgb);
		sx = dx; sy = dy;
	}
	return (int)hipGetLastError();
}

} // namespace astcd
