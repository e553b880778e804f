// SPDX-License-Identifier: Apache-2.0
// What the windowed filters' kernels share (kernel_mip_filter.hip: the plain filter of mip_resample.h; kernel_mip_weighted.hip:
// the alpha-weighted one of mip_weighted.h; kernel_mip_cube.hip: both with MIP_EDGE_CUBE): the table of taps that
// astc_mip_filter_table_build makes, how a kernel reads it, the loads and stores of a texel, the tile's size and the launch
// rules of a chain.
#pragma once
#include "backend.h"
#include "mip_weighted.h"
#include <hip/hip_runtime.h>

namespace astcd {

namespace {   // (internal linkage, as these had inside kernel_mip_filter.hip: the inliner weighs them the same)

enum MipRsKind { MIP_RS_U8 = 0, MIP_RS_U8_SRGB = 1, MIP_RS_F16 = 2, MIP_RS_F32 = 3 };
constexpr uint32_t MIP_RS_TX = 32, MIP_RS_TY = 16;        // destination tile
constexpr uint32_t MIP_RS_THREADS = 256;
constexpr uint32_t MIP_RS_PER = MIP_RS_TX * MIP_RS_TY / MIP_RS_THREADS;   // destination texels per thread
constexpr uint32_t MIP_RSW_TX = 16;                         // the alpha-weighted tile's width (kernel_mip_weighted.hip)
static_assert(MIP_RSW_TX * MIP_RS_TY == MIP_RS_THREADS, "one destination texel per thread");
constexpr uint32_t MIP_RS_ROWS = 48;                      // source rows a tile's y taps may touch (checked on the host)
constexpr uint32_t MIP_RS_TAIL_TEXELS = 4096;
constexpr uint32_t MIP_RS_MAX_GROUPS = 1u << 20;
constexpr size_t MIP_RS_TABLE_MAX = (size_t)64 << 20;     // the library's scratch bound
constexpr size_t MIP_RS_ROW_BYTES = 16 + 8 * MIP_RESAMPLE_MAX_TAPS;

/* One axis of a level in the table: rows of taps, each { int64 first, uint32 count, uint32 0, double w[17] }.  rows == 1 (a
 * source of one texel, or an even one below 2^26 texels, where c = 2j + 1 exactly and every destination has the taps of j = 0
 * moved by 2j): destination j takes row 0 with first + 2j; otherwise row j. */
struct MipRsAxis {
	uint32_t s, d, rows, edge;
	uint64_t at;                  // byte offset of row 0 in the table
};

/* A level: made from `src` (sx x sy x sz) into `dst` (dx x dy x dz); sz / dz are the layers of an ARRAY (array != 0: no z
 * filter, a layer reads its own slice) or a VOLUME's depths. */
struct MipRsLevel {
	const void* src;
	void* dst;
	uint32_t sx, sy, sz, dx, dy, dz;
	uint32_t array, tiles_x, tiles_y, pad;
	MipRsAxis ax[3];
};

struct MipRsTaps {
	long long first;
	uint32_t count;
	const double* w;
};

__device__ inline MipRsTaps mip_rs_taps(const uint8_t* table, const MipRsAxis& a, uint32_t j)
{
	const uint8_t* p = table + a.at + (a.rows == 1 ? 0 : (size_t)j * MIP_RS_ROW_BYTES);
	MipRsTaps t;
	t.first = *reinterpret_cast<const long long*>(p) + (a.rows == 1 ? 2ll * j : 0ll);
	t.count = *reinterpret_cast<const uint32_t*>(p + 8);
	t.w = reinterpret_cast<const double*>(p + 16);
	return t;
}

/* The values of source texel i (component loads: the caller's level 0 needs only the alignment of its components). */
template <int K>
__device__ inline void mip_rs_load(const void* src, size_t i, const double* lin, double v[4])
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		mip_resample_load_u8(static_cast<const uint32_t*>(src)[i], K == MIP_RS_U8_SRGB ? lin : nullptr, v);
	else if constexpr (K == MIP_RS_F16)
	{
		const uint16_t* p = static_cast<const uint16_t*>(src) + 4 * i;
		const float f[4] = { mip_float_from_half(p[0]), mip_float_from_half(p[1]), mip_float_from_half(p[2]), mip_float_from_half(p[3]) };
		mip_resample_load_float(f, v);
	}
	else
	{
		const float* p = static_cast<const float*>(src) + 4 * i;
		const float f[4] = { p[0], p[1], p[2], p[3] };
		mip_resample_load_float(f, v);
	}
}

template <int K>
__device__ inline void mip_rs_store(void* dst, size_t i, const double vol[4], const double* thr)
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		static_cast<uint32_t*>(dst)[i] = mip_resample_out_u8(vol, K == MIP_RS_U8_SRGB ? thr : nullptr);
	else
	{
		float f[4];
		mip_resample_out_float(vol, f);
		if constexpr (K == MIP_RS_F16)
			static_cast<uint2*>(dst)[i] = make_uint2((uint32_t)mip_half_from_float(f[0]) | ((uint32_t)mip_half_from_float(f[1]) << 16),
			                                         (uint32_t)mip_half_from_float(f[2]) | ((uint32_t)mip_half_from_float(f[3]) << 16));
		else
			static_cast<float4*>(dst)[i] = make_float4(f[0], f[1], f[2], f[3]);
	}
}

/* ... and with the seven values of the alpha-weighted filter (mip_weighted.h). */
template <int K>
__device__ inline void mip_rsw_load(const void* src, size_t i, const double* lin, double v[7])
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		mip_resample_load_u8_weighted(static_cast<const uint32_t*>(src)[i], K == MIP_RS_U8_SRGB ? lin : nullptr, v);
	else if constexpr (K == MIP_RS_F16)
	{
		const uint16_t* p = static_cast<const uint16_t*>(src) + 4 * i;
		const float f[4] = { mip_float_from_half(p[0]), mip_float_from_half(p[1]), mip_float_from_half(p[2]), mip_float_from_half(p[3]) };
		mip_resample_load_float_weighted(f, v);
	}
	else
	{
		const float* p = static_cast<const float*>(src) + 4 * i;
		const float f[4] = { p[0], p[1], p[2], p[3] };
		mip_resample_load_float_weighted(f, v);
	}
}

template <int K>
__device__ inline void mip_rsw_store(void* dst, size_t i, const double vol[7], const double* thr)
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		static_cast<uint32_t*>(dst)[i] = mip_resample_out_u8_weighted(vol, K == MIP_RS_U8_SRGB ? thr : nullptr);
	else
	{
		float f[4];
		mip_resample_out_float_weighted(vol, f);
		if constexpr (K == MIP_RS_F16)
			static_cast<uint2*>(dst)[i] = make_uint2((uint32_t)mip_half_from_float(f[0]) | ((uint32_t)mip_half_from_float(f[1]) << 16),
			                                         (uint32_t)mip_half_from_float(f[2]) | ((uint32_t)mip_half_from_float(f[3]) << 16));
		else
			static_cast<float4*>(dst)[i] = make_float4(f[0], f[1], f[2], f[3]);
	}
}

/* Queues levels 1 .. n-1 of `job` from the table's device copy: `level` per large level, over tiles tile_x wide, then `tail` for
 * the rest of the chain. */
static int mip_rs_launch_chain(const MipChainJob& job, const uint8_t* d_table, const double* srgb, hipStream_t stream,
                               void (*tail)(const uint8_t*, uint32_t, uint32_t, uint32_t, const double*),
                               void (*level)(const uint8_t*, uint32_t, const double*), uint32_t tile_x)
{
	const bool volume = job.kind == 1;
	const uint32_t layers = volume ? 1u : job.dim_z;
	for (uint32_t i = 1; i < job.level_count; i++)
	{
		const uint32_t sx = mip_level_dim(job.dim_x, i - 1), sy = mip_level_dim(job.dim_y, i - 1);
		const uint32_t sz = volume ? mip_level_dim(job.dim_z, i - 1) : 1u;
		if ((size_t)sx * sy * sz <= MIP_RS_TAIL_TEXELS)
		{
			const uint32_t groups = layers < MIP_RS_MAX_GROUPS ? layers : MIP_RS_MAX_GROUPS;
			hipLaunchKernelGGL(tail, dim3(groups), dim3(MIP_RS_THREADS), 0, stream, d_table, i - 1, job.level_count - 1,
			                   layers, srgb);
			break;
		}
		const uint32_t dx = mip_level_dim(job.dim_x, i), dy = mip_level_dim(job.dim_y, i);
		const uint32_t dz = volume ? mip_level_dim(job.dim_z, i) : job.dim_z;
		const size_t tiles = (size_t)((dx + tile_x - 1) / tile_x) * ((dy + MIP_RS_TY - 1) / MIP_RS_TY) * dz;
		const uint32_t groups = tiles < MIP_RS_MAX_GROUPS ? (uint32_t)tiles : MIP_RS_MAX_GROUPS;
		hipLaunchKernelGGL(level, dim3(groups), dim3(MIP_RS_THREADS), 0, stream, d_table, i - 1, srgb);
	}
	return (int)hipGetLastError();
}

} // namespace

} // namespace astcd
