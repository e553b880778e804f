// SPDX-License-Identifier: Apache-2.0
// Mip chain generation with the windowed filters and seamless cube-map edges (ASTCENC_AMD_MIP_EDGE_CUBE, include/astcenc_amd.h;
// mip_cube_source in mip_resample.h): a tap that leaves a face reads the neighbouring face of the same cube.  The kernels are
// the two shapes of kernel_mip_filter.hip over the same table of taps (mip_filter_kernels.h), plain and alpha-weighted, in a
// translation unit of their own so that the CLAMP / WRAP kernels keep their machine code:
//   - the tile is mip_rs_tile's (the weighted one mip_rsw_tile's) without a z filter: the x pass makes the row sums per (source
//     row, destination x), the y pass reads them from LDS.  A source row outside the face is a row or a column of a neighbour,
//     so only the address of a load changes; a tile whose taps all stay inside the face takes CLAMP's addresses;
//   - every level is one launch over the tiles of every face (astc_mipcube_level, astc_mipcubew_level).  There is no tail kernel:
//     a face reads four other layers of the level before, which astc_mipfilter_tail's one workgroup per layer would not have
//     written, and one workgroup per cube makes the six faces of each small level one after the other (measured: 0.75 ms for
//     the levels below 64^2 where CLAMP's tail takes 0.11 ms).  A launch per level keeps the faces side by side.
#include "mip_filter_kernels.h"

namespace astcd {

namespace {

template <bool W>
struct MipCubeShape {
	static constexpr uint32_t TX = W ? MIP_RSW_TX : MIP_RS_TX;                 // destination tile width
	static constexpr int N = W ? MIP_WEIGHTED_VALUES : 4;                      // float64 values per texel
	static constexpr uint32_t PER = TX * MIP_RS_TY / MIP_RS_THREADS;           // destination texels per thread
};

template <bool W>
struct MipCubeShared {
	double rows[MIP_RS_ROWS][MipCubeShape<W>::TX][MipCubeShape<W>::N];        // the x pass's row sums of the tile
	double srgb[MIP_SRGB_TABLE_DOUBLES];                                       // lin[256], then thr[255] (sRGB data only)
};

template <int N>
__device__ inline void mip_cube_accumulate(double sum[N], double w, const double v[N], uint32_t k)
{
	if constexpr (N == 4) mip_resample_accumulate(sum, w, v, k);
	else mip_resample_accumulate7(sum, w, v, k);
}

template <int K, int N>
__device__ inline void mip_cube_load(const void* src, size_t i, const double* lin, double v[N])
{
	if constexpr (N == 4) mip_rs_load<K>(src, i, lin, v);
	else mip_rsw_load<K>(src, i, lin, v);
}

template <int K, int N>
__device__ inline void mip_cube_store(void* dst, size_t i, const double vol[N], const double* thr)
{
	if constexpr (N == 4) mip_rs_store<K>(dst, i, vol, thr);
	else mip_rsw_store<K>(dst, i, vol, thr);
}

template <bool W>
__device__ inline uint32_t mip_cube_tiles_x(const MipRsLevel& L) { return (L.dx + MipCubeShape<W>::TX - 1) / MipCubeShape<W>::TX; }

/* Tile `tile` of level L (tiles in x, then y, then layer order; layer l is face l % 6 of cube l / 6, sx == sy).  Every thread
 * of the workgroup calls it (it has barriers). */
template <int K, bool W>
__device__ void mip_cube_tile(const uint8_t* table, const MipRsLevel& L, size_t tile, MipCubeShared<W>& sh)
{
	constexpr uint32_t TX = MipCubeShape<W>::TX, PER = MipCubeShape<W>::PER;
	constexpr int N = MipCubeShape<W>::N;
	const uint32_t tiles_x = mip_cube_tiles_x<W>(L), tiles_xy = tiles_x * L.tiles_y;
	const uint32_t layer = (uint32_t)(tile / tiles_xy), txy = (uint32_t)(tile - (size_t)layer * tiles_xy);
	const uint32_t ty_i = txy / tiles_x, tx_i = txy - ty_i * tiles_x;
	const uint32_t x0 = tx_i * TX, y0 = ty_i * MIP_RS_TY;
	const uint32_t xlast = (x0 + TX < L.dx ? x0 + TX : L.dx) - 1, ylast = (y0 + MIP_RS_TY < L.dy ? y0 + MIP_RS_TY : L.dy) - 1;
	const MipRsTaps tx_lo = mip_rs_taps(table, L.ax[0], x0), tx_hi = mip_rs_taps(table, L.ax[0], xlast);
	const MipRsTaps ty_lo = mip_rs_taps(table, L.ax[1], y0), ty_hi = mip_rs_taps(table, L.ax[1], ylast);
	const long long ylo = ty_lo.first, s = (long long)L.sx;
	const uint32_t nrows = (uint32_t)(ty_hi.first + ty_hi.count - ylo);
	// (the first tap index grows with the destination index: the tile's taps span [lo.first, hi.first + hi.count) on each axis)
	const bool inside = tx_lo.first >= 0 && tx_hi.first + tx_hi.count <= s && ylo >= 0 && ylo + nrows <= s;
	const uint32_t face = layer % 6u;
	const size_t cube0 = layer - face;                   // the cube's first layer
	const double* lin = K == MIP_RS_U8_SRGB ? sh.srgb : nullptr;

	// x pass: the row sums of every source row the tile's y taps touch, for the tile's destination columns
	for (uint32_t item = threadIdx.x; item < nrows * TX; item += MIP_RS_THREADS)
	{
		const uint32_t r = item / TX, c = item % TX, x = x0 + c;
		if (x >= L.dx) continue;
		const long long iy = ylo + r;
		const MipRsTaps tx = mip_rs_taps(table, L.ax[0], x);
		double sum[N] = {};
		if (inside)
		{
			const size_t base = ((size_t)layer * L.sy + (size_t)iy) * L.sx + (size_t)tx.first;
			for (uint32_t k = 0; k < tx.count; k++)
			{
				double v[N];
				mip_cube_load<K, N>(L.src, base + k, lin, v);
				mip_cube_accumulate<N>(sum, tx.w[k], v, k);
			}
		}
		else
		{
			for (uint32_t k = 0; k < tx.count; k++)
			{
				const MipCubeTexel t = mip_cube_source(face, tx.first + k, iy, L.sx);
				double v[N];
				mip_cube_load<K, N>(L.src, ((cube0 + t.face) * L.sy + t.y) * L.sx + t.x, lin, v);
				mip_cube_accumulate<N>(sum, tx.w[k], v, k);
			}
		}
		for (int ch = 0; ch < N; ch++) sh.rows[r][c][ch] = sum[ch];
	}
	__syncthreads();
	// y pass from LDS; an ARRAY has no z filter: vol = 1.0 * acc
	#pragma unroll
	for (uint32_t q = 0; q < PER; q++)
	{
		const uint32_t p = threadIdx.x + q * MIP_RS_THREADS, c = p % TX, x = x0 + c, y = y0 + p / TX;
		if (x >= L.dx || y >= L.dy) continue;
		const MipRsTaps ty = mip_rs_taps(table, L.ax[1], y);
		double acc[N] = {};
		for (uint32_t k = 0; k < ty.count; k++)
		{
			const uint32_t r = (uint32_t)(ty.first + k - ylo);
			double row[N];
			for (int ch = 0; ch < N; ch++) row[ch] = sh.rows[r][c][ch];
			mip_cube_accumulate<N>(acc, ty.w[k], row, k);
		}
		double vol[N] = {};
		mip_cube_accumulate<N>(vol, 1.0, acc, 0);
		mip_cube_store<K, N>(L.dst, ((size_t)layer * L.dy + y) * L.dx + x, vol, sh.srgb + 256);
	}
	__syncthreads();
}

template <int K, bool W>
__device__ inline void mip_cube_srgb_to_lds(const double* srgb, MipCubeShared<W>& sh)
{
	if constexpr (K == MIP_RS_U8_SRGB)
		for (uint32_t i = threadIdx.x; i < MIP_SRGB_TABLE_DOUBLES; i += MIP_RS_THREADS) sh.srgb[i] = srgb[i];
	__syncthreads();
}

/* One level (table entry `level`): a grid-stride loop over the tiles of every face. */
template <int K, bool W>
__device__ inline void mip_cube_level(const uint8_t* table, uint32_t level, const double* srgb, MipCubeShared<W>& sh)
{
	mip_cube_srgb_to_lds<K, W>(srgb, sh);
	const MipRsLevel& L = reinterpret_cast<const MipRsLevel*>(table)[level];
	const size_t tiles = (size_t)mip_cube_tiles_x<W>(L) * L.tiles_y * L.dz;
	for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) mip_cube_tile<K, W>(table, L, t, sh);
}

} // namespace

template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipcube_level(const uint8_t* table, uint32_t level, const double* srgb)
{
	__shared__ MipCubeShared<false> sh;
	mip_cube_level<K, false>(table, level, srgb, sh);
}

/* ... with alpha-weighted colour (mip_weighted.h): seven sums per texel in the 16 wide tile of kernel_mip_weighted.hip. */
template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipcubew_level(const uint8_t* table, uint32_t level, const double* srgb)
{
	__shared__ MipCubeShared<true> sh;
	mip_cube_level<K, true>(table, level, srgb, sh);
}

/* Queues levels 1 .. n-1 of `job` (an ARRAY of square layers, six to a cube: checked by the caller), one launch each. */
template <int K, bool W>
static int mip_cube_launch_kind(const MipChainJob& job, const uint8_t* d_table, const double* srgb, hipStream_t stream)
{
	constexpr uint32_t TX = MipCubeShape<W>::TX;
	for (uint32_t i = 1; i < job.level_count; i++)
	{
		const uint32_t d = mip_level_dim(job.dim_x, i);
		const size_t tiles = (size_t)((d + TX - 1) / TX) * ((d + MIP_RS_TY - 1) / MIP_RS_TY) * job.dim_z;
		const uint32_t groups = tiles < MIP_RS_MAX_GROUPS ? (uint32_t)tiles : MIP_RS_MAX_GROUPS;
		hipLaunchKernelGGL((W ? astc_mipcubew_level<K> : astc_mipcube_level<K>), dim3(groups), dim3(MIP_RS_THREADS), 0, stream, d_table,
		                   i - 1, srgb);
	}
	return (int)hipGetLastError();
}

template <bool W>
static int mip_cube_launch_type(const MipChainJob& job, const uint8_t* t, const double* srgb, hipStream_t s)
{
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? mip_cube_launch_kind<MIP_RS_U8_SRGB, W>(job, t, srgb, s) : mip_cube_launch_kind<MIP_RS_U8, W>(job, t, srgb, s);
	case 1: return mip_cube_launch_kind<MIP_RS_F16, W>(job, t, srgb, s);
	default: return mip_cube_launch_kind<MIP_RS_F32, W>(job, t, srgb, s);
	}
}

int astc_mip_cube_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream)
{
	if (job.level_count < 2) return 0;
	const uint8_t* t = static_cast<const uint8_t*>(d_table);
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	return job.weight ? mip_cube_launch_type<true>(job, t, srgb, s) : mip_cube_launch_type<false>(job, t, srgb, s);
}

} // namespace astcd
