// SPDX-License-Identifier: Apache-2.0
// Mip chain generation with the windowed filters (astcenc_amd_generate_mip_chain_filtered_device, mip_resample.h): MITCHELL,
// LANCZOS3 and KAISER.  The host builds the taps of every level's axes once per call (astc_mip_filter_table_build) and the
// kernels only multiply and add them in float64:
//   - a workgroup makes a tile of MIP_RS_TX x MIP_RS_TY destination texels of one slice (a VOLUME's z, an ARRAY's layer).  Per
//     z tap it runs the x pass once per source row that the tile's y taps touch -- row sums depend only on (source row,
//     destination x), so sharing them between the tile's texels changes no bit -- keeps them in LDS as float64, and runs the
//     y pass from there; vol accumulates in registers over the z taps;
//   - a large level is one launch (astc_mipfilter_level), a grid-stride loop over its tiles;
//   - once a source level has at most MIP_RS_TAIL_TEXELS texels (per layer for an ARRAY), one workgroup per layer makes every
//     remaining level (astc_mipfilter_tail), each level read back from global memory after a barrier.
// The box filter keeps its own kernels (kernel_mips.hip); nothing here runs for it.
#include "mip_filter_kernels.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace astcd {

namespace {

struct MipRsShared {
	double rows[MIP_RS_ROWS][MIP_RS_TX][4];                 // the x pass's row sums of the tile
	double srgb[MIP_SRGB_TABLE_DOUBLES];                    // lin[256], then thr[255] (sRGB data only)
};

/* Tile `tile` of level L (tiles in x, then y, then slice order).  Every thread of the workgroup calls it (it has barriers). */
template <int K>
__device__ void mip_rs_tile(const uint8_t* table, const MipRsLevel& L, size_t tile, MipRsShared& sh)
{
	const uint32_t tiles_xy = L.tiles_x * L.tiles_y;
	const uint32_t slice = (uint32_t)(tile / tiles_xy), txy = (uint32_t)(tile - (size_t)slice * tiles_xy);
	const uint32_t ty_i = txy / L.tiles_x, tx_i = txy - ty_i * L.tiles_x;
	const uint32_t x0 = tx_i * MIP_RS_TX, y0 = ty_i * MIP_RS_TY;
	const uint32_t ylast = (y0 + MIP_RS_TY < L.dy ? y0 + MIP_RS_TY : L.dy) - 1;
	const MipRsTaps t_lo = mip_rs_taps(table, L.ax[1], y0), t_hi = mip_rs_taps(table, L.ax[1], ylast);
	const long long ylo = t_lo.first;
	const uint32_t nrows = (uint32_t)(t_hi.first + t_hi.count - ylo);
	const MipRsTaps tz = L.array ? MipRsTaps{ (long long)slice, 1u, nullptr } : mip_rs_taps(table, L.ax[2], slice);
	const double* lin = K == MIP_RS_U8_SRGB ? sh.srgb : nullptr;

	double vol[MIP_RS_PER][4] = {};
	for (uint32_t kz = 0; kz < tz.count; kz++)
	{
		const uint32_t zs = L.array ? slice : mip_resample_source(tz.first + kz, L.sz, L.ax[2].edge);
		const double wz = L.array ? 1.0 : tz.w[kz];
		// x pass: the row sums of every source row the tile's y taps touch, for the tile's destination columns
		for (uint32_t item = threadIdx.x; item < nrows * MIP_RS_TX; item += MIP_RS_THREADS)
		{
			const uint32_t r = item / MIP_RS_TX, c = item % MIP_RS_TX, x = x0 + c;
			if (x >= L.dx) continue;
			const uint32_t ys = mip_resample_source(ylo + r, L.sy, L.ax[1].edge);
			const MipRsTaps tx = mip_rs_taps(table, L.ax[0], x);
			const size_t base = ((size_t)zs * L.sy + ys) * L.sx;
			double sum[4] = { 0.0, 0.0, 0.0, 0.0 };
			for (uint32_t k = 0; k < tx.count; k++)
			{
				double v[4];
				mip_rs_load<K>(L.src, base + mip_resample_source(tx.first + k, L.sx, L.ax[0].edge), lin, v);
				mip_resample_accumulate(sum, tx.w[k], v, k);
			}
			for (int ch = 0; ch < 4; ch++) sh.rows[r][c][ch] = sum[ch];
		}
		__syncthreads();
		// y pass from LDS, then this z tap's share of vol
		#pragma unroll
		for (uint32_t q = 0; q < MIP_RS_PER; q++)
		{
			const uint32_t p = threadIdx.x + q * MIP_RS_THREADS, c = p % MIP_RS_TX, x = x0 + c, y = y0 + p / MIP_RS_TX;
			if (x >= L.dx || y >= L.dy) continue;
			const MipRsTaps ty = mip_rs_taps(table, L.ax[1], y);
			double acc[4] = { 0.0, 0.0, 0.0, 0.0 };
			for (uint32_t k = 0; k < ty.count; k++)
			{
				const uint32_t r = (uint32_t)(ty.first + k - ylo);
				const double row[4] = { sh.rows[r][c][0], sh.rows[r][c][1], sh.rows[r][c][2], sh.rows[r][c][3] };
				mip_resample_accumulate(acc, ty.w[k], row, k);
			}
			mip_resample_accumulate(vol[q], wz, acc, kz);
		}
		__syncthreads();
	}
	#pragma unroll
	for (uint32_t q = 0; q < MIP_RS_PER; q++)
	{
		const uint32_t p = threadIdx.x + q * MIP_RS_THREADS, x = x0 + p % MIP_RS_TX, y = y0 + p / MIP_RS_TX;
		if (x >= L.dx || y >= L.dy) continue;
		mip_rs_store<K>(L.dst, ((size_t)slice * L.dy + y) * L.dx + x, vol[q], sh.srgb + 256);
	}
}

template <int K>
__device__ inline void mip_rs_srgb_to_lds(const double* srgb, MipRsShared& sh)
{
	if constexpr (K == MIP_RS_U8_SRGB)
		for (uint32_t i = threadIdx.x; i < MIP_SRGB_TABLE_DOUBLES; i += MIP_RS_THREADS) sh.srgb[i] = srgb[i];
	__syncthreads();
}

} // namespace

/* One level (table entry `level`): a grid-stride loop over its tiles. */
template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipfilter_level(const uint8_t* table, uint32_t level, const double* srgb)
{
	__shared__ MipRsShared sh;
	mip_rs_srgb_to_lds<K>(srgb, sh);
	const MipRsLevel& L = reinterpret_cast<const MipRsLevel*>(table)[level];
	const size_t tiles = (size_t)L.tiles_x * L.tiles_y * L.dz;
	for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) mip_rs_tile<K>(table, L, t, sh);
}

/* Table entries first .. levels - 1 in one workgroup per layer (an ARRAY's; one for a VOLUME): every tile of a level, a barrier,
 * then the next level, which reads the one just written. */
template <int K>
__global__ void __launch_bounds__(MIP_RS_THREADS)
astc_mipfilter_tail(const uint8_t* table, uint32_t first, uint32_t levels, uint32_t layers, const double* srgb)
{
	__shared__ MipRsShared sh;
	mip_rs_srgb_to_lds<K>(srgb, sh);
	for (uint32_t layer = blockIdx.x; layer < layers; layer += gridDim.x)
		for (uint32_t lv = first; lv < levels; lv++)
		{
			const MipRsLevel L = reinterpret_cast<const MipRsLevel*>(table)[lv];
			const size_t per = (size_t)L.tiles_x * L.tiles_y;
			const size_t t0 = L.array ? (size_t)layer * per : 0, t1 = L.array ? t0 + per : per * L.dz;
			for (size_t t = t0; t < t1; t++) mip_rs_tile<K>(table, L, t, sh);
			__syncthreads();
		}
}

/* The table of a job: the MipRsLevel of levels 1 .. n-1 (entry i - 1 makes level i), then the rows of their axes.  0: built;
 * 1: above MIP_RS_TABLE_MAX; 2: a tile would touch more than MIP_RS_ROWS source rows (not expected: the bound holds for every
 * axis, tests/test_mip_filter_cpu.py). */
int astc_mip_filter_table_build(const MipChainJob& job, std::vector<uint8_t>& out)
{
	const uint32_t n = job.level_count;
	const bool volume = job.kind == 1;
	auto rows_of = [](uint32_t s) -> uint32_t { return s <= 1 || ((s & 1u) == 0 && s < (1u << 26)) ? 1u : s >> 1; };
	// sizes first: nothing is built for a table that is refused
	size_t bytes = (size_t)(n - 1) * sizeof(MipRsLevel);
	for (uint32_t i = 1; i < n; i++)
	{
		const uint32_t s[3] = { mip_level_dim(job.dim_x, i - 1), mip_level_dim(job.dim_y, i - 1), volume ? mip_level_dim(job.dim_z, i - 1) : 1u };
		for (int a = 0; a < (volume ? 3 : 2); a++)
		{
			bytes += (size_t)rows_of(s[a]) * MIP_RS_ROW_BYTES;
			if (bytes > MIP_RS_TABLE_MAX) return 1;
		}
	}
	out.assign(bytes, 0);
	const auto sin_fn = [](double x) { return ::sin(x); };
	size_t at = (size_t)(n - 1) * sizeof(MipRsLevel);
	for (uint32_t i = 1; i < n; i++)
	{
		MipRsLevel L;
		memset(&L, 0, sizeof(L));
		L.src = i == 1 ? job.device_image : job.device_levels + job.texels_offset[i - 1];
		L.dst = job.device_levels + job.texels_offset[i];
		L.sx = mip_level_dim(job.dim_x, i - 1); L.sy = mip_level_dim(job.dim_y, i - 1);
		L.dx = mip_level_dim(job.dim_x, i); L.dy = mip_level_dim(job.dim_y, i);
		L.sz = volume ? mip_level_dim(job.dim_z, i - 1) : job.dim_z;
		L.dz = volume ? mip_level_dim(job.dim_z, i) : job.dim_z;
		L.array = volume ? 0u : 1u;
		L.tiles_x = (L.dx + MIP_RS_TX - 1) / MIP_RS_TX; L.tiles_y = (L.dy + MIP_RS_TY - 1) / MIP_RS_TY;
		const uint32_t s[3] = { L.sx, L.sy, volume ? L.sz : 1u };
		for (int a = 0; a < (volume ? 3 : 2); a++)
		{
			MipRsAxis& ax = L.ax[a];
			ax.s = s[a]; ax.d = s[a] > 1 ? s[a] >> 1 : 1u; ax.rows = rows_of(s[a]); ax.edge = job.filter_edge; ax.at = at;
			for (uint32_t j = 0; j < ax.rows; j++)
			{
				uint8_t* row = out.data() + at + (size_t)j * MIP_RS_ROW_BYTES;
				long long first;
				double w[MIP_RESAMPLE_MAX_TAPS];
				const uint32_t count = mip_resample_taps((int)job.filter_kind, ax.s, j, sin_fn, &first, w);
				memcpy(row, &first, 8);
				memcpy(row + 8, &count, 4);
				memcpy(row + 16, w, (size_t)count * 8);
			}
			at += (size_t)ax.rows * MIP_RS_ROW_BYTES;
		}
		// the source rows of every tile's y taps must fit the LDS rows
		auto taps_y = [&](uint32_t y, long long& first) {
			const uint8_t* row = out.data() + L.ax[1].at + (L.ax[1].rows == 1 ? 0 : (size_t)y * MIP_RS_ROW_BYTES);
			uint32_t count;
			memcpy(&first, row, 8); memcpy(&count, row + 8, 4);
			if (L.ax[1].rows == 1) first += 2ll * y;
			return count;
		};
		for (uint32_t y0 = 0; y0 < L.dy; y0 += MIP_RS_TY)
		{
			const uint32_t ylast = (y0 + MIP_RS_TY < L.dy ? y0 + MIP_RS_TY : L.dy) - 1;
			long long lo, hi;
			taps_y(y0, lo);
			const uint32_t count = taps_y(ylast, hi);
			if (hi + count - lo > (long long)MIP_RS_ROWS) return 2;
			if (L.ax[1].rows == 1) break;      // (every tile alike but a short last one)
		}
		memcpy(out.data() + (size_t)(i - 1) * sizeof(MipRsLevel), &L, sizeof(L));
	}
	return 0;
}

template <int K>
static int mip_filter_launch_kind(const MipChainJob& job, const uint8_t* d_table, const double* srgb, hipStream_t stream)
{
	// (the tail is named first: the kernels are instantiated in the order they are named, and the inliner's choices follow it)
	return mip_rs_launch_chain(job, d_table, srgb, stream, astc_mipfilter_tail<K>, astc_mipfilter_level<K>, MIP_RS_TX);
}

int astc_mip_filter_launch(const MipChainJob& job, const void* d_table, const void* d_srgb, void* stream)
{
	if (job.level_count < 2) return 0;
	const uint8_t* t = static_cast<const uint8_t*>(d_table);
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? mip_filter_launch_kind<MIP_RS_U8_SRGB>(job, t, srgb, s) : mip_filter_launch_kind<MIP_RS_U8>(job, t, srgb, s);
	case 1: return mip_filter_launch_kind<MIP_RS_F16>(job, t, srgb, s);
	default: return mip_filter_launch_kind<MIP_RS_F32>(job, t, srgb, s);
	}
}

} // namespace astcd
