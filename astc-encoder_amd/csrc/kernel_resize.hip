// SPDX-License-Identifier: Apache-2.0
// Resizing a device image to any size (astcenc_amd_resize_image_device, mip_resize.h): the box and the windowed filters of the
// mip chain at a general ratio per axis, plain or alpha-weighted.  The chain's kernels are built for halving (17 weights to a
// row, one shared row per even axis, at most 48 source rows under a tile); these assume nothing about the ratio
// (DESIGN.md section 3.6):
//   - the host builds the taps once per call (astc_resize_table_build): per axis a list of rows { first, count, offset }
//     into a pool of float64 weights, one row per destination texel or, where the arithmetic is periodic
//     (mip_resize_period), one period of them;
//   - a workgroup makes a tile of destination texels of one slice.  Per z tap it walks the index range of the tile's y taps in
//     chunks of RESIZE_ROWS source rows: the x pass fills the chunk's row sums in LDS, then every thread adds, in increasing
//     tap order, the taps of its texels that fall into the chunk.  A sum in increasing tap order does not depend on where the
//     chunk boundaries are, so any ratio gives the bits of mip_resize_texel;
//   - vol accumulates in registers over the z taps, as in astc_mipfilter_level.
// A value is a 64-bit slot: float64, or for the box filter on U8 data the exact integers of mip_filter.h.
#include "mip_filter_kernels.h"
#include "mip_resize.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace astcd {

namespace {

constexpr uint32_t RESIZE_TY = 16;                        // the tile's height; its width: 32 plain (two texels to a thread),
constexpr uint32_t RESIZE_THREADS = 256;                  // 16 weighted (one)
constexpr uint32_t RESIZE_ROWS = 48;                      // source rows of a chunk
constexpr uint32_t RESIZE_MAX_GROUPS = 1u << 20;
constexpr size_t RESIZE_TABLE_MAX = (size_t)64 << 20;     // the library's scratch bound

/* A row of an axis: the taps first .. first + count - 1, their weights at pool[at .. at + count). */
struct ResizeRow {
	long long first;
	uint32_t count, at;
};

/* An axis: destination j takes row j mod period with first + (j / period) * shift (mip_resize_period). */
struct ResizeAxis {
	uint32_t s, d, period, shift, edge;
	uint32_t rows_at, pool_at;    // byte offsets in the table (which stays below 64 MiB)
};

/* The head of the table. */
struct ResizeDesc {
	const void* src;
	void* dst;
	uint32_t dz, array, tiles_x, tiles_y;
	uint64_t den;                 // den_x * den_y * den_z of the box
	double dden;                  // ((double)den_x * (double)den_y) * (double)den_z
	ResizeAxis ax[3];
};
constexpr size_t RESIZE_HEAD = 256;
static_assert(sizeof(ResizeDesc) <= RESIZE_HEAD, "the head holds the description");

struct ResizeTaps {
	long long first;
	uint32_t count;
	const double* w;
};

__device__ inline ResizeTaps resize_taps(const uint8_t* table, const ResizeAxis& a, uint32_t j)
{
	uint32_t q, r;
	if (a.period == 1) { q = j; r = 0; }
	else if (a.period == a.d) { q = 0; r = j; }
	else { q = j / a.period; r = j - q * a.period; }
	const ResizeRow row = reinterpret_cast<const ResizeRow*>(table + a.rows_at)[r];
	ResizeTaps t;
	t.first = row.first + (long long)q * a.shift;
	t.count = row.count;
	t.w = reinterpret_cast<const double*>(table + a.pool_at) + row.at;
	return t;
}

template <int K, int N, unsigned int INTS>
__device__ inline void resize_load(const void* src, size_t i, const double* lin, MipResizeSlot v[N])
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		mip_resize_load_u8<N, INTS>(static_cast<const uint32_t*>(src)[i], K == MIP_RS_U8_SRGB ? lin : nullptr, v);
	else if constexpr (K == MIP_RS_F16)
	{
		const uint16_t* p = static_cast<const uint16_t*>(src) + 4 * i;
		const float f[4] = { mip_float_from_half(p[0]), mip_float_from_half(p[1]), mip_float_from_half(p[2]), mip_float_from_half(p[3]) };
		mip_resize_load_float<N>(f, v);
	}
	else
	{
		const float* p = static_cast<const float*>(src) + 4 * i;
		const float f[4] = { p[0], p[1], p[2], p[3] };
		mip_resize_load_float<N>(f, v);
	}
}

template <int K, int N, bool BOX>
__device__ inline void resize_store(void* dst, size_t i, const MipResizeSlot vol[N], const double* thr, uint64_t den, double dden)
{
	if constexpr (K == MIP_RS_U8 || K == MIP_RS_U8_SRGB)
		static_cast<uint32_t*>(dst)[i] = mip_resize_out_u8<N, BOX>(vol, K == MIP_RS_U8_SRGB ? thr : nullptr, den, dden);
	else
	{
		float f[4];
		mip_resize_out_float<N, BOX>(vol, dden, f);
		if constexpr (K == MIP_RS_F16)
			static_cast<uint2*>(dst)[i] = make_uint2((uint32_t)mip_half_from_float(f[0]) | ((uint32_t)mip_half_from_float(f[1]) << 16),
			                                         (uint32_t)mip_half_from_float(f[2]) | ((uint32_t)mip_half_from_float(f[3]) << 16));
		else
			static_cast<float4*>(dst)[i] = make_float4(f[0], f[1], f[2], f[3]);
	}
}

template <int N, uint32_t TX>
struct ResizeShared {
	MipResizeSlot rows[RESIZE_ROWS][TX][N];                 // the x pass's row sums of a chunk
	double srgb[MIP_SRGB_TABLE_DOUBLES];                    // lin[256], then thr[255] (sRGB data only)
};

} // namespace

/* K: MIP_RS_* (mip_filter_kernels.h); WEIGHTED: seven values to a texel (mip_weighted.h); BOX: the box's integers and division.
 * A grid-stride loop over the tiles (x, then y, then slice).  Inside a tile the y taps are counted from the tile's first
 * source row (the table.s bound keeps a tile.s span far inside 32 bits). */
template <int K, bool WEIGHTED, bool BOX>
__global__ void __launch_bounds__(RESIZE_THREADS)
astc_resize_image(const uint8_t* __restrict__ table, const double* __restrict__ srgb)
{
	constexpr int N = WEIGHTED ? 7 : 4;
	constexpr uint32_t TX = WEIGHTED ? 16 : 32, PER = TX * RESIZE_TY / RESIZE_THREADS;
	constexpr unsigned int INTS = mip_resize_ints(K == MIP_RS_U8 ? MIP_RESIZE_U8 : K == MIP_RS_U8_SRGB ? MIP_RESIZE_U8_SRGB : MIP_RESIZE_FLOAT, BOX, WEIGHTED);
	__shared__ ResizeShared<N, TX> sh;
	if constexpr (K == MIP_RS_U8_SRGB)
		for (uint32_t i = threadIdx.x; i < MIP_SRGB_TABLE_DOUBLES; i += RESIZE_THREADS) sh.srgb[i] = srgb[i];
	__syncthreads();
	const double* lin = K == MIP_RS_U8_SRGB ? sh.srgb : nullptr;
	const ResizeDesc& D = *reinterpret_cast<const ResizeDesc*>(table);
	const uint32_t sx = D.ax[0].s, sy = D.ax[1].s, dx = D.ax[0].d, dy = D.ax[1].d;
	const uint32_t tiles_xy = D.tiles_x * D.tiles_y;
	const size_t tiles = (size_t)tiles_xy * D.dz;
	const uint32_t c = threadIdx.x % TX, row0 = threadIdx.x / TX;

	for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
	{
		const uint32_t slice = (uint32_t)(tile / tiles_xy), txy = (uint32_t)(tile - (size_t)slice * tiles_xy);
		const uint32_t ty_i = txy / D.tiles_x, tx_i = txy - ty_i * D.tiles_x;
		const uint32_t x0 = tx_i * TX, y0 = ty_i * RESIZE_TY, x = x0 + c;
		const uint32_t ylast = (y0 + RESIZE_TY < dy ? y0 + RESIZE_TY : dy) - 1;
		// (the first and the last tap of a destination do not decrease with it: the tile's rows are those from y0's first
		//  to ylast's last)
		const ResizeTaps t_lo = resize_taps(table, D.ax[1], y0), t_hi = resize_taps(table, D.ax[1], ylast);
		const long long ylo = t_lo.first;
		const uint32_t span = (uint32_t)(t_hi.first + t_hi.count - ylo);
		const ResizeTaps tz = D.array ? ResizeTaps{ (long long)slice, 1u, nullptr } : resize_taps(table, D.ax[2], slice);
		const ResizeTaps tx = x < dx ? resize_taps(table, D.ax[0], x) : ResizeTaps{ 0, 0u, nullptr };
		uint32_t ty_at[PER], ty_n[PER];
		const double* ty_w[PER];
		#pragma unroll
		for (uint32_t q = 0; q < PER; q++)
		{
			const uint32_t y = y0 + row0 + q * (RESIZE_THREADS / TX);
			const ResizeTaps ty = x < dx && y < dy ? resize_taps(table, D.ax[1], y) : ResizeTaps{ ylo, 0u, nullptr };
			ty_at[q] = (uint32_t)(ty.first - ylo); ty_n[q] = ty.count; ty_w[q] = ty.w;
		}

		MipResizeSlot vol[PER][N];
		for (uint32_t kz = 0; kz < tz.count; kz++)
		{
			const uint32_t zs = D.array ? slice : mip_resample_source(tz.first + kz, D.ax[2].s, D.ax[2].edge);
			const double wz = D.array ? 1.0 : tz.w[kz];
			MipResizeSlot acc[PER][N];
			for (uint32_t chunk = 0; chunk < span; chunk += RESIZE_ROWS)
			{
				const uint32_t n = span - chunk < RESIZE_ROWS ? span - chunk : RESIZE_ROWS;
				// x pass: a thread's column is the same for every row it takes (RESIZE_THREADS is a multiple of TX)
				if (x < dx)
					for (uint32_t r = row0; r < n; r += RESIZE_THREADS / TX)
					{
						const uint32_t ys = mip_resample_source(ylo + (chunk + r), sy, D.ax[1].edge);
						const size_t base = ((size_t)zs * sy + ys) * sx;
						MipResizeSlot sum[N];
						for (uint32_t k = 0; k < tx.count; k++)
						{
							MipResizeSlot v[N];
							resize_load<K, N, INTS>(D.src, base + mip_resample_source(tx.first + k, sx, D.ax[0].edge), lin, v);
							mip_resize_accumulate<N, INTS>(sum, tx.w[k], v, k == 0);
						}
						#pragma unroll
						for (int ch = 0; ch < N; ch++) sh.rows[r][c][ch] = sum[ch];
					}
				__syncthreads();
				// y pass: the taps of this thread's texels that fall into the chunk
				#pragma unroll
				for (uint32_t q = 0; q < PER; q++)
				{
					const uint32_t end = ty_at[q] + ty_n[q];
					const uint32_t a = ty_at[q] > chunk ? ty_at[q] : chunk, b = end < chunk + n ? end : chunk + n;
					for (uint32_t i = a; i < b; i++)
					{
						const uint32_t r = i - chunk, k = i - ty_at[q];
						MipResizeSlot row[N];
						#pragma unroll
						for (int ch = 0; ch < N; ch++) row[ch] = sh.rows[r][c][ch];
						mip_resize_accumulate<N, INTS>(acc[q], ty_w[q][k], row, k == 0);
					}
				}
				__syncthreads();
			}
			#pragma unroll
			for (uint32_t q = 0; q < PER; q++) mip_resize_accumulate<N, INTS>(vol[q], wz, acc[q], kz == 0);
		}
		#pragma unroll
		for (uint32_t q = 0; q < PER; q++)
		{
			const uint32_t y = y0 + row0 + q * (RESIZE_THREADS / TX);
			if (x >= dx || y >= dy) continue;
			resize_store<K, N, BOX>(D.dst, ((size_t)slice * dy + y) * dx + x, vol[q], sh.srgb + 256, D.den, D.dden);
		}
	}
}

/* The table of a job: the head (ResizeDesc), then per axis (x, y and, for a VOLUME, z) its rows and its pool of weights.  0:
 * built; 1: above the 64 MiB bound (sized first: nothing is built for a table that is refused). */
int astc_resize_table_build(const ResizeJob& job, std::vector<uint8_t>& out)
{
	const bool volume = job.kind == 1, box = job.filter_kind == MIP_FILTER_BOX;
	const int axes = volume ? 3 : 2;
	const uint32_t s[3] = { job.dim_x, job.dim_y, job.dim_z }, d[3] = { job.out_x, job.out_y, job.out_z };
	ResizeDesc D;
	memset(&D, 0, sizeof(D));
	D.src = job.device_image; D.dst = job.device_out;
	D.dz = job.out_z; D.array = volume ? 0u : 1u;
	const uint32_t tile_x = job.weight ? 16u : 32u;
	D.tiles_x = (job.out_x + tile_x - 1) / tile_x; D.tiles_y = (job.out_y + RESIZE_TY - 1) / RESIZE_TY;
	D.den = 1;
	double dd[3] = { 1.0, 1.0, 1.0 };
	size_t bytes = RESIZE_HEAD;
	std::vector<ResizeRow> rows[3];
	for (int a = 0; a < 3; a++)
	{
		ResizeAxis& ax = D.ax[a];
		ax.s = s[a]; ax.d = d[a]; ax.edge = job.filter_edge; ax.period = 1;
		if (a >= axes) continue;
		mip_resize_period((int)job.filter_kind, s[a], d[a], &ax.period, &ax.shift);
		ax.rows_at = (uint32_t)bytes;
		bytes += (size_t)ax.period * sizeof(ResizeRow);
		if (bytes > RESIZE_TABLE_MAX) return 1;
		rows[a].resize(ax.period);
		ax.pool_at = (uint32_t)bytes;
		uint64_t at = 0;
		for (uint32_t j = 0; j < ax.period; j++)
		{
			unsigned int den;
			const unsigned long long count = mip_resize_tap_count((int)job.filter_kind, s[a], d[a], j, &rows[a][j].first, &den);
			if (count > RESIZE_TABLE_MAX / 8 || bytes + (at + count) * 8 > RESIZE_TABLE_MAX) return 1;
			rows[a][j].count = (uint32_t)count;
			rows[a][j].at = (uint32_t)at;
			at += count;
			if (box && j == 0) { D.den *= den; dd[a] = (double)den; }
		}
		bytes += (size_t)at * 8;
	}
	D.dden = (dd[0] * dd[1]) * dd[2];
	out.assign(bytes, 0);
	memcpy(out.data(), &D, sizeof(D));
	const auto sin_fn = [](double x) { return ::sin(x); };
	for (int a = 0; a < axes; a++)
	{
		memcpy(out.data() + D.ax[a].rows_at, rows[a].data(), rows[a].size() * sizeof(ResizeRow));
		double* pool = reinterpret_cast<double*>(out.data() + D.ax[a].pool_at);
		for (uint32_t j = 0; j < D.ax[a].period; j++)
			mip_resize_tap_weights((int)job.filter_kind, s[a], d[a], j, sin_fn, rows[a][j].first, rows[a][j].count, pool + rows[a][j].at);
	}
	return 0;
}

namespace {

template <int K, bool WEIGHTED, bool BOX>
int resize_launch_as(const ResizeJob& job, const uint8_t* d_table, const double* srgb, hipStream_t stream)
{
	constexpr uint32_t TX = WEIGHTED ? 16 : 32;
	const size_t tiles = (size_t)((job.out_x + TX - 1) / TX) * ((job.out_y + RESIZE_TY - 1) / RESIZE_TY) * job.out_z;
	const uint32_t groups = tiles < RESIZE_MAX_GROUPS ? (uint32_t)tiles : RESIZE_MAX_GROUPS;
	hipLaunchKernelGGL((astc_resize_image<K, WEIGHTED, BOX>), dim3(groups), dim3(RESIZE_THREADS), 0, stream, d_table, srgb);
	return (int)hipGetLastError();
}

template <int K>
int resize_launch_kind(const ResizeJob& job, const uint8_t* t, const double* srgb, hipStream_t s)
{
	const bool box = job.filter_kind == MIP_FILTER_BOX;
	if (job.weight) return box ? resize_launch_as<K, true, true>(job, t, srgb, s) : resize_launch_as<K, true, false>(job, t, srgb, s);
	return box ? resize_launch_as<K, false, true>(job, t, srgb, s) : resize_launch_as<K, false, false>(job, t, srgb, s);
}

} // namespace

int astc_resize_launch(const ResizeJob& job, const void* d_table, const void* d_srgb, void* stream)
{
	const uint8_t* t = static_cast<const uint8_t*>(d_table);
	const double* srgb = static_cast<const double*>(d_srgb);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return srgb && job.srgb ? resize_launch_kind<MIP_RS_U8_SRGB>(job, t, srgb, s) : resize_launch_kind<MIP_RS_U8>(job, t, srgb, s);
	case 1: return resize_launch_kind<MIP_RS_F16>(job, t, srgb, s);
	default: return resize_launch_kind<MIP_RS_F32>(job, t, srgb, s);
	}
}

} // namespace astcd
