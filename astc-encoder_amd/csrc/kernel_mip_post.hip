// SPDX-License-Identifier: Apache-2.0
// The post-passes of a mip chain (astcenc_amd_generate_mip_chain_ex_device, mip_post.h): normal-map renormalisation and
// alpha-test coverage preservation, queued on the call's stream after the whole chain has been generated and before anything
// reads the levels.  No host synchronisation anywhere.
//
// A surface is what coverage is kept over: one per level of a 2D image or a volume, one per (level, layer) of an array.  The
// launches below walk tiles of TILE_UNITS 16-byte units (4 RGBA8, 2 F16 or 1 F32 texels each); a tile never spans two
// surfaces, so a workgroup knows its surface without a per-texel division.  Per group of layers (all of them, unless an array
// has so many layers that the scratch would pass MIP_POST_SCRATCH_LIMIT: post_plan):
//   1. astc_mippost_count   covered texels of every level-0 surface: a wave ballot + popcount per bit of the lane counts, the waves summed
//                           in LDS, one 64-bit atomic per workgroup and tile;
//   2. astc_mippost_hist    per pass, one 8-bit radix digit of the order-preserving alpha key (mip_post.h) over every surface
//                           of levels 1 .. n-1: texels whose higher digits equal the surface's prefix go into a 256-bin LDS
//                           histogram, flushed with one 64-bit atomic per non-zero bin; integer counts, so the result does not
//                           depend on arrival order.  U8 takes 1 pass, F16 2, F32 4;
//      astc_mippost_select  after each pass, one wave per surface: the first pass derives k from the level-0 count; the bins
//                           are scanned from the top, the digit fixed, the prefix and the remaining k updated and the bins
//                           zeroed for the next pass.  After the last pass the prefix is a_k;
//   3. astc_mippost_apply   one read-modify-write pass over levels 1 .. n-1: RGB renormalised and / or alpha remapped.
// The scratch (the level-0 counts, the bins and a state record per surface) is cleared by one fill per group.
#include "backend.h"
#include "mip_filter.h"
#include "mip_post.h"
#include <hip/hip_runtime.h>
#include <cstring>

namespace astcd {

constexpr uint32_t POST_THREADS = 256;
constexpr uint32_t POST_UNITS_PER_LANE = 4;
constexpr uint32_t TILE_UNITS = POST_THREADS * POST_UNITS_PER_LANE;    // 16-byte units per tile
constexpr uint32_t POST_MAX_GROUPS = 1u << 16;
constexpr size_t MIP_POST_SCRATCH_LIMIT = (size_t)64 << 20;            // a group's scratch stays below this

/* One level of a group: its surfaces lie back to back from `base` (the group's first layer), n texels each. */
struct MipPostSeg {
	uint8_t* base;
	unsigned long long n;              // texels per surface
	unsigned long long tiles;          // per surface
	unsigned long long first_tile;     // of the segment within the launch
	uint32_t surfaces;
	uint32_t first_surface;            // index of its first surface in the group's state (surface s: level-0 surface s - first_surface)
};

struct MipPostArgs {
	MipPostSeg seg[MIP_MAX_LEVELS];
	uint32_t segs;
	unsigned long long tiles;          // all segments'
	unsigned long long n0;             // texels of a level-0 surface
	uint32_t flags, t;                 // MIP_POST_*; U8 coverage threshold
	float cutoff, hi, lo;
};

/* Per surface, in the scratch (zeroed at the start of the group). */
struct MipPostState {
	unsigned long long k;              // the rank still to find within the current prefix
	uint32_t prefix;                   // the key digits fixed so far
	uint32_t skip;                     // 1: the surface stays unchanged (k == 0, a_k <= 0 or not finite)
	float ak;                          // the threshold alpha (float data); U8: ak_u8
	uint32_t ak_u8;
	uint32_t pad[2];
};
static_assert(sizeof(MipPostState) == 32, "state record");

template <int K> struct PostTexel;                 // 0 U8, 1 F16, 2 F32: a texel as stored
template <> struct PostTexel<0> { typedef uint32_t T; };
template <> struct PostTexel<1> { typedef uint2 T; };
template <> struct PostTexel<2> { typedef float4 T; };

/* Texel i of a surface with the component loads and stores a caller's level-0 image allows (U8 4 bytes, F16 2, F32 4). */
template <int K> __device__ inline typename PostTexel<K>::T post_load(const uint8_t* p, unsigned long long i);
template <> __device__ inline uint32_t post_load<0>(const uint8_t* p, unsigned long long i) { return reinterpret_cast<const uint32_t*>(p)[i]; }
template <> __device__ inline uint2 post_load<1>(const uint8_t* p, unsigned long long i)
{
	const uint16_t* h = reinterpret_cast<const uint16_t*>(p) + 4 * i;
	return make_uint2((uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16));
}
template <> __device__ inline float4 post_load<2>(const uint8_t* p, unsigned long long i)
{
	const float* f = reinterpret_cast<const float*>(p) + 4 * i;
	return make_float4(f[0], f[1], f[2], f[3]);
}
template <int K> __device__ inline void post_store(uint8_t* p, unsigned long long i, const typename PostTexel<K>::T& v);
template <> __device__ inline void post_store<0>(uint8_t* p, unsigned long long i, const uint32_t& v) { reinterpret_cast<uint32_t*>(p)[i] = v; }
template <> __device__ inline void post_store<1>(uint8_t* p, unsigned long long i, const uint2& v)
{
	uint16_t* h = reinterpret_cast<uint16_t*>(p) + 4 * i;
	h[0] = (uint16_t)v.x; h[1] = (uint16_t)(v.x >> 16); h[2] = (uint16_t)v.y; h[3] = (uint16_t)(v.y >> 16);
}
template <> __device__ inline void post_store<2>(uint8_t* p, unsigned long long i, const float4& v)
{
	float* f = reinterpret_cast<float*>(p) + 4 * i;
	f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
}

/* Tile -> (segment, surface within the segment, first texel within the surface, texel count). */
struct PostTile {
	uint32_t seg, surface;
	unsigned long long t0, count;
};
__device__ inline PostTile post_tile(const MipPostArgs& a, unsigned long long tile, uint32_t tpu)
{
	PostTile t;
	t.seg = 0;
	for (uint32_t i = 1; i < a.segs; i++)
		if (tile >= a.seg[i].first_tile) t.seg = i;
	const MipPostSeg& s = a.seg[t.seg];
	const unsigned long long local = tile - s.first_tile;
	const unsigned long long surface = local / s.tiles;
	t.surface = (uint32_t)surface;
	t.t0 = (local - surface * s.tiles) * TILE_UNITS * tpu;
	const unsigned long long left = s.n - t.t0;
	t.count = left < (unsigned long long)TILE_UNITS * tpu ? left : (unsigned long long)TILE_UNITS * tpu;
	return t;
}

/* Calls f(texel) for the texels of unit u of a tile, reading 16 bytes at once where the surface allows it.  f returns the
 * texel to store (write == true) or anything (write == false: read-only). */
template <int K, bool WRITE, typename F>
__device__ inline void post_unit(uint8_t* surf, unsigned long long t0, unsigned long long count, uint32_t u, bool aligned, F f)
{
	typedef typename PostTexel<K>::T T;
	constexpr uint32_t TPU = 16 / (uint32_t)sizeof(T);
	const unsigned long long first = (unsigned long long)u * TPU;
	if (first >= count) return;
	if (aligned && first + TPU <= count)
	{
		uint4* p = reinterpret_cast<uint4*>(surf + (t0 + first) * sizeof(T));
		uint4 v = *p;
		T tx[TPU];
		__builtin_memcpy(tx, &v, 16);
		#pragma unroll
		for (uint32_t j = 0; j < TPU; j++) tx[j] = f(tx[j]);
		if constexpr (WRITE)
		{
			__builtin_memcpy(&v, tx, 16);
			*p = v;
		}
		return;
	}
	for (uint32_t j = 0; j < TPU && first + j < count; j++)
	{
		const T v = f(post_load<K>(surf, t0 + first + j));
		if constexpr (WRITE) post_store<K>(surf, t0 + first + j, v);
	}
}

/* A texel's alpha: covered at level 0, and its radix key. */
template <int K> __device__ inline bool post_covered(const typename PostTexel<K>::T& v, const MipPostArgs& a);
template <> __device__ inline bool post_covered<0>(const uint32_t& v, const MipPostArgs& a) { return mip_covered_u8(v >> 24, a.t); }
template <> __device__ inline bool post_covered<1>(const uint2& v, const MipPostArgs& a)
{
	return mip_covered_float(mip_float_from_half((unsigned short)(v.y >> 16)), a.cutoff);
}
template <> __device__ inline bool post_covered<2>(const float4& v, const MipPostArgs& a) { return mip_covered_float(v.w, a.cutoff); }

template <int K> __device__ inline uint32_t post_key(const typename PostTexel<K>::T& v);
template <> __device__ inline uint32_t post_key<0>(const uint32_t& v) { return v >> 24; }
template <> __device__ inline uint32_t post_key<1>(const uint2& v) { return mip_key_f16((unsigned short)(v.y >> 16)); }
template <> __device__ inline uint32_t post_key<2>(const float4& v) { return mip_key_f32(v.w); }

template <int K> constexpr uint32_t post_passes() { return K == 0 ? 1u : K == 1 ? 2u : 4u; }

/* 1. Covered texels of every level-0 surface (the launch's one segment) into c0[surface]. */
template <int K>
__global__ void __launch_bounds__(POST_THREADS)
astc_mippost_count(MipPostArgs a, unsigned long long* __restrict__ c0)
{
	typedef typename PostTexel<K>::T T;
	constexpr uint32_t TPU = 16 / (uint32_t)sizeof(T);
	__shared__ uint32_t wave_sum[POST_THREADS / 64];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (unsigned long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x)
	{
		const PostTile t = post_tile(a, tile, TPU);
		const MipPostSeg& s = a.seg[t.seg];
		uint8_t* surf = s.base + (unsigned long long)t.surface * s.n * sizeof(T);
		const bool aligned = (reinterpret_cast<uintptr_t>(surf) & 15u) == 0;
		uint32_t mine = 0;                         // covered texels of this lane (at most 16)
		#pragma unroll
		for (uint32_t r = 0; r < POST_UNITS_PER_LANE; r++)
			post_unit<K, false>(surf, t.t0, t.count, r * POST_THREADS + threadIdx.x, aligned, [&](const T& v) {
				mine += post_covered<K>(v, a) ? 1u : 0u; return v; });
		// the wave's sum, bit by bit: a ballot and a popcount per bit of the lane counts (wave-uniform)
		uint32_t total = 0;
		#pragma unroll
		for (uint32_t bit = 0; bit < 5; bit++) total += (uint32_t)__popcll(__ballot((mine >> bit) & 1u)) << bit;
		if (lane == 0) wave_sum[wave] = total;
		__syncthreads();
		if (threadIdx.x == 0)
		{
			unsigned long long sum = 0;
			for (uint32_t w = 0; w < POST_THREADS / 64; w++) sum += wave_sum[w];
			if (sum) atomicAdd(&c0[t.surface], sum);
		}
		__syncthreads();
	}
}

/* 2. One radix pass over every surface of levels 1 .. n-1: digit `shift` of the keys whose digits above it equal the prefix. */
template <int K>
__global__ void __launch_bounds__(POST_THREADS)
astc_mippost_hist(MipPostArgs a, const MipPostState* __restrict__ state, unsigned long long* __restrict__ bins, uint32_t shift)
{
	typedef typename PostTexel<K>::T T;
	constexpr uint32_t TPU = 16 / (uint32_t)sizeof(T);
	__shared__ uint32_t hist[256];
	hist[threadIdx.x] = 0;                     // (POST_THREADS == 256: one bin per thread)
	__syncthreads();
	for (unsigned long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x)
	{
		const PostTile t = post_tile(a, tile, TPU);
		const MipPostSeg& s = a.seg[t.seg];
		const uint32_t id = s.first_surface + t.surface;
		const MipPostState st = state[id];
		if (st.skip) continue;                     // (uniform across the workgroup)
		uint8_t* surf = s.base + (unsigned long long)t.surface * s.n * sizeof(T);
		const bool aligned = (reinterpret_cast<uintptr_t>(surf) & 15u) == 0;
		const unsigned long long want = st.prefix;
		#pragma unroll
		for (uint32_t r = 0; r < POST_UNITS_PER_LANE; r++)
			post_unit<K, false>(surf, t.t0, t.count, r * POST_THREADS + threadIdx.x, aligned, [&](const T& v) {
				const unsigned long long key = post_key<K>(v);
				if ((key >> (shift + 8)) == want) atomicAdd(&hist[(key >> shift) & 0xFFu], 1u);
				return v; });
		__syncthreads();
		const uint32_t h = hist[threadIdx.x];
		if (h) atomicAdd(&bins[(size_t)id * 256 + threadIdx.x], (unsigned long long)h);
		hist[threadIdx.x] = 0;
		__syncthreads();
	}
}

/* ... and the digit it fixes: one wave per surface.  first: derive k from the level-0 count; last: turn the prefix into a_k. */
template <int K>
__global__ void __launch_bounds__(64)
astc_mippost_select(MipPostArgs a, const unsigned long long* __restrict__ c0, MipPostState* __restrict__ state,
                    unsigned long long* __restrict__ bins, uint32_t surfaces, uint32_t first, uint32_t last)
{
	const uint32_t lane = threadIdx.x;
	for (uint32_t id = blockIdx.x; id < surfaces; id += gridDim.x)
	{
		unsigned long long* b = bins + (size_t)id * 256;
		// lane l holds bins 255 - 4l .. 252 - 4l: descending key order runs along the lanes
		unsigned long long mine[4], sum = 0;
		#pragma unroll
		for (int j = 0; j < 4; j++) { mine[j] = b[255 - 4 * lane - j]; sum += mine[j]; }
		#pragma unroll
		for (int j = 0; j < 4; j++) b[255 - 4 * lane - j] = 0;            // (clear for the next pass)
		MipPostState st = state[id];
		if (st.skip) continue;
		if (first)
		{
			uint32_t seg = 0;
			for (uint32_t i = 1; i < a.segs; i++)
				if (id >= a.seg[i].first_surface) seg = i;
			st.k = mip_cover_target(c0[id - a.seg[seg].first_surface], a.seg[seg].n, a.n0);
		}
		unsigned long long incl = sum;
		#pragma unroll
		for (int d = 1; d < 64; d <<= 1)
		{
			const unsigned long long o = __shfl_up(incl, d, 64);
			if ((int)lane >= d) incl += o;
		}
		const unsigned long long hit = __ballot(st.k != 0 && incl >= st.k);
		if (!hit)
		{
			// k == 0 (or no texel left under the prefix): the surface stays unchanged
			if (lane == 0) { st.skip = 1; state[id] = st; }
			continue;
		}
		if (lane == (uint32_t)__builtin_ctzll(hit))
		{
			unsigned long long rem = st.k - (incl - sum);
			uint32_t digit = 0;
			for (int j = 0; j < 4; j++)
			{
				if (rem <= mine[j]) { digit = 255u - 4u * lane - (uint32_t)j; break; }
				rem -= mine[j];
			}
			st.prefix = (st.prefix << 8) | digit;
			st.k = rem;
			if (last)
			{
				if (K == 0)
				{
					st.ak_u8 = st.prefix;
					st.skip = st.prefix == 0 ? 1u : 0u;
				}
				else
				{
					const float ak = K == 1 ? mip_key_f16_value(st.prefix) : mip_key_f32_value(st.prefix);
					st.ak = ak;
					st.skip = (ak > 0.0f && ak < __builtin_inff()) ? 0u : 1u;
				}
			}
			state[id] = st;
		}
	}
}

/* 3. Levels 1 .. n-1: RGB renormalised (MIP_POST_NORMALIZE) and / or alpha remapped (MIP_POST_ALPHA_COVERAGE). */
template <int K>
__global__ void __launch_bounds__(POST_THREADS)
astc_mippost_apply(MipPostArgs a, const MipPostState* __restrict__ state)
{
	typedef typename PostTexel<K>::T T;
	constexpr uint32_t TPU = 16 / (uint32_t)sizeof(T);
	const bool norm = (a.flags & MIP_POST_NORMALIZE) != 0;
	for (unsigned long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x)
	{
		const PostTile t = post_tile(a, tile, TPU);
		const MipPostSeg& s = a.seg[t.seg];
		bool cover = false;
		MipPostState st;
		st.ak = 0.0f; st.ak_u8 = 0;
		if (a.flags & MIP_POST_ALPHA_COVERAGE)
		{
			st = state[s.first_surface + t.surface];
			cover = st.skip == 0;
		}
		if (!norm && !cover) continue;
		uint8_t* surf = s.base + (unsigned long long)t.surface * s.n * sizeof(T);
		const bool aligned = (reinterpret_cast<uintptr_t>(surf) & 15u) == 0;
		#pragma unroll
		for (uint32_t r = 0; r < POST_UNITS_PER_LANE; r++)
			post_unit<K, true>(surf, t.t0, t.count, r * POST_THREADS + threadIdx.x, aligned, [&](const T& v) {
				T o = v;
				if constexpr (K == 0)
				{
					if (norm) o = mip_normalize_u8(o);
					if (cover) o = (o & 0x00FFFFFFu) | (mip_cover_remap_u8(o >> 24, st.ak_u8, a.t) << 24);
				}
				else if constexpr (K == 1)
				{
					if (norm)
					{
						float x[3] = { mip_float_from_half((unsigned short)o.x), mip_float_from_half((unsigned short)(o.x >> 16)),
						               mip_float_from_half((unsigned short)o.y) };
						if (mip_normalize_float(x))
							o = make_uint2((uint32_t)mip_half_from_float(x[0]) | ((uint32_t)mip_half_from_float(x[1]) << 16),
							               (uint32_t)mip_half_from_float(x[2]) | (o.y & 0xFFFF0000u));
					}
					const unsigned short ah = (unsigned short)(o.y >> 16);
					if (cover && (ah & 0x7FFFu) <= 0x7C00u)            // (a NaN alpha keeps its bits)
					{
						const float r2 = mip_cover_remap_float(mip_float_from_half(ah), st.ak, a.cutoff, a.hi, a.lo, true);
						o.y = (o.y & 0xFFFFu) | ((uint32_t)mip_half_from_float(r2) << 16);
					}
				}
				else
				{
					if (norm)
					{
						float x[3] = { o.x, o.y, o.z };
						if (mip_normalize_float(x)) { o.x = x[0]; o.y = x[1]; o.z = x[2]; }
					}
					if (cover) o.w = mip_cover_remap_float(o.w, st.ak, a.cutoff, a.hi, a.lo, false);
				}
				return o; });
	}
}

namespace {

/* The group plan of a job: layers per group and the scratch one group needs. */
struct PostPlan {
	uint32_t layers;          // of the chain (ARRAY: dim_z; else 1)
	uint32_t group;           // layers per group
	size_t c0_bytes, bins_bytes, state_bytes;
};

PostPlan post_plan(const MipChainJob& job)
{
	PostPlan p;
	memset(&p, 0, sizeof(p));
	p.layers = job.kind == 0 ? job.dim_z : 1u;
	p.group = p.layers;
	if (!(job.post_flags & MIP_POST_ALPHA_COVERAGE) || job.level_count < 2) return p;
	const size_t per_layer = sizeof(unsigned long long) + (size_t)(job.level_count - 1) * (256 * sizeof(unsigned long long) + sizeof(MipPostState));
	const size_t fit = MIP_POST_SCRATCH_LIMIT / per_layer;
	if (fit < p.group) p.group = (uint32_t)(fit ? fit : 1);
	p.c0_bytes = (((size_t)p.group * sizeof(unsigned long long)) + 255) & ~(size_t)255;
	p.bins_bytes = (size_t)p.group * (job.level_count - 1) * 256 * sizeof(unsigned long long);
	p.state_bytes = (size_t)p.group * (job.level_count - 1) * sizeof(MipPostState);
	return p;
}

uint32_t grid_for(unsigned long long tiles) { return (uint32_t)(tiles < POST_MAX_GROUPS ? tiles : POST_MAX_GROUPS); }

template <int K>
int post_launch_kind(const MipChainJob& job, uint8_t* scratch, hipStream_t stream)
{
	typedef typename PostTexel<K>::T T;
	constexpr uint32_t TPU = 16 / (uint32_t)sizeof(T);
	const PostPlan plan = post_plan(job);
	const bool cover = (job.post_flags & MIP_POST_ALPHA_COVERAGE) != 0;
	const bool array = job.kind == 0;
	const uint32_t n = job.level_count;
	unsigned long long* c0 = reinterpret_cast<unsigned long long*>(scratch);
	unsigned long long* bins = reinterpret_cast<unsigned long long*>(scratch + plan.c0_bytes);
	MipPostState* state = reinterpret_cast<MipPostState*>(scratch + plan.c0_bytes + plan.bins_bytes);

	MipPostArgs base;
	memset(&base, 0, sizeof(base));
	base.flags = job.post_flags; base.t = job.cover_t;
	base.cutoff = job.alpha_cutoff; base.hi = job.cover_hi; base.lo = job.cover_lo;
	base.n0 = (unsigned long long)job.dim_x * job.dim_y * (array ? 1u : job.dim_z);
	const size_t tile_texels = (size_t)TILE_UNITS * TPU;

	for (uint32_t l0 = 0; l0 < plan.layers; l0 += plan.group)
	{
		const uint32_t g = plan.layers - l0 < plan.group ? plan.layers - l0 : plan.group;
		// levels 1 .. n-1 of layers [l0, l0 + g): segment i - 1 is level i, its surfaces numbered (i - 1) * g + layer
		MipPostArgs lv = base;
		uint32_t dx = job.dim_x, dy = job.dim_y, dz = job.dim_z;
		unsigned long long tiles = 0;
		for (uint32_t i = 1; i < n; i++)
		{
			dx = dx > 1 ? dx >> 1 : 1u; dy = dy > 1 ? dy >> 1 : 1u;
			if (!array) dz = dz > 1 ? dz >> 1 : 1u;
			MipPostSeg& s = lv.seg[i - 1];
			s.n = (unsigned long long)dx * dy * (array ? 1u : dz);
			s.base = job.device_levels + job.texels_offset[i] + (size_t)l0 * s.n * sizeof(T);
			s.surfaces = array ? g : 1u;
			s.tiles = (s.n + tile_texels - 1) / tile_texels;
			s.first_tile = tiles;
			s.first_surface = (i - 1) * s.surfaces;
			tiles += s.tiles * s.surfaces;
		}
		lv.segs = n - 1;
		lv.tiles = tiles;
		const uint32_t surfaces = (n - 1) * (array ? g : 1u);
		if (cover)
		{
			const size_t used = plan.c0_bytes + plan.bins_bytes + plan.state_bytes;
			const hipError_t me = hipMemsetAsync(scratch, 0, used, stream);
			if (me != hipSuccess) return (int)me;
			MipPostArgs top = base;
			MipPostSeg& s = top.seg[0];
			s.n = base.n0;
			s.base = static_cast<uint8_t*>(const_cast<void*>(job.device_image)) + (size_t)l0 * s.n * sizeof(T);
			s.surfaces = array ? g : 1u;
			s.tiles = (s.n + tile_texels - 1) / tile_texels;
			top.segs = 1;
			top.tiles = s.tiles * s.surfaces;
			hipLaunchKernelGGL(astc_mippost_count<K>, dim3(grid_for(top.tiles)), dim3(POST_THREADS), 0, stream, top, c0);
			constexpr uint32_t passes = post_passes<K>();
			const uint32_t sel_grid = surfaces < POST_MAX_GROUPS ? surfaces : POST_MAX_GROUPS;
			for (uint32_t p = 0; p < passes; p++)
			{
				const uint32_t shift = 8 * (passes - 1 - p);
				hipLaunchKernelGGL(astc_mippost_hist<K>, dim3(grid_for(tiles)), dim3(POST_THREADS), 0, stream, lv, state, bins, shift);
				hipLaunchKernelGGL(astc_mippost_select<K>, dim3(sel_grid), dim3(64), 0, stream, lv, c0, state, bins, surfaces,
				                   p == 0 ? 1u : 0u, p + 1 == passes ? 1u : 0u);
			}
		}
		hipLaunchKernelGGL(astc_mippost_apply<K>, dim3(grid_for(tiles)), dim3(POST_THREADS), 0, stream, lv, state);
		const hipError_t e = hipGetLastError();
		if (e != hipSuccess) return (int)e;
	}
	return 0;
}

} // namespace

size_t astc_mip_post_scratch_bytes(const MipChainJob& job)
{
	const PostPlan p = post_plan(job);
	return p.c0_bytes + p.bins_bytes + p.state_bytes;
}

int astc_mip_post_launch(const MipChainJob& job, void* d_scratch, void* stream)
{
	if (job.level_count < 2 || job.post_flags == 0) return 0;
	uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
	const hipStream_t s = static_cast<hipStream_t>(stream);
	switch (job.data_type)
	{
	case 0: return post_launch_kind<0>(job, scratch, s);
	case 1: return post_launch_kind<1>(job, scratch, s);
	default: return post_launch_kind<2>(job, scratch, s);
	}
}

} // namespace astcd
