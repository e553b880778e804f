// SPDX-License-Identifier: Apache-2.0
// Block selection and merge (astcenc_amd_select_blocks_device, astcenc_amd_compress_image_adaptive_device): an ascending,
// deterministic stream compaction of per-block error records against the criterion of block_select.h, and the keep-the-better
// rule between two streams.
//
// Selection is three kinds of launch on the stream, and no workgroup ever waits for another one:
//   astc_select_count    a workgroup of four wavefronts owns a tile of SELECT_TILE consecutive blocks, wavefront w the
//                        SELECT_WAVE_RUN blocks from w * SELECT_WAVE_RUN on; a wavefront ballots the predicate of 64 blocks at a
//                        time and adds the population counts, the four totals meet in LDS, counts[tile] = their sum
//   astc_select_scan     ONE workgroup turns counts[0 .. tiles) into their exclusive prefix sums in place, SCAN_THREADS at a time
//                        with a running carry, and leaves the total in counts[tiles]
//   astc_select_scatter  the tiles again: a wavefront recomputes its ballots, its first slot is counts[tile] plus the totals of
//                        the wavefronts before it in the tile, and a selected block's slot is that plus the selected blocks before
//                        it in the wavefront's run (the ballots so far, and the lanes below it in the current one)
// No atomics: a block's slot is a function of the records alone, so the list is ascending and the same on every run.  Block
// indices, counts and sums are 32-bit: at most 2^32 - 1 blocks, the limit of an image set.  The tiles of such an image exceed one
// grid's x dimension nowhere (2^21 of them), the scan loops.
//
// astc_merge_blocks: one thread per listed block; the replaced blocks are counted with one integer atomic per wavefront (a count,
// not a placement).
#include "backend.h"
#include "block_select.h"
#include <hip/hip_runtime.h>

namespace astcd {

constexpr uint32_t SELECT_WAVES = 4;
constexpr uint32_t SELECT_WAVE_TRIPS = 8;                        // ballots per wavefront
constexpr uint32_t SELECT_WAVE_RUN = 64u * SELECT_WAVE_TRIPS;    // blocks per wavefront
constexpr uint32_t SELECT_TILE = SELECT_WAVES * SELECT_WAVE_RUN; // blocks per workgroup
constexpr uint32_t SCAN_THREADS = 1024;

struct SelectArgs {
	const double* errors;
	uint32_t blocks;
	uint32_t dim_x, dim_y, dim_z, block_x, block_y, block_z;
	double weight[4], max_mse;
};

/* The predicate of block `b` (false past the image's blocks). */
__device__ inline bool select_test(const SelectArgs& a, uint32_t b, bool in_range)
{
	if (!in_range) return false;
	const double* s = a.errors + (size_t)b * 4;
	const double e = block_select_error(a.weight, s[0], s[1], s[2], s[3]);
	return block_select_test(e, a.max_mse, block_select_texels(b, a.dim_x, a.dim_y, a.dim_z, a.block_x, a.block_y, a.block_z));
}

/* Trip t of the calling wavefront: its block (and whether that is one of the image's; the comparison in 64 bits, the index
 * may wrap at 2^32) and the ballot of the predicate. */
__device__ inline unsigned long long select_trip(const SelectArgs& a, uint32_t wave, uint32_t lane, uint32_t t, uint32_t* block)
{
	const unsigned long long at = (unsigned long long)blockIdx.x * SELECT_TILE + wave * SELECT_WAVE_RUN + t * 64u + lane;
	*block = (uint32_t)at;
	return __ballot(select_test(a, (uint32_t)at, at < a.blocks));
}

__global__ void __launch_bounds__(64 * SELECT_WAVES)
astc_select_count(SelectArgs a, uint32_t* __restrict__ counts)
{
	__shared__ uint32_t wave_total[SELECT_WAVES];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	uint32_t n = 0, block;
	for (uint32_t t = 0; t < SELECT_WAVE_TRIPS; t++) n += (uint32_t)__popcll(select_trip(a, wave, lane, t, &block));
	if (lane == 0) wave_total[wave] = n;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		uint32_t sum = 0;
		for (uint32_t w = 0; w < SELECT_WAVES; w++) sum += wave_total[w];
		counts[blockIdx.x] = sum;
	}
}

/* counts[0 .. tiles) -> exclusive prefix sums, counts[tiles] = the total.  One workgroup. */
__global__ void __launch_bounds__(SCAN_THREADS)
astc_select_scan(uint32_t* __restrict__ counts, uint32_t tiles)
{
	__shared__ uint32_t wave_sum[SCAN_THREADS / 64];
	__shared__ uint32_t carry_out;
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	uint32_t carry = 0;
	for (uint32_t i0 = 0; i0 < tiles; i0 += SCAN_THREADS)
	{
		const uint32_t i = i0 + threadIdx.x;
		const uint32_t v = i < tiles ? counts[i] : 0u;
		uint32_t incl = v;                                          // inclusive scan inside the wavefront
		for (uint32_t off = 1; off < 64u; off <<= 1)
		{
			const uint32_t o = __shfl_up(incl, off);
			if (lane >= off) incl += o;
		}
		if (lane == 63u) wave_sum[wave] = incl;
		__syncthreads();
		uint32_t before = 0;
		for (uint32_t w = 0; w < wave; w++) before += wave_sum[w];
		if (i < tiles) counts[i] = carry + before + incl - v;
		if (threadIdx.x == SCAN_THREADS - 1u) carry_out = before + incl;
		__syncthreads();
		carry += carry_out;
	}
	if (threadIdx.x == 0) counts[tiles] = carry;
}

__global__ void __launch_bounds__(64 * SELECT_WAVES)
astc_select_scatter(SelectArgs a, const uint32_t* __restrict__ counts, uint32_t* __restrict__ list)
{
	__shared__ uint32_t wave_total[SELECT_WAVES];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	unsigned long long ballots[SELECT_WAVE_TRIPS];
	uint32_t n = 0, block;
	#pragma unroll
	for (uint32_t t = 0; t < SELECT_WAVE_TRIPS; t++)
	{
		ballots[t] = select_trip(a, wave, lane, t, &block);
		n += (uint32_t)__popcll(ballots[t]);
	}
	if (lane == 0) wave_total[wave] = n;
	__syncthreads();
	uint32_t slot = counts[blockIdx.x];
	for (uint32_t w = 0; w < wave; w++) slot += wave_total[w];
	const unsigned long long below = ((unsigned long long)1 << lane) - 1ull;
	#pragma unroll
	for (uint32_t t = 0; t < SELECT_WAVE_TRIPS; t++)
	{
		// (a set bit is a block of the image: select_trip's predicate is false past them)
		if ((ballots[t] >> lane) & 1ull)
			list[slot + (uint32_t)__popcll(ballots[t] & below)] = blockIdx.x * SELECT_TILE + wave * SELECT_WAVE_RUN + t * 64u + lane;
		slot += (uint32_t)__popcll(ballots[t]);
	}
}

struct MergeArgs {
	const uint32_t* list; const uint32_t* count;
	const double* strong_errors; double* base_errors;
	const uint8_t* strong; uint8_t* out;     // (16 bytes per block; the caller's buffer need not be 16-byte aligned)
	double weight[4];
	uint32_t blocks;
};

__global__ void __launch_bounds__(256)
astc_merge_blocks(MergeArgs m, uint32_t* __restrict__ replaced)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	bool take = false;
	if (i < *m.count)
	{
		const uint32_t b = m.list[i];
		if (b < m.blocks)
		{
			const double* s1 = m.strong_errors + (size_t)b * 4;
			double* s0 = m.base_errors + (size_t)b * 4;
			const double r0 = s1[0], r1 = s1[1], r2 = s1[2], r3 = s1[3];
			take = block_select_error(m.weight, r0, r1, r2, r3) < block_select_error(m.weight, s0[0], s0[1], s0[2], s0[3]);
			if (take)
			{
				for (int k = 0; k < 16; k++) m.out[(size_t)b * 16 + k] = m.strong[(size_t)b * 16 + k];
				s0[0] = r0; s0[1] = r1; s0[2] = r2; s0[3] = r3;
			}
		}
	}
	const unsigned long long taken = __ballot(take);
	if (threadIdx.x % 64u == 0 && taken) atomicAdd(replaced, (uint32_t)__popcll(taken));
}

static uint32_t select_tiles(size_t blocks) { return (uint32_t)((blocks + SELECT_TILE - 1) / SELECT_TILE); }
size_t astc_select_total_word(size_t blocks) { return select_tiles(blocks); }
size_t astc_select_scratch_words(size_t blocks) { return (size_t)select_tiles(blocks) + 1; }

int astc_select_launch(const SelectLaunch& s)
{
	SelectArgs a;
	a.errors = s.d_errors;
	a.dim_x = s.dim_x; a.dim_y = s.dim_y; a.dim_z = s.dim_z;
	a.block_x = s.block_x; a.block_y = s.block_y; a.block_z = s.block_z;
	const size_t blocks = s.blocks;
	if (blocks == 0) return (int)hipErrorInvalidValue;
	a.blocks = s.blocks;
	for (int i = 0; i < 4; i++) a.weight[i] = s.weight[i];
	a.max_mse = s.max_mse;
	const uint32_t tiles = select_tiles(blocks);
	const hipStream_t stream = static_cast<hipStream_t>(s.stream);
	hipLaunchKernelGGL(astc_select_count, dim3(tiles), dim3(64 * SELECT_WAVES), 0, stream, a, s.d_counts);
	hipLaunchKernelGGL(astc_select_scan, dim3(1), dim3(SCAN_THREADS), 0, stream, s.d_counts, tiles);
	hipLaunchKernelGGL(astc_select_scatter, dim3(tiles), dim3(64 * SELECT_WAVES), 0, stream, a, s.d_counts, s.d_list);
	return (int)hipGetLastError();
}

int astc_merge_launch(const MergeLaunch& l)
{
	const hipStream_t stream = static_cast<hipStream_t>(l.stream);
	hipError_t e = hipMemsetAsync(l.d_replaced, 0, sizeof(uint32_t), stream);
	if (e != hipSuccess) return (int)e;
	if (l.max_count == 0) return 0;
	MergeArgs m;
	m.list = l.d_list; m.count = l.d_count;
	m.strong_errors = l.d_strong_errors; m.base_errors = l.d_base_errors;
	m.strong = l.d_strong; m.out = l.d_out;
	for (int i = 0; i < 4; i++) m.weight[i] = l.weight[i];
	m.blocks = l.blocks;
	hipLaunchKernelGGL(astc_merge_blocks, dim3((l.max_count + 255u) / 256u), dim3(256), 0, stream, m, l.d_replaced);
	return (int)hipGetLastError();
}

} // namespace astcd
