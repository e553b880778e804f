// SPDX-License-Identifier: Apache-2.0
// Block selection over an image set with a block budget, and the keep-the-better merge over a set's separate output buffers
// (astcenc_amd_select_blocks_set_device, astcenc_amd_compress_images_adaptive_device; the arithmetic: block_budget.h).
//
// The launches of one selection, all on one stream; no workgroup ever waits for another one and nothing returns to the host
// between them:
//   astc_budget_keys     one thread per block of the set: the block's entry (image_set_find over the table's first[]), its key
//                        into keys[g] (0: no candidate), and -- with a budget -- the histogram of the keys' top digit
//   astc_budget_hist     digits 1 .. 7: the histogram of the keys that agree with the prefix fixed so far.  LDS histograms
//                        (integer atomics; a wavefront whose keys share a digit adds their number once), then one integer atomic
//                        per non-empty bin into the global histogram of the digit
//   astc_budget_pick     ONE workgroup, a thread per bin: a suffix sum over the bins from the top, and the one thread whose bin
//                        holds the cutoff (budget_bin_hit) fixes the digit and carries prefix and remaining count in BudgetState
//   astc_budget_count / astc_budget_scan / astc_budget_scatter
//                        the shape of kernel_select.hip with two counters per tile: keys above the cutoff, keys equal to it.  A
//                        block's slot is budget_slot() of the two counts before it in index order
// With ASTCENC_AMD_NO_BLOCK_BUDGET the histogram and pick launches are left out (the zeroed state is the cutoff 0 with r = 0: every
// candidate); with a budget that every candidate fits, or one of 0, the first pick marks the state done and the later ones return.
// The atomics count; they never place: the list is a function of the records alone.
#include "backend.h"
#include "block_budget.h"
#include <hip/hip_runtime.h>

namespace astcd {

constexpr uint32_t BUDGET_WAVES = 8;
constexpr uint32_t BUDGET_WAVE_TRIPS = 8;                          // ballots per wavefront
constexpr uint32_t BUDGET_WAVE_RUN = 64u * BUDGET_WAVE_TRIPS;      // blocks per wavefront
constexpr uint32_t BUDGET_TILE = BUDGET_WAVES * BUDGET_WAVE_RUN;   // blocks per workgroup: two words of scratch per 4096 blocks
constexpr uint32_t BUDGET_SCAN_THREADS = 1024;
constexpr uint32_t HIST_THREADS = 256;
constexpr uint32_t HIST_TRIPS = 8;                                 // keys per thread
constexpr uint32_t HIST_TILE = HIST_THREADS * HIST_TRIPS;
static_assert(BUDGET_BINS == HIST_THREADS, "astc_budget_pick and the histogram flush have one thread per bin");

struct BudgetKeyArgs {
	const double* errors;
	const uint8_t* table;            // ImageSetTable, first[count], BudgetEntry[count] (astc_budget_table_build)
	unsigned long long* keys;
	uint32_t* hist;                  // BUDGET_DIGITS x BUDGET_BINS words, zeroed; null: no histogram (no budget)
	uint32_t block_x, block_y, block_z;
	double weight[4], max_mse;
};

/* Adds the digits of a wavefront's keys (active: the lane has one) to the LDS histogram. */
__device__ inline void hist_add(uint32_t* bins, bool active, uint32_t digit)
{
	const unsigned long long any = __ballot(active);
	if (!any) return;
	// the digit of the first lane that has a key, and every lane that shares it: one atomic for all of them
	const uint32_t lead = (uint32_t)__builtin_ctzll(any);
	const uint32_t d0 = (uint32_t)__shfl((int)digit, (int)lead);
	const unsigned long long same = __ballot(active && digit == d0);
	const uint32_t lane = threadIdx.x % 64u;
	if (lane == lead) atomicAdd(&bins[d0], (uint32_t)__popcll(same));
	else if (active && digit != d0) atomicAdd(&bins[digit], 1u);
}

/* The workgroup's LDS histogram into the global one of digit `pass`. */
__device__ inline void hist_flush(const uint32_t* bins, uint32_t* hist, uint32_t pass)
{
	__syncthreads();
	const uint32_t n = bins[threadIdx.x];
	if (n) atomicAdd(&hist[pass * BUDGET_BINS + threadIdx.x], n);
}

__global__ void __launch_bounds__(HIST_THREADS)
astc_budget_keys(BudgetKeyArgs a)
{
	__shared__ uint32_t bins[BUDGET_BINS];
	bins[threadIdx.x] = 0u;
	__syncthreads();
	const ImageSetTable* t = reinterpret_cast<const ImageSetTable*>(a.table);
	const uint32_t count = t->count, total = t->total;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(a.table + image_set_first_offset());
	const BudgetEntry* entries = reinterpret_cast<const BudgetEntry*>(a.table + image_set_records_offset(count));
	for (uint32_t trip = 0; trip < HIST_TRIPS; trip++)
	{
		// (the comparison in 64 bits: the index may wrap at 2^32)
		const unsigned long long at = (unsigned long long)blockIdx.x * HIST_TILE + trip * HIST_THREADS + threadIdx.x;
		const bool in_range = at < total;
		unsigned long long key = 0ull;
		if (in_range)
		{
			uint32_t entry;
			key = budget_block_key(first, entries, count, (uint32_t)at, a.weight, a.max_mse, a.errors + (size_t)at * 4, a.block_x, a.block_y, a.block_z, &entry);
			a.keys[at] = key;
		}
		if (a.hist) hist_add(bins, key != 0ull, budget_digit(key, 0));
	}
	if (a.hist) hist_flush(bins, a.hist, 0);
}

__global__ void __launch_bounds__(HIST_THREADS)
astc_budget_hist(const unsigned long long* __restrict__ keys, uint32_t total, const BudgetState* __restrict__ state, uint32_t* __restrict__ hist, uint32_t pass)
{
	__shared__ uint32_t bins[BUDGET_BINS];
	if (state->done) return;
	const unsigned long long prefix = state->prefix;
	bins[threadIdx.x] = 0u;
	__syncthreads();
	for (uint32_t trip = 0; trip < HIST_TRIPS; trip++)
	{
		const unsigned long long at = (unsigned long long)blockIdx.x * HIST_TILE + trip * HIST_THREADS + threadIdx.x;
		const unsigned long long key = at < total ? keys[at] : 0ull;
		hist_add(bins, key != 0ull && budget_in_prefix(key, prefix, pass), budget_digit(key, pass));
	}
	hist_flush(bins, hist, pass);
}

/* One workgroup, thread t owns bin BUDGET_BINS - 1 - t: the bins from the top. */
__global__ void __launch_bounds__(HIST_THREADS)
astc_budget_pick(const uint32_t* __restrict__ hist, BudgetState* __restrict__ state, uint32_t pass, uint32_t max_blocks)
{
	__shared__ uint32_t wave_sum[HIST_THREADS / 64];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	const uint32_t bin = BUDGET_BINS - 1u - threadIdx.x;
	const uint32_t n = hist[pass * BUDGET_BINS + bin];
	uint32_t incl = n;                                            // inclusive sum of this bin and the bins above it
	for (uint32_t off = 1; off < 64u; off <<= 1)
	{
		const uint32_t o = __shfl_up(incl, off);
		if (lane >= off) incl += o;
	}
	if (lane == 63u) wave_sum[wave] = incl;
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t w = 0; w < HIST_THREADS / 64; w++) { if (w < wave) before += wave_sum[w]; all += wave_sum[w]; }
	const uint32_t above = before + incl - n;
	// (every thread reads the state before any thread writes it: the barrier below)
	BudgetState s = *state;
	if (pass == 0) budget_begin(s, all, max_blocks);
	__syncthreads();
	// (thread 0 writes what budget_begin decides, and prefix and remaining only when that is final: otherwise they are the
	//  writes of the one thread below)
	if (pass == 0 && threadIdx.x == 0)
	{
		state->candidates = s.candidates;
		state->done = s.done;
		if (s.done) { state->prefix = s.prefix; state->remaining = s.remaining; }
	}
	if (s.done) return;
	if (budget_bin_hit(above, n, s.remaining))
	{
		// (one thread: the bins above this one hold fewer than `remaining` keys, with this one they hold at least as many)
		state->prefix = s.prefix | ((unsigned long long)bin << budget_shift(pass));
		state->remaining = s.remaining - above;
	}
}

/* Trip t of the calling wavefront: the ballots of "above the cutoff" and "equal to it" over its 64 blocks. */
__device__ inline void budget_trip(const unsigned long long* keys, uint32_t total, unsigned long long cutoff, uint32_t wave, uint32_t lane, uint32_t t,
                                   unsigned long long* above, unsigned long long* equal)
{
	const unsigned long long at = (unsigned long long)blockIdx.x * BUDGET_TILE + wave * BUDGET_WAVE_RUN + t * 64u + lane;
	const bool in_range = at < total;
	const unsigned long long key = in_range ? keys[at] : 0ull;
	*above = __ballot(in_range && budget_above(key, cutoff));
	*equal = __ballot(in_range && budget_equal(key, cutoff));
}

/* counts[2 * tile] = the tile's keys above the cutoff, counts[2 * tile + 1] = its keys equal to it. */
__global__ void __launch_bounds__(64 * BUDGET_WAVES)
astc_budget_count(const unsigned long long* __restrict__ keys, uint32_t total, const BudgetState* __restrict__ state, uint32_t* __restrict__ counts)
{
	__shared__ uint32_t wave_total[BUDGET_WAVES][2];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	const unsigned long long cutoff = state->prefix;
	uint32_t na = 0, ne = 0;
	for (uint32_t t = 0; t < BUDGET_WAVE_TRIPS; t++)
	{
		unsigned long long above, equal;
		budget_trip(keys, total, cutoff, wave, lane, t, &above, &equal);
		na += (uint32_t)__popcll(above);
		ne += (uint32_t)__popcll(equal);
	}
	if (lane == 0) { wave_total[wave][0] = na; wave_total[wave][1] = ne; }
	__syncthreads();
	if (threadIdx.x < 2u)
	{
		uint32_t sum = 0;
		for (uint32_t w = 0; w < BUDGET_WAVES; w++) sum += wave_total[w][threadIdx.x];
		counts[2u * blockIdx.x + threadIdx.x] = sum;
	}
}

/* The pairs counts[2 i], counts[2 i + 1], i < tiles -> their exclusive prefix sums in place; the length of the list into the
 * state (and, without a budget, the candidate count: the same number).  One workgroup. */
__global__ void __launch_bounds__(BUDGET_SCAN_THREADS)
astc_budget_scan(uint32_t* __restrict__ counts, uint32_t tiles, BudgetState* __restrict__ state, uint32_t no_budget)
{
	__shared__ uint32_t wave_sum[BUDGET_SCAN_THREADS / 64][2];
	__shared__ uint32_t carry_out[2];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	uint32_t carry[2] = { 0u, 0u };
	for (uint32_t i0 = 0; i0 < tiles; i0 += BUDGET_SCAN_THREADS)
	{
		const uint32_t i = i0 + threadIdx.x;
		uint32_t v[2], incl[2];
		for (uint32_t k = 0; k < 2u; k++) incl[k] = v[k] = i < tiles ? counts[2u * i + k] : 0u;
		for (uint32_t off = 1; off < 64u; off <<= 1)
			for (uint32_t k = 0; k < 2u; k++)
			{
				const uint32_t o = __shfl_up(incl[k], off);
				if (lane >= off) incl[k] += o;
			}
		if (lane == 63u) { wave_sum[wave][0] = incl[0]; wave_sum[wave][1] = incl[1]; }
		__syncthreads();
		for (uint32_t k = 0; k < 2u; k++)
		{
			uint32_t before = 0;
			for (uint32_t w = 0; w < wave; w++) before += wave_sum[w][k];
			if (i < tiles) counts[2u * i + k] = carry[k] + before + incl[k] - v[k];
			if (threadIdx.x == BUDGET_SCAN_THREADS - 1u) carry_out[k] = before + incl[k];
		}
		__syncthreads();
		carry[0] += carry_out[0];
		carry[1] += carry_out[1];
	}
	if (threadIdx.x == 0)
	{
		const uint32_t selected = budget_slot(carry[0], carry[1], state->remaining);
		state->selected = selected;
		if (no_budget) state->candidates = selected;
	}
}

__global__ void __launch_bounds__(64 * BUDGET_WAVES)
astc_budget_scatter(const unsigned long long* __restrict__ keys, uint32_t total, const BudgetState* __restrict__ state, const uint32_t* __restrict__ counts,
                    uint32_t* __restrict__ list)
{
	__shared__ uint32_t wave_total[BUDGET_WAVES][2];
	const uint32_t wave = threadIdx.x / 64u, lane = threadIdx.x % 64u;
	const unsigned long long cutoff = state->prefix;
	const uint32_t r = state->remaining;
	unsigned long long above[BUDGET_WAVE_TRIPS], equal[BUDGET_WAVE_TRIPS];
	uint32_t na = 0, ne = 0;
	#pragma unroll
	for (uint32_t t = 0; t < BUDGET_WAVE_TRIPS; t++)
	{
		budget_trip(keys, total, cutoff, wave, lane, t, &above[t], &equal[t]);
		na += (uint32_t)__popcll(above[t]);
		ne += (uint32_t)__popcll(equal[t]);
	}
	if (lane == 0) { wave_total[wave][0] = na; wave_total[wave][1] = ne; }
	__syncthreads();
	uint32_t a_before = counts[2u * blockIdx.x], e_before = counts[2u * blockIdx.x + 1u];
	for (uint32_t w = 0; w < wave; w++) { a_before += wave_total[w][0]; e_before += wave_total[w][1]; }
	const unsigned long long below = ((unsigned long long)1 << lane) - 1ull;
	#pragma unroll
	for (uint32_t t = 0; t < BUDGET_WAVE_TRIPS; t++)
	{
		// (a set bit is a block of the set: budget_trip's ballots are clear past them)
		const uint32_t a_mine = a_before + (uint32_t)__popcll(above[t] & below), e_mine = e_before + (uint32_t)__popcll(equal[t] & below);
		const bool is_above = (above[t] >> lane) & 1ull, is_equal = (equal[t] >> lane) & 1ull;
		if (is_above || (is_equal && e_mine < r))
			list[budget_slot(a_mine, e_mine, r)] = blockIdx.x * BUDGET_TILE + wave * BUDGET_WAVE_RUN + t * 64u + lane;
		a_before += (uint32_t)__popcll(above[t]);
		e_before += (uint32_t)__popcll(equal[t]);
	}
}

/* The merge over a set: as astc_merge_blocks, with the strong stream and both record arrays indexed by the global block and the
 * 16 bytes stored into the entry's own buffer (byte stores: a caller's buffer need not be aligned). */
struct MergeSetArgs {
	const uint32_t* list; const BudgetState* state;
	const double* strong_errors; double* base_errors;
	const uint8_t* strong;
	const uint8_t* table;
	double weight[4];
};

__global__ void __launch_bounds__(256)
astc_merge_blocks_set(MergeSetArgs m, uint32_t* __restrict__ replaced)
{
	const ImageSetTable* t = reinterpret_cast<const ImageSetTable*>(m.table);
	const uint32_t count = t->count, total = t->total;
	const uint32_t* first = reinterpret_cast<const uint32_t*>(m.table + image_set_first_offset());
	const BudgetEntry* entries = reinterpret_cast<const BudgetEntry*>(m.table + image_set_records_offset(count));
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	bool take = false;
	if (i < m.state->selected)
	{
		const uint32_t g = m.list[i];
		if (g < total)
		{
			const double* s1 = m.strong_errors + (size_t)g * 4;
			double* s0 = m.base_errors + (size_t)g * 4;
			const double r0 = s1[0], r1 = s1[1], r2 = s1[2], r3 = s1[3];
			take = block_select_error(m.weight, r0, r1, r2, r3) < block_select_error(m.weight, s0[0], s0[1], s0[2], s0[3]);
			if (take)
			{
				const uint32_t e = image_set_find(first, count, g);
				uint8_t* out = reinterpret_cast<uint8_t*>(entries[e].out) + (size_t)(g - first[e]) * 16;
				for (int k = 0; k < 16; k++) out[k] = m.strong[(size_t)g * 16 + k];
				s0[0] = r0; s0[1] = r1; s0[2] = r2; s0[3] = r3;
			}
		}
	}
	const unsigned long long taken = __ballot(take);
	if (threadIdx.x % 64u == 0 && taken) atomicAdd(replaced, (uint32_t)__popcll(taken));
}

static uint32_t budget_tiles(size_t blocks) { return (uint32_t)((blocks + BUDGET_TILE - 1) / BUDGET_TILE); }
size_t astc_budget_count_words(size_t blocks) { return 2 * (size_t)budget_tiles(blocks); }
size_t astc_budget_fixed_bytes() { return sizeof(BudgetState) + (size_t)BUDGET_DIGITS * BUDGET_BINS * sizeof(uint32_t); }
size_t astc_budget_table_bytes(uint32_t count) { return (size_t)image_set_records_offset(count) + (size_t)count * sizeof(BudgetEntry); }

void astc_budget_table_build(void* out, const BudgetSetEntry* entries, uint32_t count, uint32_t block_x, uint32_t block_y, uint32_t block_z)
{
	uint8_t* p = static_cast<uint8_t*>(out);
	ImageSetTable* t = reinterpret_cast<ImageSetTable*>(p);
	uint32_t* first = reinterpret_cast<uint32_t*>(p + image_set_first_offset());
	BudgetEntry* rec = reinterpret_cast<BudgetEntry*>(p + image_set_records_offset(count));
	size_t total = 0;
	for (uint32_t e = 0; e < count; e++)
	{
		first[e] = (uint32_t)total;
		rec[e].dim_x = entries[e].dim_x; rec[e].dim_y = entries[e].dim_y; rec[e].dim_z = entries[e].dim_z; rec[e].pad = 0;
		rec[e].out = reinterpret_cast<uintptr_t>(entries[e].device_out);
		total += (size_t)((entries[e].dim_x + block_x - 1) / block_x) * ((entries[e].dim_y + block_y - 1) / block_y) * ((entries[e].dim_z + block_z - 1) / block_z);
	}
	t->count = count;
	t->total = (uint32_t)total;     // (at most 2^32 - 1: the entry points check)
	t->pad[0] = t->pad[1] = 0;
}

int astc_budget_select_launch(const BudgetSelectLaunch& s)
{
	if (s.blocks == 0) return (int)hipErrorInvalidValue;
	const hipStream_t stream = static_cast<hipStream_t>(s.stream);
	BudgetState* state = reinterpret_cast<BudgetState*>(s.d_fixed);
	uint32_t* hist = reinterpret_cast<uint32_t*>(s.d_fixed + sizeof(BudgetState));
	const bool budget = s.max_blocks != BUDGET_NONE;
	hipError_t e = hipMemsetAsync(s.d_fixed, 0, astc_budget_fixed_bytes(), stream);
	if (e != hipSuccess) return (int)e;
	BudgetKeyArgs a;
	a.errors = s.d_errors; a.table = s.d_table; a.keys = s.d_keys; a.hist = budget ? hist : nullptr;
	a.block_x = s.block_x; a.block_y = s.block_y; a.block_z = s.block_z;
	for (int i = 0; i < 4; i++) a.weight[i] = s.weight[i];
	a.max_mse = s.max_mse;
	const uint32_t hist_grid = (uint32_t)(((size_t)s.blocks + HIST_TILE - 1) / HIST_TILE), tiles = budget_tiles(s.blocks);
	hipLaunchKernelGGL(astc_budget_keys, dim3(hist_grid), dim3(HIST_THREADS), 0, stream, a);
	if (budget)
		for (uint32_t pass = 0; pass < BUDGET_DIGITS; pass++)
		{
			if (pass) hipLaunchKernelGGL(astc_budget_hist, dim3(hist_grid), dim3(HIST_THREADS), 0, stream, s.d_keys, s.blocks, state, hist, pass);
			hipLaunchKernelGGL(astc_budget_pick, dim3(1), dim3(HIST_THREADS), 0, stream, hist, state, pass, s.max_blocks);
		}
	hipLaunchKernelGGL(astc_budget_count, dim3(tiles), dim3(64 * BUDGET_WAVES), 0, stream, s.d_keys, s.blocks, state, s.d_counts);
	hipLaunchKernelGGL(astc_budget_scan, dim3(1), dim3(BUDGET_SCAN_THREADS), 0, stream, s.d_counts, tiles, state, budget ? 0u : 1u);
	hipLaunchKernelGGL(astc_budget_scatter, dim3(tiles), dim3(64 * BUDGET_WAVES), 0, stream, s.d_keys, s.blocks, state, s.d_counts, s.d_list);
	return (int)hipGetLastError();
}

const uint32_t* astc_budget_counts(const uint8_t* d_fixed) { return &reinterpret_cast<const BudgetState*>(d_fixed)->candidates; }

int astc_merge_set_launch(const MergeSetLaunch& l)
{
	const hipStream_t stream = static_cast<hipStream_t>(l.stream);
	hipError_t e = hipMemsetAsync(l.d_replaced, 0, sizeof(uint32_t), stream);
	if (e != hipSuccess) return (int)e;
	if (l.max_count == 0) return 0;
	MergeSetArgs m;
	m.list = l.d_list; m.state = reinterpret_cast<const BudgetState*>(l.d_fixed);
	m.strong_errors = l.d_strong_errors; m.base_errors = l.d_base_errors;
	m.strong = l.d_strong; m.table = l.d_table;
	for (int i = 0; i < 4; i++) m.weight[i] = l.weight[i];
	hipLaunchKernelGGL(astc_merge_blocks_set, dim3((l.max_count + 255u) / 256u), dim3(256), 0, stream, m, l.d_replaced);
	return (int)hipGetLastError();
}

} // namespace astcd
