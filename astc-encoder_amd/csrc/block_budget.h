// SPDX-License-Identifier: Apache-2.0
// Block selection over an image set with a block budget (astcenc_amd_select_blocks_set_device and the set driver,
// include/astcenc_amd.h): the global block index, the ranking key of a candidate, and the radix select
// that turns "the max_blocks candidates with the largest keys, lowest indices first among equal keys" into a cutoff key and the
// number `r` of blocks equal to it that are admitted.  The kernels of kernel_select_set.hip and the g++ harness of
// tests/test_block_budget_cpu.py compile this text.
//
//   global index   block g of the set counts the blocks of all entries back to back, raster order within an entry
//   candidate      e > max_mean_squared_error * n (block_select.h), n from the entry's own dimensions
//   key            the 64 bits of e / (double)n, one rounded fp64 division; 0 for a block that is no candidate.  A candidate has
//                  e > 0, so its key is a positive double or +inf: never 0, never a NaN, and keys order as their bits do
//   selected       with c candidates and c <= max_blocks every candidate; else the first max_blocks candidates in the order (key
//                  descending, global index ascending)
//
// The radix select walks the key from its most significant digit (BUDGET_DIGIT_BITS each).  Per digit the keys that agree with
// the prefix fixed so far are counted per digit value; walking the bins from the top, the first bin at which the running count
// reaches `remaining` holds the cutoff: its value joins the prefix, and `remaining` drops by the keys of the bins above it.
// After the last digit the prefix is the cutoff key and `remaining` is r (1 <= r <= the keys equal to the cutoff).
//
// No includes beyond the two headers below (which have none) and no HIP types.
#pragma once
#include "block_select.h"
#include "image_set.h"

namespace astcd {

constexpr unsigned int BUDGET_DIGIT_BITS = 8;
constexpr unsigned int BUDGET_BINS = 1u << BUDGET_DIGIT_BITS;
constexpr unsigned int BUDGET_DIGITS = 64 / BUDGET_DIGIT_BITS;
constexpr unsigned int BUDGET_NONE = 0xFFFFFFFFu;          // ASTCENC_AMD_NO_BLOCK_BUDGET

/* What the selection needs of entry i: its dimensions (the merge of the set driver adds the entry's output, `out`). */
struct BudgetEntry {
	unsigned int dim_x, dim_y, dim_z, pad;
	unsigned long long out;
};

/* The state of one selection in device memory, carried from launch to launch (no host round trip between digits). */
struct BudgetState {
	unsigned long long prefix;      // the digits fixed so far, in place; after the last digit: the cutoff key
	unsigned int remaining;         // keys still to admit among those that agree with the prefix; after the last digit: r
	unsigned int done;              // != 0: the cutoff is final (every candidate fits the budget, or the budget is 0)
	unsigned int candidates;        // c
	unsigned int selected;          // the length of the list
	unsigned int pad[2];
};

/* The 64 bits of a double. */
ASTC_SELECT_FN unsigned long long budget_bits(double v)
{
	unsigned long long b;
	__builtin_memcpy(&b, &v, sizeof(b));
	return b;
}

/* The key of a block from its weighted error `e` and its texels `n`: 0 when the block is no candidate. */
ASTC_SELECT_FN unsigned long long budget_key(double e, double max_mean_squared_error, unsigned int n)
{
	if (!block_select_test(e, max_mean_squared_error, n)) return 0ull;
	const double k = e / (double)n;
	return budget_bits(k);
}

/* The key of global block `g` of a set: first[] / entries[] as in image_set.h (first[i] the global index at which entry i
 * starts), `record` the block's four sums.  *entry receives the entry the block belongs to. */
template <typename FirstPtr, typename EntryPtr>
ASTC_SELECT_FN unsigned long long budget_block_key(FirstPtr first, EntryPtr entries, unsigned int count, unsigned int g, const double w[4],
                                                   double max_mean_squared_error, const double* record, unsigned int block_x,
                                                   unsigned int block_y, unsigned int block_z, unsigned int* entry)
{
	const unsigned int i = image_set_find(first, count, g);
	*entry = i;
	const unsigned int n = block_select_texels(g - first[i], entries[i].dim_x, entries[i].dim_y, entries[i].dim_z, block_x, block_y, block_z);
	return budget_key(block_select_error(w, record[0], record[1], record[2], record[3]), max_mean_squared_error, n);
}

/* Digit `pass` (0 = most significant) of a key, and whether the key agrees with `prefix` in the digits above it. */
ASTC_SELECT_FN unsigned int budget_shift(unsigned int pass) { return 64u - BUDGET_DIGIT_BITS * (pass + 1u); }
ASTC_SELECT_FN unsigned int budget_digit(unsigned long long key, unsigned int pass) { return (unsigned int)(key >> budget_shift(pass)) & (BUDGET_BINS - 1u); }
ASTC_SELECT_FN bool budget_in_prefix(unsigned long long key, unsigned long long prefix, unsigned int pass)
{
	// (a shift by 64 is undefined: pass 0 has no digits above it)
	return pass == 0u || (key >> (budget_shift(pass) + BUDGET_DIGIT_BITS)) == (prefix >> (budget_shift(pass) + BUDGET_DIGIT_BITS));
}

/* The bin that holds the cutoff: `above` keys lie in the bins over this one, `count` in it. */
ASTC_SELECT_FN bool budget_bin_hit(unsigned int above, unsigned int count, unsigned int remaining)
{
	return above < remaining && remaining - above <= count;
}

/* What the state is before the first digit, from the candidate count (the sum of the first histogram). */
ASTC_SELECT_FN void budget_begin(BudgetState& s, unsigned int candidates, unsigned int max_blocks)
{
	s.prefix = 0ull;
	s.candidates = candidates;
	s.remaining = max_blocks;
	s.done = 0u;
	// (the budget is 0: no key is above all ones, and none equals it -- that would be a NaN)
	if (max_blocks == 0u) { s.prefix = ~0ull; s.remaining = 0u; s.done = 1u; }
	// (every candidate fits: every key above 0 is listed, the blocks of key 0 are no candidates)
	else if (candidates <= max_blocks) { s.remaining = 0u; s.done = 1u; }
}

/* One digit, sequentially: hist[d] counts the keys of digit value d that agree with the prefix. */
ASTC_SELECT_FN void budget_step(BudgetState& s, const unsigned int* hist, unsigned int pass)
{
	if (s.done) return;
	unsigned int above = 0u;
	for (unsigned int d = BUDGET_BINS; d-- > 0u;)
	{
		if (budget_bin_hit(above, hist[d], s.remaining))
		{
			s.prefix |= (unsigned long long)d << budget_shift(pass);
			s.remaining -= above;
			return;
		}
		above += hist[d];
	}
}

/* Listed: the key is above the cutoff, or equals it with fewer than r equal keys before it in index order. */
ASTC_SELECT_FN bool budget_above(unsigned long long key, unsigned long long cutoff) { return key > cutoff; }
ASTC_SELECT_FN bool budget_equal(unsigned long long key, unsigned long long cutoff) { return key == cutoff; }
/* The slot of a listed block from the keys above the cutoff and the keys equal to it that precede the block in index order. */
ASTC_SELECT_FN unsigned int budget_slot(unsigned int above_before, unsigned int equal_before, unsigned int r)
{
	return above_before + (equal_before < r ? equal_before : r);
}

} // namespace astcd
