// SPDX-License-Identifier: Apache-2.0
// Host harness of tests/test_block_budget_cpu.py: csrc/block_budget.h -- the text the set selection kernels compile -- over the
// records of a file, for a numpy model to compare with: every block's key, candidate flag and entry, and the sequential form
// of the radix select (cutoff key and r) with the list it gives.
//   block_budget_check <in> <out>
//   in : uint32 block_x, block_y, block_z, entries, max_blocks, 0, 0, 0; double weight[4], threshold; uint32 dims[entries][3];
//        double records[blocks of the set][4]
//   out: per block  uint64 key; uint32 candidate; uint32 entry
//        then       uint64 cutoff; uint32 r, candidates, selected, 0; uint32 list[selected]
#include "block_budget.h"

#include <cstdint>
#include <cstdio>
#include <vector>

using namespace astcd;

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	uint32_t head[8];
	double crit[5];
	if (fread(head, sizeof(head), 1, in) != 1 || fread(crit, sizeof(crit), 1, in) != 1) return 3;
	const uint32_t count = head[3], max_blocks = head[4];
	std::vector<uint32_t> dims((size_t)count * 3), first(count);
	if (count && fread(dims.data(), sizeof(uint32_t), dims.size(), in) != dims.size()) return 3;
	std::vector<BudgetEntry> entries(count);
	uint32_t total = 0;
	for (uint32_t e = 0; e < count; e++)
	{
		first[e] = total;
		entries[e] = { dims[3 * e], dims[3 * e + 1], dims[3 * e + 2], 0u, 0ull };
		total += ((dims[3 * e] + head[0] - 1) / head[0]) * ((dims[3 * e + 1] + head[1] - 1) / head[1]) * ((dims[3 * e + 2] + head[2] - 1) / head[2]);
	}
	std::vector<double> records((size_t)total * 4);
	if (total && fread(records.data(), sizeof(double), records.size(), in) != records.size()) return 3;

	std::vector<unsigned long long> keys(total);
	for (uint32_t g = 0; g < total; g++)
	{
		uint32_t entry = 0;
		keys[g] = budget_block_key(first.data(), entries.data(), count, g, crit, crit[4], &records[(size_t)g * 4], head[0], head[1], head[2], &entry);
		const uint32_t candidate = keys[g] != 0ull ? 1u : 0u;
		fwrite(&keys[g], sizeof(keys[g]), 1, out);
		fwrite(&candidate, sizeof(candidate), 1, out);
		fwrite(&entry, sizeof(entry), 1, out);
	}

	// the radix select, digit by digit, as the kernels run it (without a budget: the zeroed state, every candidate)
	BudgetState s = {};
	if (max_blocks != BUDGET_NONE)
		for (uint32_t pass = 0; pass < BUDGET_DIGITS; pass++)
		{
			std::vector<uint32_t> hist(BUDGET_BINS, 0u);
			uint32_t candidates = 0;
			for (uint32_t g = 0; g < total; g++)
			{
				if (keys[g] == 0ull) continue;
				candidates++;
				if (budget_in_prefix(keys[g], s.prefix, pass)) hist[budget_digit(keys[g], pass)]++;
			}
			if (pass == 0) budget_begin(s, candidates, max_blocks);
			budget_step(s, hist.data(), pass);
		}
	std::vector<uint32_t> list;
	uint32_t above = 0, equal = 0, candidates = 0;
	for (uint32_t g = 0; g < total; g++)
	{
		const bool is_above = budget_above(keys[g], s.prefix), is_equal = budget_equal(keys[g], s.prefix);
		if (keys[g] != 0ull) candidates++;
		if (is_above || (is_equal && equal < s.remaining))
		{
			if (budget_slot(above, equal, s.remaining) != list.size()) return 5;
			list.push_back(g);
		}
		above += is_above ? 1u : 0u;
		equal += is_equal ? 1u : 0u;
	}
	const uint32_t tail[4] = { s.remaining, candidates, (uint32_t)list.size(), 0u };
	if (budget_slot(above, equal, s.remaining) != list.size()) return 6;
	fwrite(&s.prefix, sizeof(s.prefix), 1, out);
	fwrite(tail, sizeof(tail), 1, out);
	if (!list.empty()) fwrite(list.data(), sizeof(uint32_t), list.size(), out);
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
