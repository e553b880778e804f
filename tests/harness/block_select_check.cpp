// SPDX-License-Identifier: Apache-2.0
// Host harness of tests/test_adaptive_cpu.py: the criterion of csrc/block_select.h -- the text the selection and merge kernels
// compile -- evaluated over the records of a file, for a numpy model to compare with.
//   block_select_check <in> <out>
//   in : uint32 block_x, block_y, block_z, dim_x, dim_y, dim_z, blocks, 0; double weight[4], threshold; double records[blocks][4]
//   out: per block  double e; uint32 n; uint32 selected
#include "block_select.h"

#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char** argv)
{
	if (argc != 3) return 2;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	uint32_t head[8];
	double crit[5];
	if (fread(head, sizeof(head), 1, in) != 1 || fread(crit, sizeof(crit), 1, in) != 1) return 3;
	const uint32_t blocks = head[6];
	std::vector<double> records((size_t)blocks * 4);
	if (blocks && fread(records.data(), sizeof(double), records.size(), in) != records.size()) return 3;
	for (uint32_t b = 0; b < blocks; b++)
	{
		const double* s = &records[(size_t)b * 4];
		const double e = astcd::block_select_error(crit, s[0], s[1], s[2], s[3]);
		const uint32_t n = astcd::block_select_texels(b, head[3], head[4], head[5], head[0], head[1], head[2]);
		const uint32_t selected = astcd::block_select_test(e, crit[4], n) ? 1u : 0u;
		fwrite(&e, sizeof(e), 1, out);
		fwrite(&n, sizeof(n), 1, out);
		fwrite(&selected, sizeof(selected), 1, out);
	}
	fclose(in);
	return fclose(out) == 0 ? 0 : 4;
}
