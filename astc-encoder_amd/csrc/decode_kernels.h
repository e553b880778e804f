// SPDX-License-Identifier: Apache-2.0
// What the kernels over a table share on either side of the launch (kernel_decode.hip, kernel_decode_scaled.hip,
// kernel_decode_sample.hip, kernel_decode_lod.hip, kernel_quality.hip): the kernel head that maps a work item to its record, the
// test limit on a grid, the loop of launches that covers a table's work items and the pick of a kernel's build by tensor type
// and layout.  HIP source -- address spaces, hipLaunchKernelGGL -- so included by .hip files only; decode_table.h is the part
// that g++ compiles too.
#pragma once
#include "decode_table.h"
#include <hip/hip_runtime.h>
#include <cstdlib>

namespace astcd { inline namespace ASTC_VARIANT {

typedef const __attribute__((address_space(4))) uint8_t* constant_bytes;
typedef const __attribute__((address_space(4))) uint32_t* constant_words;

/* The kernel head: the record of the entry that work item `item` (uniform, < total) of the table belongs to, found in first[]
 * (image_set.h) and read word by word -- all of it scalar loads from the constant address space -- and, in `local`, the item's
 * number within that entry. */
template <class Record>
__device__ inline Record decode_table_item(const ImageSetTable* __restrict__ set, uint32_t item, uint32_t& local)
{
	const constant_bytes t = (constant_bytes)reinterpret_cast<uintptr_t>(set);
	const uint32_t count = reinterpret_cast<const __attribute__((address_space(4))) ImageSetTable*>(t)->count;
	const constant_words first = reinterpret_cast<constant_words>(t + image_set_first_offset());
	const uint32_t e = image_set_find(first, count, item);
	const Record rec = image_set_record<Record>(reinterpret_cast<constant_words>(t + image_set_records_offset(count) + (size_t)e * sizeof(Record)));
	local = item - first[e];
	return rec;
}

/* ASTCENC_AMD_DECODE_GRID_LIMIT: a smaller limit on a launch for the tests, which cannot allocate what it takes to exceed the
 * real one (a 262 144-row image, 2^26 runs).  The variable's value where it is 1 .. below - 1, else `normal`. */
inline uint32_t decode_grid_limit(uint32_t normal, long below = 65535)
{
	const char* e = getenv("ASTCENC_AMD_DECODE_GRID_LIMIT");
	const long v = e ? strtol(e, nullptr, 10) : 0;
	return v >= 1 && v < below ? (uint32_t)v : normal;
}

/* Work items [0, total) of the table at d_table, one wavefront each on a 1D grid: one launch unless they exceed the grid -- at
 * most 2^32 - 1 threads in all, i.e. 2^26 - 1 wavefronts of 64 (or the test limit) -- and every launch told where its items
 * start. */
typedef void (*DecodeTableKernel)(const ImageSetTable*, uint32_t);

inline int decode_table_launch(DecodeTableKernel kernel, const void* d_table, uint32_t total, void* stream)
{
	static const uint32_t limit = decode_grid_limit(0xFFFFFFFFu / 64u);
	const ImageSetTable* set = static_cast<const ImageSetTable*>(d_table);
	for (uint32_t item0 = 0; item0 < total; item0 += limit)
	{
		const uint32_t n = total - item0 < limit ? total - item0 : limit;
		hipLaunchKernelGGL(kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), set, item0);
	}
	return (int)hipGetLastError();
}

/* The builds of a kernel template per tensor type and layout (astcenc_amd_tensor_type / _layout), which hold for a call ... */
#define DECODE_TENSOR_BUILDS(kernel) { { kernel<0, 0>, kernel<0, 1> }, { kernel<1, 0>, kernel<1, 1> }, { kernel<2, 0>, kernel<2, 1> } }

/* ... and the launch of the one a table was built for. */
inline int decode_table_launch(const DecodeTableKernel (&builds)[3][2], uint32_t type, uint32_t layout, const void* d_table, uint32_t total, void* stream)
{
	if (type > 2 || layout > 1) return (int)hipErrorInvalidValue;
	return decode_table_launch(builds[type][layout], d_table, total, stream);
}

} } // namespace astcd::ASTC_VARIANT
