// SPDX-License-Identifier: Apache-2.0
// The table of an image set (astcenc_amd_compress_images_device / astcenc_amd_decompress_images_device) and the lookup that
// maps a work item -- a block of the compressor, a run of blocks of the decoder -- to the entry it belongs to.  One launch
// covers the work items of every entry back to back; the kernel head finds its entry here.
//
// No includes and no HIP types: the header is part of the run-time build's source (kernel_jit.cpp) and is compiled by g++ in
// tests/test_image_set_lookup.py.
//
// Layout in device memory (16-byte aligned), written by the host:
//   ImageSetTable                     count, total
//   unsigned int first[count]         work item at which entry e starts: first[0] = 0, strictly ascending (an entry has >= 1 item)
//   (padding to 16 bytes)
//   Record entries[count]             at image_set_records_offset(count): what the kernel needs of entry e
#pragma once

#if defined(__HIPCC__)
#define ASTC_SET_FN __host__ __device__ inline
#else
#define ASTC_SET_FN inline
#endif

namespace astcd {

struct ImageSetTable {
	unsigned int count;     // entries (>= 1)
	unsigned int total;     // work items of all entries
	unsigned int pad[2];
};

/* Byte offset of first[] and of the entry records from the start of the table. */
ASTC_SET_FN unsigned long long image_set_first_offset() { return sizeof(ImageSetTable); }
ASTC_SET_FN unsigned long long image_set_records_offset(unsigned int count)
{
	return (image_set_first_offset() + 4ull * count + 15ull) & ~15ull;
}

/* The entry work item `item` (< total) belongs to: the largest e with first[e] <= item.  `first` may be a pointer of any
 * address space; with a uniform `item` every step is a scalar load (log2(count) of them, each one dependent on the last). */
template <typename FirstPtr>
ASTC_SET_FN unsigned int image_set_find(FirstPtr first, unsigned int count, unsigned int item)
{
	unsigned int lo = 0, n = count;       // the answer lies in [lo, lo + n)
	while (n > 1)
	{
		const unsigned int half = n >> 1;
		if (first[lo + half] <= item) lo += half;
		n -= half;
	}
	return lo;
}

/* A record of the table, read word by word into a register copy: a record's own copy constructor takes a generic reference,
 * which a pointer to the constant address space (scalar loads) does not bind to. */
template <typename T, typename WordPtr>
ASTC_SET_FN T image_set_record(WordPtr words)
{
	static_assert(sizeof(T) % 4 == 0, "records are whole words");
	unsigned int w[sizeof(T) / 4];
	for (unsigned int i = 0; i < sizeof(T) / 4; i++) w[i] = words[i];
	T v;
	__builtin_memcpy(&v, w, sizeof(T));
	return v;
}

} // namespace astcd
