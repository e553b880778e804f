// SPDX-License-Identifier: Apache-2.0
// Block tickets: how a launch of fewer workgroups than blocks deals its launch indices.  A launch over
// `n` blocks whose grid is smaller than n passes the kernel eight ticket heads, zeroed; a workgroup draws ticket t from head x
// with one returning atomic add and compresses launch index 8 * t + x -- the index that blockIdx.x is in a launch of one
// workgroup per block, so everything behind it (the XCD remap, the block list, the image-set lookup) stays what it is.  Head x
// hands out the indices that are x modulo 8: the ones the dispatcher deals to one XCD.  A workgroup starts at the head of the
// XCD it runs on, and moves to the next head (x + 1 modulo 8) when a ticket is past the head's last index; a head that is
// exhausted stays so, which makes eight heads in a row the end of the work.  Nothing waits for anything: the order in which
// workgroups draw changes which of them compresses a block, never the set of blocks.
//
// No includes and no HIP types: the header is part of the run-time build's source (kernel_jit.cpp) and is compiled by g++ in
// tests/test_block_tickets_cpu.py.
#pragma once

#if defined(__HIPCC__)
#define ASTC_TICKET_FN __host__ __device__ inline
#else
#define ASTC_TICKET_FN inline
#endif

namespace astcd {

constexpr unsigned int TICKET_HEADS = 8;
constexpr unsigned int TICKET_HEAD_STRIDE_WORDS = 16;      // one head per 64-byte line
constexpr unsigned int TICKET_BUFFER_BYTES = TICKET_HEADS * TICKET_HEAD_STRIDE_WORDS * 4;

/* The word of head x in the ticket buffer. */
ASTC_TICKET_FN unsigned int ticket_head_word(unsigned int x) { return x * TICKET_HEAD_STRIDE_WORDS; }

/* Tickets of head x that name a launch index below n: the indices x, x + 8, ... */
ASTC_TICKET_FN unsigned int ticket_head_count(unsigned int n, unsigned int x)
{
	return n > x ? (n - x - 1u) / TICKET_HEADS + 1u : 0u;
}

/* The launch index of ticket t of head x (t < ticket_head_count(n, x): no overflow for any 32-bit n). */
ASTC_TICKET_FN unsigned int ticket_index(unsigned int t, unsigned int x) { return TICKET_HEADS * t + x; }

/* The head a workgroup whose home is `home` tries after `dry` exhausted ones (dry < TICKET_HEADS). */
ASTC_TICKET_FN unsigned int ticket_head_after(unsigned int home, unsigned int dry) { return (home + dry) % TICKET_HEADS; }

} // namespace astcd
