# SPDX-License-Identifier: Apache-2.0
"""Block tickets without a GPU (csrc/block_tickets.h): the header the kernel draws its launch indices with, compiled by g++,
in a simulated drain.

`grid` pullers run the kernel's loop -- heads home, home + 1, ... each until a ticket is past the head's last index -- one
atomic add per step, the steps of the pullers interleaved by a schedule: round-robin, one puller to the end before the next
starts, and random orders.  Homes are dealt round-robin (the dispatcher's placement), all the same (every workgroup on one XCD)
and at random.  For every n and grid: every index in [0, n) is drawn exactly once, nothing else is, and no head ends more than
`grid` past its count (every puller fails once per head and never comes back)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

DRAIN_TEST = r"""
#include "block_tickets.h"
#include <cstdio>
#include <vector>
using namespace astcd;

struct Puller { unsigned int home, dry; bool done; };

static unsigned int rng_state = 2463534242u;
static unsigned int rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// schedule 0: round-robin, 1: one puller after the other, 2..: random; homes 0: p % 8, 1: all 3, 2: random
static int drain(unsigned int n, unsigned int grid, int schedule, int homes)
{
	std::vector<unsigned int> heads(TICKET_BUFFER_BYTES / 4, 0u);
	std::vector<unsigned int> drawn(n, 0u);
	std::vector<Puller> p(grid);
	for (unsigned int i = 0; i < grid; i++) p[i] = { homes == 0 ? i % TICKET_HEADS : homes == 1 ? 3u : rng() % TICKET_HEADS, 0u, false };
	unsigned int live = grid, turn = 0;
	while (live)
	{
		unsigned int i;
		if (schedule == 0) { do { i = turn++ % grid; } while (p[i].done); }
		else if (schedule == 1) { i = 0; while (p[i].done) i++; }
		else { do { i = rng() % grid; } while (p[i].done); }
		// one step of the kernel's loop (kernel_device.h)
		const unsigned int x = ticket_head_after(p[i].home, p[i].dry);
		const unsigned int t = heads[ticket_head_word(x)]++;
		if (t < ticket_head_count(n, x))
		{
			const unsigned int index = ticket_index(t, x);
			if (index >= n) { printf("n %u grid %u: index %u drawn\n", n, grid, index); return 1; }
			drawn[index]++;
		}
		else if (++p[i].dry == TICKET_HEADS) { p[i].done = true; live--; }
	}
	for (unsigned int i = 0; i < n; i++)
		if (drawn[i] != 1) { printf("n %u grid %u schedule %d homes %d: index %u drawn %u times\n", n, grid, schedule, homes, i, drawn[i]); return 1; }
	unsigned int total = 0;
	for (unsigned int x = 0; x < TICKET_HEADS; x++)
	{
		const unsigned int count = ticket_head_count(n, x), end = heads[ticket_head_word(x)];
		total += count;
		if (end < count || end - count > grid) { printf("n %u grid %u: head %u ends at %u, count %u\n", n, grid, x, end, count); return 1; }
		if (end - count != grid) { printf("n %u grid %u: head %u failed %u pullers, not every one once\n", n, grid, x, end - count); return 1; }
	}
	if (total != n) { printf("n %u: the heads count %u indices\n", n, total); return 1; }
	for (size_t w = 0; w < heads.size(); w++)
		if (w % TICKET_HEAD_STRIDE_WORDS != 0 && heads[w] != 0) { printf("word %zu written\n", w); return 1; }
	return 0;
}

int main()
{
	static_assert(TICKET_HEAD_STRIDE_WORDS * 4 == 64 && TICKET_BUFFER_BYTES == 512, "eight heads, each on its own 64-byte line");
	const unsigned int ns[] = { 0, 1, 7, 8, 9, 204, 8191, 8192, 8193, 16385 };
	const unsigned int grids[] = { 1, 8, 24 };
	int bad = 0;
	for (unsigned int n : ns)
		for (unsigned int grid : grids)
			for (int homes = 0; homes < 3; homes++)
				for (int schedule = 0; schedule < 6; schedule++)
					bad |= drain(n, grid, schedule, homes);
	// the counts near the end of the 32-bit range: no overflow in the count or in an index that is handed out
	for (unsigned int x = 0; x < TICKET_HEADS; x++)
	{
		const unsigned int n = 0xFFFFFFFFu, count = ticket_head_count(n, x);
		if (count == 0 || ticket_index(count - 1, x) >= n || (unsigned long long)ticket_index(count - 1, x) + TICKET_HEADS < n) { printf("head %u at n = 2^32 - 1\n", x); bad = 1; }
	}
	printf(bad ? "FAIL\n" : "OK\n");
	return bad;
}
"""


def test_drain_visits_every_index_once(tmp_path):
    src, exe = tmp_path / "drain.cpp", tmp_path / "drain"
    src.write_text(DRAIN_TEST)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
