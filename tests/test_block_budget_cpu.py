# SPDX-License-Identifier: Apache-2.0
"""The host side of the image-set forms of the adaptive-effort calls (include/astcenc_amd.h): no GPU.

  - tests/harness/block_budget_check.cpp: csrc/block_budget.h -- the text the set selection kernels compile -- built by g++ into a
    program of its own with -ffp-contract=off -fsanitize=address,undefined and run on the sets and patterns of
    tests/test_block_select_set.py and on random sets, against that file's numpy model: every block's key bit for bit, its
    candidate flag and its entry, and the sequential form of the radix select (cutoff key and r), whose list, counts and cutoff
    must be the model's for every budget.
  - a C program prints the size and field offsets of struct astcenc_amd_adaptive_set_stats for the binding's ctypes layout to be
    held against, and the binding names the three new calls."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_block_select_set as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = T.NONE


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which("g++") is not None, "the CPU suite needs g++ (as the build of oracle/emu does)"
    exe = str(tmp_path_factory.mktemp("budget") / "block_budget_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"), os.path.join(ROOT, "tests", "harness", "block_budget_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_harness(exe, tmp_path, block, dims, records, weight, threshold, max_blocks):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array(list(block) + [len(dims), max_blocks, 0, 0, 0], dtype=np.uint32).tobytes())
        f.write(np.array(list(weight) + [threshold], dtype=np.float64).tobytes())
        f.write(np.array(dims, dtype=np.uint32).tobytes())
        f.write(np.ascontiguousarray(records, dtype=np.float64).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    blocks = records.shape[0]
    per_block = np.dtype([("key", "<u8"), ("candidate", "<u4"), ("entry", "<u4")])
    raw = open(dst, "rb").read()
    got = np.frombuffer(raw[:blocks * per_block.itemsize], dtype=per_block)
    tail = raw[blocks * per_block.itemsize:]
    cutoff = int(np.frombuffer(tail[:8], dtype="<u8")[0])
    r, candidates, selected, _ = (int(v) for v in np.frombuffer(tail[8:24], dtype="<u4"))
    chosen = np.frombuffer(tail[24:], dtype="<u4")
    assert chosen.size == selected
    return got, cutoff, r, candidates, chosen


def check(harness, tmp_path, block, dims, pattern, seed):
    n = T.set_texels(block, dims)
    records, weight, threshold = T.case(pattern, n, seed)
    cand, key = T.keys_model(records, n, weight, threshold)
    key_bits = np.where(cand, key.view(np.uint64), np.uint64(0))
    c = int(cand.sum())
    for max_blocks in T.budgets(c):
        what = (block, len(dims), pattern, max_blocks)
        got, cutoff, r, candidates, chosen = run_harness(harness, tmp_path, block, dims, records, weight, threshold, max_blocks)
        assert np.array_equal(got["key"], key_bits), what
        assert np.array_equal(got["candidate"].astype(bool), cand), what
        assert np.array_equal(got["entry"], T.set_entry_of(block, dims)), what
        want, _ = T.model(records, n, weight, threshold, max_blocks)
        assert candidates == c and np.array_equal(chosen, want), what
        if max_blocks != NONE and 0 < max_blocks < c:
            # the cutoff is the smallest selected key, r the selected blocks that have it
            assert cutoff == int(key_bits[want].min()) and r == int((key_bits[want] == cutoff).sum()) and r >= 1, what
        elif max_blocks != 0:
            assert cutoff == 0 and r == 0, what
    return c


@pytest.mark.parametrize("name", [s for s in T.SETS if s != "many"])
def test_header_matches_the_model(harness, tmp_path, name):
    block, dims = T.SETS[name]
    for i, pattern in enumerate(T.PATTERNS):
        c = check(harness, tmp_path, block, dims, pattern, 500 + i)
        if pattern in ("none", "threshold_inf"):
            assert c == 0
        elif T.set_texels(block, dims).size >= 60:
            assert c >= 8, (name, pattern)


def test_random_sets(harness, tmp_path):
    rng = np.random.default_rng(21)
    for trial in range(6):
        block = [(4, 4, 1), (6, 6, 1), (5, 4, 1), (3, 3, 3), (12, 12, 1), (6, 5, 5)][trial]
        dims = [tuple(int(v) for v in rng.integers(1, 40, 3)) for _ in range(int(rng.integers(1, 12)))]
        for pattern in ("distinct", "tie", "low_bits", "exponents", "nan"):
            check(harness, tmp_path, block, dims, pattern, 900 + trial)


def test_model_cases_are_what_they_claim():
    """The properties tests/test_block_select_set.py asserts of its own cases on the GPU, here without one."""
    T.test_set_geometry()
    for name in ("chain_50x45", "seams", "many"):
        block, dims = T.SETS[name]
        n = T.set_texels(block, dims)
        records, weight, threshold = T.case("tie", n, 500 + T.PATTERNS.index("tie"))
        cand, key = T.keys_model(records, n, weight, threshold)
        c, above, tied = int(cand.sum()), int((key[cand] > 0.5).sum()), np.flatnonzero(cand & (key == 0.5))
        assert above < c // 2 < above + tied.size, (name, above, tied.size, c)
        if name == "seams":         # (nearly all of its blocks are full: n tells nothing apart there)
            continue
        records, weight, threshold = T.case("by_mean", n, 500 + T.PATTERNS.index("by_mean"))
        cand, key = T.keys_model(records, n, weight, threshold)
        index = np.flatnonzero(cand)
        c = index.size
        by_e = np.sort(index[np.argsort(-records[index, 0], kind="stable")[:c // 2]])
        assert not np.array_equal(by_e, T.model(records, n, weight, threshold, c // 2)[0]), name


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "astcenc.h"
#include "astcenc_amd.h"
int main(void)
{
	printf("AdaptiveSetStats %zu blocks %zu candidates %zu selected %zu replaced %zu kernel_ms_base %zu kernel_ms_strong %zu kernel_ms_other %zu\n",
	       sizeof(struct astcenc_amd_adaptive_set_stats), offsetof(struct astcenc_amd_adaptive_set_stats, blocks),
	       offsetof(struct astcenc_amd_adaptive_set_stats, candidates), offsetof(struct astcenc_amd_adaptive_set_stats, selected),
	       offsetof(struct astcenc_amd_adaptive_set_stats, replaced), offsetof(struct astcenc_amd_adaptive_set_stats, kernel_ms_base),
	       offsetof(struct astcenc_amd_adaptive_set_stats, kernel_ms_strong), offsetof(struct astcenc_amd_adaptive_set_stats, kernel_ms_other));
	printf("budget %u\n", ASTCENC_AMD_NO_BLOCK_BUDGET);
	return 0;
}
"""


def test_struct_layout_matches_the_binding(A, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the CPU suite needs a C compiler (as the build of oracle does)"
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT_C)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    words = lines[0].split()
    struct = A.AdaptiveSetStats
    assert words[0] == struct.__name__ and int(words[1]) == C.sizeof(struct), lines[0]
    fields = dict(zip(words[2::2], map(int, words[3::2])))
    assert fields == {name: getattr(struct, name).offset for name, _ in struct._fields_}, lines[0]
    assert int(lines[1].split()[1]) == A.NO_BLOCK_BUDGET == NONE


def test_the_binding_names_the_new_calls(A):
    with open(os.path.join(ROOT, "include", "astcenc_amd.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "astc-encoder_amd", "exports.map")) as f:
        assert "astcenc_*" in f.read()
    for name in ("astcenc_amd_select_blocks_set_device", "astcenc_amd_compress_block_list_set_device", "astcenc_amd_compress_images_adaptive_device"):
        assert name in A.EXPORTS_AMD and name + "(" in header
    assert hasattr(A.Library, "compress_mip_chain_adaptive")
