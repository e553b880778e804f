# SPDX-License-Identifier: Apache-2.0
"""The host side of the adaptive-effort calls (include/astcenc_amd.h): no GPU.

  - tests/harness/block_select_check.cpp: csrc/block_select.h -- the criterion text the selection and merge kernels compile --
    built by g++ into a program of its own with -fsanitize=address,undefined and run on random records and geometries against
    the numpy model of tests/test_block_select.py: e bit for bit (NaNs as NaNs), n, and the predicate, with partial blocks on
    all three axes, 2D footprints over slices, NaN and infinite records, zero weights, thresholds 0 and +inf, and ties.
  - a C program prints the sizes and field offsets of struct astcenc_amd_block_criterion and struct astcenc_amd_adaptive_stats
    for the binding's ctypes layouts to be held against."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import test_block_select as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRY = S.GEOMETRY + [((12, 12, 1), (134, 50, 1)), ((6, 6, 6), (7, 13, 20)), ((5, 4, 1), (23, 9, 4)), ((3, 3, 3), (100, 4, 4))]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    assert shutil.which("g++") is not None, "the CPU suite needs g++ (as the build of oracle/emu does)"
    exe = str(tmp_path_factory.mktemp("select") / "block_select_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"), os.path.join(ROOT, "tests", "harness", "block_select_check.cpp"), "-o", exe],
                   check=True)
    return exe


def run_harness(exe, tmp_path, block, dims, records, weight, threshold):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.array(list(block) + list(dims) + [records.shape[0], 0], dtype=np.uint32).tobytes())
        f.write(np.array(list(weight) + [threshold], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(records, dtype=np.float64).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.fromfile(dst, dtype=np.dtype([("e", "<f8"), ("n", "<u4"), ("selected", "<u4")]))
    assert got.size == records.shape[0]
    return got


@pytest.mark.parametrize("block,dims", GEOMETRY, ids=["%s-%s" % ("x".join(map(str, b)), "x".join(map(str, d))) for b, d in GEOMETRY])
def test_criterion_matches_the_model(harness, tmp_path, block, dims):
    n = S.texels(block, dims)
    for i, pattern in enumerate(S.PATTERNS):
        records, weight, threshold = S.case(pattern, n, 300 + i)
        got = run_harness(harness, tmp_path, block, dims, records, weight, threshold)
        assert np.array_equal(got["n"], n), (pattern, "texels")
        w = np.asarray(weight, dtype=np.float64)
        with np.errstate(all="ignore"):
            e = ((w[0] * records[:, 0] + w[1] * records[:, 1]) + w[2] * records[:, 2]) + w[3] * records[:, 3]
        same = (got["e"].view(np.uint64) == e.view(np.uint64)) | (np.isnan(got["e"]) & np.isnan(e))
        assert same.all(), (pattern, "e", np.flatnonzero(~same)[:8])
        assert np.array_equal(got["selected"].astype(bool), S.model(records, n, weight, threshold)), (pattern, "selected")


def test_rounding_order(harness, tmp_path):
    """Records whose sum depends on the order and on every product being rounded on its own: a fused multiply-add or another
    association gives other bits."""
    rng = np.random.default_rng(11)
    block, dims = (4, 4, 1), (64, 64, 1)
    n = S.texels(block, dims)
    records = rng.random((n.size, 4)) * np.array([1.0, 1e-8, 1e8, 1e-3])
    weight = (1.0 / 3.0, 0.7, 1e-9, 3.3)
    got = run_harness(harness, tmp_path, block, dims, records, weight, 0.02)
    w = np.asarray(weight)
    e = ((w[0] * records[:, 0] + w[1] * records[:, 1]) + w[2] * records[:, 2]) + w[3] * records[:, 3]
    other = (w[0] * records[:, 0] + w[1] * records[:, 1]) + (w[2] * records[:, 2] + w[3] * records[:, 3])
    assert (e != other).any()                       # (the case tells the two orders apart)
    assert np.array_equal(got["e"].view(np.uint64), e.view(np.uint64))


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "astcenc.h"
#include "astcenc_amd.h"
int main(void)
{
	printf("BlockCriterion %zu channel_weight %zu max_mean_squared_error %zu\n", sizeof(struct astcenc_amd_block_criterion),
	       offsetof(struct astcenc_amd_block_criterion, channel_weight), offsetof(struct astcenc_amd_block_criterion, max_mean_squared_error));
	printf("AdaptiveStats %zu blocks %zu selected %zu replaced %zu kernel_ms_base %zu kernel_ms_strong %zu kernel_ms_other %zu\n",
	       sizeof(struct astcenc_amd_adaptive_stats), offsetof(struct astcenc_amd_adaptive_stats, blocks),
	       offsetof(struct astcenc_amd_adaptive_stats, selected), offsetof(struct astcenc_amd_adaptive_stats, replaced),
	       offsetof(struct astcenc_amd_adaptive_stats, kernel_ms_base), offsetof(struct astcenc_amd_adaptive_stats, kernel_ms_strong),
	       offsetof(struct astcenc_amd_adaptive_stats, kernel_ms_other));
	return 0;
}
"""


def test_struct_layouts_match_the_binding(A, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the CPU suite needs a C compiler (as the build of oracle does)"
    src, exe = str(tmp_path / "layout.c"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(LAYOUT_C)
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, struct in zip(lines, (A.BlockCriterion, A.AdaptiveStats)):
        words = line.split()
        assert words[0] == struct.__name__ and int(words[1]) == __import__("ctypes").sizeof(struct), line
        fields = dict(zip(words[2::2], map(int, words[3::2])))
        assert fields == {name: getattr(struct, name).offset for name, _ in struct._fields_}, line


def test_the_binding_names_the_new_calls(A):
    for name in ("astcenc_amd_compress_block_list_device", "astcenc_amd_select_blocks_device", "astcenc_amd_compress_image_adaptive_device"):
        assert name in A.EXPORTS_AMD
        with open(os.path.join(ROOT, "include", "astcenc_amd.h")) as f:
            assert name + "(" in f.read()
