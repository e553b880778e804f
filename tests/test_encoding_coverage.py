# SPDX-License-Identifier: Apache-2.0
"""GPU side of tests/test_encoding_coverage_cpu.py: on every image of the coverage matrix (tests/encoding_cases.py) the
product's kernel -- the build the row names, asserted -- gives the reference's bytes; the rows of the three fixed-context
builds once more on the generic builds (a fresh child process with ASTCENC_AMD_KERNEL=generic), one row per build class on
a run-time specialised build (the generic classes: a context served by a fixed-context build gets no run-time build, with
or without ASTCENC_AMD_KERNEL=generic -- csrc/backend_hip.hip, backend_create), and float edge values through the device's block load.  The CPU module shows from the same
reference bytes which encodings these images reach."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import block_census
import encoding_cases as E
import images
from jit_builds import is_jit, prewarm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def reference(ref):
    return E.Reference(ref)


def _describe(case, want, bad):
    """The differing block indices with their census features (of the reference's bytes)."""
    infos = block_census.block_infos(want, case.block)
    return "%s: %d blocks differ: %s" % (case.id, len(bad), [(int(i), block_census.features(infos[i])) for i in bad[:8]])


@pytest.mark.parametrize("case_id", E.case_ids())
def test_product_matches_reference(reference, product, case_id):
    case = reference.by_id[case_id]
    want = reference.want(case_id)
    got = product.compress(case.image(), case.block, case.quality, profile=case.profile)
    assert product.last_kernel == case.kernel, (case_id, product.last_kernel)
    bad = images.mismatches(want, got)
    assert len(bad) == 0, _describe(case, want, bad)


SCRIPT = r"""
import sys, hashlib
sys.path[:0] = %r
import numpy as np, torch
torch.zeros(1, device="cuda:0")
import astcenc_amd as A
import encoding_cases as E
lib = A.Library(A.LIB_PRODUCT)
for case in E.cases():
    if case.row in E.GENERIC_OF_FIXED:
        data = lib.compress(case.image(), case.block, case.quality, profile=case.profile)
        print("CASE %%s %%s %%s" %% (case.id, lib.last_kernel, hashlib.sha256(np.asarray(data).tobytes()).hexdigest()), flush=True)
"""
PATHS = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle")]


def _fixed_rows_in_a_child(reference, **extra_env):
    """R1 to R3 in a fresh process with the fixed-context builds switched off: [(case, kernel that ran)], after checking
    that every image's bytes are the reference's."""
    env = dict(os.environ, ASTCENC_AMD_KERNEL="generic", **extra_env)
    r = subprocess.run([sys.executable, "-c", SCRIPT % (PATHS,)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split() for ln in r.stdout.split("\n") if ln.startswith("CASE ")]
    expected = [c for c in E.cases() if c.row in E.GENERIC_OF_FIXED]
    assert [ln[1] for ln in lines] == [c.id for c in expected]
    wrong = [case.id for (_, _, _, digest), case in zip(lines, expected)
             if hashlib.sha256(np.asarray(reference.want(case.id)).tobytes()).hexdigest() != digest]
    assert not wrong, wrong
    return [(case, ln[2]) for ln, case in zip(lines, expected)]


def test_fixed_rows_on_the_generic_builds(reference, product):
    """The generic builds give the reference's bytes on the images of the fixed-context rows."""
    for case, kernel in _fixed_rows_in_a_child(reference):
        assert kernel == E.GENERIC_OF_FIXED[case.row], (case.id, kernel)


@pytest.fixture(scope="module")
def jit_cache(built, tmp_path_factory):
    """The run-time builds of JIT_ROWS' contexts, compiled on the CPUs into a cache of this module's."""
    cache = str(tmp_path_factory.mktemp("jit_cache"))
    prewarm(cache, [(E.ROWS[row][0], E.ROWS[row][1], E.ROWS[row][2], 0) for row in E.JIT_ROWS])
    return cache


@pytest.mark.parametrize("row", E.JIT_ROWS)
def test_run_time_builds_match_reference(reference, product, jit_cache, monkeypatch, row):
    """One row per build class through the context's run-time specialised build."""
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", jit_cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    monkeypatch.delenv("ASTCENC_AMD_JIT_OPTIONS", raising=False)
    monkeypatch.delenv("ASTCENC_AMD_JIT_SELF_CHECK", raising=False)
    failures = []
    for case in E.cases():
        if case.row != row:
            continue
        want = reference.want(case.id)
        got = product.compress(case.image(), case.block, case.quality, profile=case.profile, specialize=True)
        assert is_jit(product.last_kernel), (case.id, product.last_kernel)
        bad = images.mismatches(want, got)
        if len(bad):
            failures.append(_describe(case, want, bad))
    assert not failures, failures


# ---- float edge values through load_block (csrc/wave_*.h): med3 clamps on the device, compares in the sequential build -------


@pytest.mark.parametrize("case", E.float_edge_cases(), ids=E.float_edge_id)
def test_float_edge_values(ref, product, case):
    dtype, profile, block, swizzle = case
    img = E.float_edge_image(dtype)
    want = ref.compress(img, block, E.FLOAT_EDGE_QUALITY, profile=profile, swizzle=swizzle)
    got = product.compress(img, block, E.FLOAT_EDGE_QUALITY, profile=profile, swizzle=swizzle)
    bad = images.mismatches(want, got)
    assert len(bad) == 0, "blocks differ: %s" % bad[:8]
