# SPDX-License-Identifier: Apache-2.0
"""GPU side of tests/test_straight_stages_cpu.py: the product's kernels -- the 6x6 -medium fixed-context build, the
run-time-table builds for 6x6 -thorough, HDR and the 10x8 footprint, and one run-time specialised build at 5x5 -medium --
produce the reference's bytes on the images of tests/straight_stages_cases.py."""
import pytest

import images
import straight_stages_cases as S
from jit_builds import compress_both, prewarm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(ref):
    return S.Reference(ref)


@pytest.mark.parametrize("name", [n for n in S.NAMES if n != "footprint_5x5"])
def test_product_matches_reference(reference, product, name):
    img, block, quality, profile, what = reference.cases[name]
    want = reference.want(name)
    if what:
        assert S.coverage(want, what) >= S.MIN_BLOCKS, (name, what)
    got = product.compress(img, block, quality, profile=profile)
    bad = images.mismatches(want, got)
    assert len(bad) == 0, "%s: blocks differ: %s" % (name, bad[:8])


def test_kernel_builds_that_ran(product, reference, A):
    """The cases above reach the builds they are meant for: the fixed 6x6 -medium context, and the generic build for a
    footprint above 64 texels."""
    img, block, quality, profile, _ = reference.cases["rgba"]
    product.compress(img, block, quality, profile=profile)
    assert product.last_kernel == "astc_compress_blocks_ldr_6x6m", product.last_kernel
    img, block, quality, profile, _ = reference.cases["footprint_10x8"]
    product.compress(img, block, quality, profile=profile)
    assert product.last_kernel == "astc_compress_blocks_ldr", product.last_kernel


def test_run_time_build_matches_reference(reference, product, ref, A, tmp_path, monkeypatch):
    """5x5 -medium on its own run-time build (compiled on the CPUs into a cache of this test's, found there by the context)."""
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    img, block, quality, profile, _ = reference.cases["footprint_5x5"]
    prewarm(cache, [(profile, block, quality, 0)])
    bad, name = compress_both(product, ref, A, img, block, quality, profile)
    assert name.startswith("astc_compress_blocks_jit_"), name
    assert bad == 0
