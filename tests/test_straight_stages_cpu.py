# SPDX-License-Identifier: Apache-2.0
"""The ideal-endpoint and endpoint-format stages work on registers -- literal trip counts over components and partitions,
the partition combination nest without LDS cells (csrc/wave_ideal.h, csrc/wave_format.h) -- and still produce the
reference's bytes: the sequential build of the kernel source against oracle/_ref, one 96x96 image per rewritten branch
(tests/straight_stages_cases.py), and the reference's own output shows that the branch was taken."""
import pytest

import images
import straight_stages_cases as S


@pytest.fixture(scope="module")
def reference(ref):
    return S.Reference(ref)


@pytest.mark.parametrize("name", S.NAMES)
def test_sequential_build_matches_reference(reference, emu, name):
    img, block, quality, profile, _ = reference.cases[name]
    got = emu.compress(img, block, quality, profile=profile)
    bad = images.mismatches(reference.want(name), got)
    assert len(bad) == 0, "%s: blocks differ: %s" % (name, bad[:8])


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.cases()[n][4]])
def test_reference_output_takes_the_branch(reference, name):
    """At least MIN_BLOCKS blocks of the reference's output have the partition count (or the second weight plane) the image
    is there for: the search went through that arm and found it the best."""
    what = reference.cases[name][4]
    count = S.coverage(reference.want(name), what)
    print("%s: %d blocks with %s" % (name, count, what))
    assert count >= S.MIN_BLOCKS, (name, what, count)
