# SPDX-License-Identifier: Apache-2.0
"""bench.py builds its input image in bands of rows on several host threads (make_image); the bands must join into the very
bytes of the binding's one-call generators, which is what every earlier bench run compressed."""
import numpy as np
import pytest

import bench


@pytest.mark.parametrize("hdr", [False, True])
@pytest.mark.parametrize("seed", [0x9E3779B1, 0x9E3779B2])
def test_banded_image_matches_the_binding(A, hdr, seed):
    cfg = dict(bench.CONFIGS["c4" if hdr else "c2"], size=300)
    got = bench.make_image(cfg, seed, band=64)                   # 300 rows: four full bands and a short one
    want = (A.synthetic_hdr_image if hdr else A.synthetic_image)(300, 300, seed)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize("hdr", [False, True])
def test_rows_far_from_the_origin(A, hdr):
    """The coordinates of an 8192^2 image: the last columns of its first rows, the first columns of its last rows."""
    gen = A.synthetic_hdr_image if hdr else A.synthetic_image
    seed = 0x9E3779B1
    wide = bench.synthetic_rows(8192, 0, 40, seed, hdr)
    assert np.array_equal(wide.view(np.uint8), gen(8192, 40, seed).view(np.uint8))
    tall = bench.synthetic_rows(96, 8192 - 200, 8192, seed, hdr)
    assert np.array_equal(tall.view(np.uint8), gen(96, 8192, seed)[-200:].view(np.uint8))
