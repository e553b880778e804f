#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Generate tests/golden/resize_48x40_to_36x30_6x6_medium.npy: the reference encoder's blocks (oracle/_ref, as
make_golden.py uses it) of the image that tests/test_resize.py::test_blocks_equal_the_reference resizes, resized by the numpy
model (tests/resize_model.py).

Run where the reference is built:  python tests/golden/make_resize_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import astcenc_amd as A  # noqa: E402
import oracle_libs as O  # noqa: E402
import resize_model as R  # noqa: E402


def main():
    ref = A.Library(O.LIB_REF_NONE)
    rng = np.random.default_rng(12)                  # the test's _image(np.uint8, (1, 48, 40), 12)
    img = rng.integers(0, 256, (1, 48, 40, 4), dtype=np.uint8)
    img[..., 3][rng.random((1, 48, 40)) < 0.3] = 0
    resized = R.resize(img, (36, 30), R.VOLUME, R.LANCZOS3, R.WRAP)
    blocks = ref.compress(resized[0], (6, 6), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
    np.save(os.path.join(HERE, "resize_48x40_to_36x30_6x6_medium.npy"), blocks)
    print(blocks.shape[0], "blocks")


if __name__ == "__main__":
    main()
