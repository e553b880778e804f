# SPDX-License-Identifier: Apache-2.0
"""The loader stage (csrc/wave_load.h) on texels outside the format's range (tests/input_cases.py), on the CPU.

1. The sequential build of the kernel source gives the reference's bytes over the whole case table: what fails on the GPU
   (tests/test_input_coverage.py) and not here is the device build's.
2. The table proves itself, on the reference alone: a class the clamp makes trivial would test nothing.  Per class and profile
   the scalar and the AVX2 build of the reference agree (the input lies inside the reference's invariance guarantee), more than
   half of the blocks differ from those of the unspoilt base image, `nonfinite` and `huge` hold void-extent blocks of colour
   zero and of another colour, and the square of subnormal reds of `tiny` is encoded otherwise than with a red of zero under the
   LDR profiles.  These are conditions on the inputs: they are never evaluated on the code under test.
3. The two properties a user can rely on, on the reference and on the sequential build:
   (P1) an F16 image and the F32 image of the same values give the same blocks;
   (P2) an image and input_cases.sanitised(image) -- NaN to zero, then clipped to [0, 1] or [0, 65536] -- give the same blocks."""
import numpy as np
import pytest

import input_cases as I
import oracle_libs as O

import astcenc_amd as A  # noqa: E402  (path set up by conftest.py)

PROOF_BLOCK, PROOF_QUALITY = (6, 6), A.PRE_MEDIUM
PROPERTY_CONTEXTS = [(6, 6, A.PRE_MEDIUM), (4, 4, A.PRE_FAST)]


@pytest.fixture(scope="module")
def want(ref):
    return I.Outputs(ref)


@pytest.fixture(scope="module")
def ref_avx2(ref):
    return A.Library(O.LIB_REF_AVX2)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", I.BUILDS)
def test_sequential_build_matches_the_reference(emu, want, build):
    bad = []
    for ctx in I.CONTEXTS[build]:
        for case in I.cases():
            got = I.compress(emu, ctx, I.content(case, ctx[1]), case.swizzle)
            d = I.differing(want.of(ctx, case), got)
            if d:
                bad.append((I.ctx_id(ctx), I.case_id(case), d))
    assert not bad, bad


# ---- 2 ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("profile", list(I.PROFILES))
@pytest.mark.parametrize("cls", I.FLOAT_CLASSES)
def test_the_table_proves_itself(ref, ref_avx2, cls, profile):
    ctx = (I.PROFILES[profile], PROOF_BLOCK, PROOF_QUALITY)
    base = I.compress(ref, ctx, I.image("base"))
    for dtype in ("f16", "f32"):
        img = I.image(cls, dtype)
        blocks = I.compress(ref, ctx, img)
        assert I.differing(blocks, I.compress(ref_avx2, ctx, img)) == 0, dtype
        assert I.differing(blocks, base) > len(base) // 2, dtype
        if cls in ("nonfinite", "huge"):
            colours = set(I.void_extent_colours(blocks))
            assert "00" * 8 in colours and len(colours) >= 2, (dtype, colours)
        if cls == "tiny" and ctx[0] not in I.HDR_PROFILES:
            flushed = np.array(img)
            flushed[:I.REGION, :I.REGION, 0] = 0
            inside = I.compress(ref, ctx, img[:I.REGION, :I.REGION])
            assert I.differing(inside, I.compress(ref, ctx, flushed[:I.REGION, :I.REGION])) == len(inside) == 4, dtype
            assert not I.void_extent_colours(inside), dtype


def test_the_content_is_what_the_table_says():
    """The values the classes are named after are in the arrays handed to the libraries, in both types."""
    for dtype in ("f16", "f32"):
        nf, tiny, huge, rng = (I.image(c, dtype) for c in ("nonfinite", "tiny", "huge", "range"))
        assert -1.0 <= rng.min() < -0.5 and 1.5 < rng.max() <= 2.0
        for img in (nf, huge):
            assert np.isnan(img).any() and np.isposinf(img).any() and np.isneginf(img).any() and (img < 0).any()
        negzero = nf[I.REGION:2 * I.REGION, :I.REGION]
        assert np.signbit(negzero).all() and (negzero == 0).all()
        smallest_normal = np.finfo(tiny.dtype).tiny
        sub = (tiny > 0) & (tiny < smallest_normal)
        assert 0.25 < sub.mean() < 0.4 and sub[:I.REGION, :I.REGION, 0].all()
        assert ((huge > 0) & (huge < np.finfo(huge.dtype).tiny)).any()
        assert huge[np.isfinite(huge)].max() == (np.float32(1e30) if dtype == "f32" else 65504.0)
    f32 = I.image("huge", "f32")
    assert (f32 == 65520.0).any() and (f32 == 70000.0).any()
    assert I.volume("nonfinite", "f16").shape == (I.VOL_D, I.VOL_H, I.VOL_W, 4)


# ---- 3 ----------------------------------------------------------------------------------------------------------------------

LIBS = ["ref", "emu"]


@pytest.fixture(params=LIBS)
def lib(request):
    return request.getfixturevalue(request.param)


@pytest.mark.parametrize("profile", list(I.PROFILES))
def test_a_half_is_the_float_of_the_same_value(lib, profile):
    """(P1)"""
    for bx, by, quality in PROPERTY_CONTEXTS:
        ctx = (I.PROFILES[profile], (bx, by), quality)
        for cls in I.FLOAT_CLASSES:
            for swz in ("rgba", "ba01"):
                img = I.image(cls, "f16")
                assert I.differing(I.compress(lib, ctx, img, swz), I.compress(lib, ctx, I.widened(img), swz)) == 0, (ctx, cls, swz)


@pytest.mark.parametrize("profile", list(I.PROFILES))
def test_an_image_is_its_sanitised_twin(lib, profile):
    """(P2)"""
    for bx, by, quality in PROPERTY_CONTEXTS:
        ctx = (I.PROFILES[profile], (bx, by), quality)
        for cls in I.FLOAT_CLASSES:
            for dtype in ("f16", "f32"):
                img = I.image(cls, dtype)
                twin = I.sanitised(img, ctx[0])
                assert twin.dtype == np.float32 and np.isfinite(twin).all() and twin.min() >= 0
                for swz in ("rgba", "aaar"):
                    assert I.differing(I.compress(lib, ctx, img, swz), I.compress(lib, ctx, twin, swz)) == 0, (ctx, cls, dtype, swz)
