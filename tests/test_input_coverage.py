# SPDX-License-Identifier: Apache-2.0
"""The loader stage (csrc/wave_load.h, load_block) of every HIP build of the compression kernel on texels outside the format's
range: the case table of tests/input_cases.py, byte for byte against the reference (oracle/_ref).  Bytes are equal or the test
fails; tests/test_input_coverage_cpu.py shows on the reference that the table bites and that the sequential build of the same
source already gives these bytes, so what fails here is the device build's (v_med3_f32 in v_clamp, half_to_float on subnormals,
the masks of float_to_lns, `(int)e` on the way to the void-extent colour).

(a) the host API over the whole table, one test per build of the kernel, the kernel that ran asserted per case;
(b) the two properties a user can rely on, on the product alone: an F16 image and the F32 image of the same values give the same
    blocks (P1), an image and input_cases.sanitised(image) give the same blocks (P2);
(c) the flags that read the loaded block -- USE_ALPHA_WEIGHT scales the channel weights by the block's largest alpha, which is
    then a clamped infinity or a NaN;
(d) the alpha-scale pre-pass with NaN and infinite alpha (a NaN poisons the prefix sums of its tile as in the reference);
(e) the device entry points, each of which fills an image descriptor of its own: device image, device volume, image set,
    block list.
(c) and (d) run on the sequential build too (not marked gpu).

Not here, on purpose:
  - the adaptive calls and the quality / metrics kernels on non-finite originals: the reference's error sums become NaN, and
    there is no defined byte contract to compare against;
  - the mip-chain calls: their filters have infinity cases of their own (tests/test_mip_filter.py), and their compression step
    is the image-set path of (e)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import input_cases as I

import astcenc_amd as A  # noqa: E402  (path set up by conftest.py)

gpu = pytest.mark.gpu
LIBS = [pytest.param("emu", id="emu"), pytest.param("product", id="hip", marks=gpu)]
CANARY = 0xA5


@pytest.fixture(params=LIBS)
def lib(request):
    return request.getfixturevalue(request.param)


@pytest.fixture(scope="module")
def want(ref):
    return I.Outputs(ref)


# ---- (a) ------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("build", I.BUILDS)
def test_every_build_loads_every_class(product, want, build):
    bad, cases, blocks = [], 0, 0
    for ctx in I.CONTEXTS[build]:
        for case in I.cases():
            got = I.compress(product, ctx, I.content(case, ctx[1]), case.swizzle)
            assert product.last_kernel == I.kernel_of(build, ctx), (I.ctx_id(ctx), I.case_id(case), product.last_kernel)
            expect = want.of(ctx, case)
            cases, blocks = cases + 1, blocks + len(expect)
            d = I.differing(expect, got)
            if d:
                bad.append((I.ctx_id(ctx), I.case_id(case), d))
    print("(a) %-9s %3d cases, %5d blocks compared, %d cases differ" % (build, cases, blocks, len(bad)))
    assert not bad, bad


# ---- (b) ------------------------------------------------------------------------------------------------------------------
PROPERTY_CONTEXTS = [("ldr_6x6m", I.CONTEXTS["ldr_6x6m"][0]), ("ldr_8x8t", I.CONTEXTS["ldr_8x8t"][0]), ("hdr_6x6m", I.CONTEXTS["hdr_6x6m"][0]),
                     ("hdr", I.CONTEXTS["hdr"][0]), ("ldr", I.CONTEXTS["ldr"][0]), ("3d", I.CONTEXTS["3d"][1])]


@gpu
@pytest.mark.parametrize("build,ctx", PROPERTY_CONTEXTS, ids=[b for b, _ in PROPERTY_CONTEXTS])
def test_properties_on_the_product(product, build, ctx):
    bad = []
    for cls in I.FLOAT_CLASSES:
        for swz in ("rgba", "ba01"):
            got = {}
            for dtype in ("f16", "f32"):
                img = I.content(I.Case(cls, dtype, swz), ctx[1])
                got[dtype] = I.compress(product, ctx, img, swz)
                assert product.last_kernel == I.kernel_of(build, ctx), (cls, dtype, product.last_kernel)
                if I.differing(got[dtype], I.compress(product, ctx, I.sanitised(img, ctx[0]), swz)):
                    bad.append(("P2", cls, dtype, swz))
            half = I.content(I.Case(cls, "f16", swz), ctx[1])
            if I.differing(got["f16"], I.compress(product, ctx, I.widened(half), swz)):
                bad.append(("P1", cls, swz))
    assert not bad, bad


# ---- (c) ------------------------------------------------------------------------------------------------------------------
FLAGS = ["FLG_USE_ALPHA_WEIGHT", "FLG_USE_PERCEPTUAL", "FLG_MAP_NORMAL", "FLG_MAP_RGBM", "FLG_USE_DECODE_UNORM8"]


@pytest.mark.parametrize("flag", FLAGS)
def test_flags_on_non_finite_texels(lib, ref, flag):
    ctx = (A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    img = I.image("nonfinite", "f32")
    for swz in ("rgba", "ba01"):
        expect = I.compress(ref, ctx, img, swz, flags=getattr(A, flag))
        got = I.compress(lib, ctx, img, swz, flags=getattr(A, flag))
        if lib.has_amd and lib.backend_name().startswith("hip"):
            assert lib.last_kernel == I.K + "ldr64", lib.last_kernel      # (a flag changes a record: no fixed-context build)
        assert I.differing(expect, got) == 0, swz


# ---- (d) ------------------------------------------------------------------------------------------------------------------

def _alpha_image():
    img = np.array(I.image("nonfinite", "f32", 70, 66))
    img[-30:, -30:, 3] = 0.0                         # a transparent corner: blocks the pre-pass turns into constant zero
    return img


@pytest.mark.parametrize("radius", [1, 3])
def test_alpha_scale_with_non_finite_alpha(lib, ref, radius):
    ctx = (A.PRF_LDR, (6, 6), A.PRE_FAST)
    img = _alpha_image()
    assert not np.isfinite(img[..., 3]).all()

    def tweak(cfg):
        cfg.a_scale_radius = radius
    expect = I.compress(ref, ctx, img, tweak=tweak)
    assert I.differing(expect, I.compress(ref, ctx, img)) > 0, "the image must contain blocks that the alpha test skips"
    assert I.differing(expect, I.compress(lib, ctx, img, tweak=tweak)) == 0


# ---- (e) ------------------------------------------------------------------------------------------------------------------
ENTRY_CONTEXTS = [(A.PRF_LDR, (5, 4), A.PRE_MEDIUM), (A.PRF_HDR, (8, 8), A.PRE_MEDIUM)]
ENTRY_VOLUME_CONTEXTS = ENTRY_CONTEXTS + [(A.PRF_LDR, (4, 4, 4), A.PRE_MEDIUM)]
ENTRY_KERNELS = {ENTRY_CONTEXTS[0]: I.K + "ldr64", ENTRY_CONTEXTS[1]: I.K + "hdr64", ENTRY_VOLUME_CONTEXTS[2]: I.K + "ldr64"}
ENTRY_CASES = [I.Case(cls, dtype, "ba01") for cls in ("nonfinite", "huge") for dtype in ("f16", "f32")]
TYPES = {np.dtype(np.uint8): A.TYPE_U8, np.dtype(np.float16): A.TYPE_F16, np.dtype(np.float32): A.TYPE_F32}


@contextlib.contextmanager
def _context(product, ctx):
    """A context of the product for one of ENTRY_*_CONTEXTS, the kernel it launches asserted."""
    profile, block, quality = ctx
    err, cfg = product.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, quality, 0)
    assert err == 0
    err, handle = product.context_alloc(cfg, 1)
    assert err == 0, product.error_string(err)
    try:
        name = product.lib.astcenc_amd_context_kernel_name(handle).decode()
        assert name == ENTRY_KERNELS[ctx], (I.ctx_id(ctx), name)
        yield handle
    finally:
        product.context_free(handle)


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _fresh(blocks):
    import torch
    return torch.full((blocks * 16,), CANARY, dtype=torch.uint8, device="cuda")


@gpu
@pytest.mark.parametrize("ctx", ENTRY_CONTEXTS, ids=I.ctx_id)
def test_device_image_entry_point(product, want, ctx):
    with _context(product, ctx) as handle:
        for case in ENTRY_CASES:
            img, expect = I.image(case.cls, case.dtype), want.of(ctx, case)
            t_img, out = _dev(img), _fresh(len(expect))
            err = product.lib.astcenc_amd_compress_image_device(handle, t_img.data_ptr(), img.shape[1], img.shape[0], TYPES[img.dtype],
                                                                C.byref(A.Swizzle(*I.SWIZZLES[case.swizzle])), out.data_ptr(), out.numel(),
                                                                A.torch_stream(), None)
            assert err == 0, product.error_string(err)
            assert I.differing(expect, out.cpu().numpy()) == 0, I.case_id(case)


@gpu
@pytest.mark.parametrize("ctx", ENTRY_VOLUME_CONTEXTS, ids=I.ctx_id)
def test_device_volume_entry_point(product, ref, ctx):
    """The seven-slice stack under a 2D footprint (every slice through the general loader) and as a volume under 4x4x4."""
    with _context(product, ctx) as handle:
        for case in ENTRY_CASES:
            vol = I.volume(case.cls, case.dtype)
            expect = I.compress(ref, ctx, vol, case.swizzle)
            t_vol, out = _dev(vol), _fresh(len(expect))
            err = product.lib.astcenc_amd_compress_volume_device(handle, t_vol.data_ptr(), vol.shape[2], vol.shape[1], vol.shape[0],
                                                                 TYPES[vol.dtype], C.byref(A.Swizzle(*I.SWIZZLES[case.swizzle])),
                                                                 out.data_ptr(), out.numel(), A.torch_stream(), None)
            assert err == 0, product.error_string(err)
            assert I.differing(expect, out.cpu().numpy()) == 0, I.case_id(case)


def _set_entries():
    """Six entries of three types, each with a swizzle and a size of its own: (array, swizzle)."""
    nonfinite16, huge32, u8 = I.image("nonfinite", "f16"), I.image("huge", "f32"), I.image("u8", "u8")
    return [(I.image("nonfinite", "f32"), "ba01"), (I.image("huge", "f16"), "aaar"), (u8, "ba01"),
            (np.ascontiguousarray(nonfinite16[10:15, 8:15]), "rgba"),         # 7 x 5 across the NaN and +Inf squares and the noise
            (np.ascontiguousarray(huge32[:1, :1]), "rgba"),                   # 1 x 1: (70000, 1e9, +Inf, 1)
            (np.ascontiguousarray(u8[3:8, 2:9]), "rgba")]


@gpu
@pytest.mark.parametrize("ctx", ENTRY_CONTEXTS, ids=I.ctx_id)
def test_image_set_entry_point(product, ref, ctx):
    entries = _set_entries()
    assert [e[0].shape[:2] for e in entries] == [(I.H, I.W)] * 3 + [(5, 7), (1, 1), (5, 7)]
    assert {e[0].dtype.name for e in entries} == {"uint8", "float16", "float32"}
    expect = [I.compress(ref, ctx, img, swz) for img, swz in entries]
    with _context(product, ctx) as handle:
        t_imgs = [_dev(img) for img, _ in entries]
        outs = [_fresh(len(e)) for e in expect]
        err = product.compress_images_device(handle, [(t, o, I.SWIZZLES[swz]) for t, o, (_, swz) in zip(t_imgs, outs, entries)])
        assert err == 0, product.error_string(err)
        bad = [(k, I.differing(e, o.cpu().numpy())) for k, (e, o) in enumerate(zip(expect, outs))]
    assert not [b for b in bad if b[1]], bad


@gpu
@pytest.mark.parametrize("ctx", ENTRY_CONTEXTS, ids=I.ctx_id)
def test_block_list_entry_point(product, want, ctx):
    """Every block index in descending order, then every third: the listed blocks are the reference's, the others the canary."""
    import torch
    with _context(product, ctx) as handle:
        for case in ENTRY_CASES:
            img, expect = I.image(case.cls, case.dtype), want.of(ctx, case)
            n = len(expect)
            t_img = _dev(img)
            for name, listed in (("descending", np.arange(n)[::-1].copy()), ("every third", np.arange(n)[::3].copy())):
                out = _fresh(n)
                err = product.compress_block_list_device(handle, t_img, torch.from_numpy(listed.astype(np.int32)).cuda(), out,
                                                         swizzle=I.SWIZZLES[case.swizzle])
                assert err == 0, product.error_string(err)
                full = np.full((n, 16), CANARY, dtype=np.uint8)
                full[listed] = expect[listed]
                assert I.differing(full, out.cpu().numpy()) == 0, (I.case_id(case), name)
