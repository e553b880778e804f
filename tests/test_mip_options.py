# SPDX-License-Identifier: Apache-2.0
"""Mip chain options on the GPU (astcenc_amd_generate_mip_chain_ex_device / astcenc_amd_compress_mip_chain_ex_device).

Every level equals the numpy model (tests/mip_options_model.py: levels(options) == post(levels(no options))) for NORMALIZE,
ALPHA_COVERAGE and both, for U8, F16 and F32, for 2D images, arrays and volumes; all 2^24 RGB8 triples are renormalised on the
device; coverage holds on every surface; null options and flags == 0 give the plain calls' bytes; compressed levels equal the
volume call on the model's levels (and the reference's on one small chain); bad options write nothing and are named in the log;
the call keeps stream order on a side stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model_3d as V  # noqa: E402
import mip_options_model as P  # noqa: E402

BOTH = P.NORMALIZE | P.ALPHA_COVERAGE


def _ctx(lib, profile, block, quality=None):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality if quality is not None else 0.0, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(kind, shape, seed, alpha="random"):
    """[Z, H, W, 4] of uint8 / float16 / float32: RGB a noisy normal map, alpha by `alpha`."""
    rng = np.random.default_rng(seed)
    z, h, w = shape
    n = rng.standard_normal((z, h, w, 3)) * 0.3 + np.array([0.0, 0.0, 1.0])
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    rgb = (n + 1.0) / 2.0
    if alpha == "random":
        a = rng.random((z, h, w))
    elif alpha == "ties":
        a = rng.integers(0, 4, (z, h, w)) / 3.0                       # four values only
    elif alpha == "zero":
        a = np.zeros((z, h, w))
    elif alpha == "none":                                             # nothing covered at level 0: k == 0 everywhere
        a = rng.random((z, h, w)) * 0.3
    else:                                                             # per layer coverage: layer l has alpha l / z-ish
        a = np.clip(rng.random((z, h, w)) * 0.5 + (np.arange(z) / max(z - 1, 1))[:, None, None] * 0.6, 0, 1)
    v = np.concatenate([rgb, a[..., None]], axis=-1)
    if kind == "u8":
        return np.clip(np.floor(v * 255.0 + 0.5), 0, 255).astype(np.uint8)
    return v.astype(np.float16 if kind == "f16" else np.float32)


def _same(g, m):
    g = np.ascontiguousarray(g)
    return g.shape == m.shape and g.tobytes() == np.ascontiguousarray(m).tobytes()


def _check_chain(product, ctx, img, kind, flags, cutoff=0.5, levels=0):
    got = product.generate_mip_chain_ex_device(ctx, _dev(img), kind, levels, (flags, cutoff))
    torch.cuda.synchronize()
    want = P.chain(img, kind, flags, cutoff, levels)
    assert len(got) == len(want)
    got = [g.cpu().numpy() for g in got]
    for i, (g, m) in enumerate(zip(got, want)):
        bad = int((g.view(np.uint8).reshape(-1, 4 * g.itemsize) != m.view(np.uint8).reshape(-1, 4 * m.itemsize)).any(axis=1).sum()) \
            if g.shape == m.shape else -1
        assert bad == 0, (img.dtype, img.shape, kind, flags, cutoff, "level %d: %d texels differ" % (i, bad))
    return got


def _coverage_holds(levels, kind, cutoff):
    """Every surface of levels 1 .. n-1 covers at least the target count of texels."""
    top = levels[0]
    layers = top.shape[0] if kind == P.ARRAY else 1
    for l in range(layers):
        t0 = top[l] if kind == P.ARRAY else top
        c0, n0 = int(P.covered(t0[..., 3], cutoff).sum()), t0[..., 3].size
        for lv in levels[1:]:
            s = lv[l] if kind == P.ARRAY else lv
            k = P.target(c0, s[..., 3].size, n0)
            assert int(P.covered(s[..., 3], cutoff).sum()) >= k, (l, s.shape, k)


SHAPES = [("2d", P.VOLUME, (1, 37, 23)), ("2d", P.VOLUME, (1, 512, 256)), ("array", P.ARRAY, (6, 33, 17)),
          ("array", P.ARRAY, (3, 130, 66)), ("volume", P.VOLUME, (9, 33, 17)), ("volume", P.VOLUME, (32, 64, 48))]


@pytest.mark.parametrize("kind", ["u8", "f16", "f32"])
def test_normalize_matches_model(product, A, kind):
    ctx = _ctx(product, A.PRF_HDR if kind != "u8" else A.PRF_LDR, (6, 6))
    try:
        for what, mk, shape in SHAPES:
            _check_chain(product, ctx, _image(kind, shape, len(what) + shape[0]), mk, P.NORMALIZE)
    finally:
        product.context_free(ctx)


def test_normalize_every_u8_triple_on_the_device(product, A):
    """An 8192^2 level 0 of 2 x 2 quads of all 2^24 RGB triples: level 1 holds each triple once, renormalised as the model."""
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        i = torch.arange(1 << 24, dtype=torch.int32, device="cuda")
        quads = torch.stack([i & 0xFF, (i >> 8) & 0xFF, (i >> 16) & 0xFF, torch.full_like(i, 200)], dim=-1).to(torch.uint8)
        quads = quads.view(4096, 4096, 4)
        top = quads.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1).contiguous()[None]
        del i
        torch.cuda.synchronize()               # (a null stream handle is the context's own stream: top must be complete)
        got = product.generate_mip_chain_ex_device(ctx, top, A.MIP_VOLUME, 2, (A.MIP_NORMALIZE, 0.0))
        torch.cuda.synchronize()
        lv1 = got[1][0].cpu().numpy()
        q = quads.cpu().numpy()
        assert np.array_equal(lv1[..., 3], q[..., 3])
        want = P.normalize_u8(q[..., :3])
        bad = int((lv1[..., :3] != want).any(axis=-1).sum())
        assert bad == 0, "%d of 2^24 triples differ" % bad
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("kind", ["u8", "f16", "f32"])
def test_alpha_coverage_matches_model(product, A, kind):
    ctx = _ctx(product, A.PRF_HDR if kind != "u8" else A.PRF_LDR, (6, 6))
    try:
        cases = [("ties", P.VOLUME, (1, 64, 64), 0.5), ("ties", P.VOLUME, (1, 37, 23), 1.0 / 3.0), ("random", P.VOLUME, (1, 512, 256), 0.5),
                 ("layers", P.ARRAY, (6, 33, 33), 0.5), ("layers", P.ARRAY, (6, 64, 64), 0.7), ("random", P.VOLUME, (9, 33, 17), 0.4),
                 ("ties", P.VOLUME, (32, 64, 48), 0.5), ("none", P.VOLUME, (1, 40, 40), 0.5), ("zero", P.ARRAY, (2, 20, 24), 0.5),
                 ("random", P.VOLUME, (1, 64, 64), 1.0)]
        for alpha, mk, shape, cutoff in cases:
            img = _image(kind, shape, shape[1] + shape[0], alpha)
            got = _check_chain(product, ctx, img, mk, P.ALPHA_COVERAGE, cutoff)
            _coverage_holds(got, mk, cutoff)
            if alpha in ("none", "zero"):
                plain = V.chain_array(img) if mk == P.ARRAY else V.chain_volume(img)
                for g, m in zip(got, plain):
                    assert _same(g, m), (alpha, "a surface with k == 0 or all alphas zero must stay unchanged")
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("kind", ["u8", "f16", "f32"])
def test_both_options(product, A, kind):
    ctx = _ctx(product, A.PRF_HDR if kind != "u8" else A.PRF_LDR, (6, 6))
    try:
        for what, mk, shape in SHAPES:
            got = _check_chain(product, ctx, _image(kind, shape, 7 + shape[1], "ties"), mk, BOTH, 0.5)
            _coverage_holds(got, mk, 0.5)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("kind", ["u8", "f16", "f32"])
def test_null_options_and_zero_flags_are_the_plain_calls(product, A, kind):
    ctx = _ctx(product, A.PRF_HDR if kind != "u8" else A.PRF_LDR, (6, 6))
    try:
        img2 = _dev(_image(kind, (1, 130, 66), 3)[0])
        plain = product.generate_mip_chain_device(ctx, img2)
        for opts in (None, (0, 0.0), (0, float("nan"))):
            got = product.generate_mip_chain_ex_device(ctx, img2[None].contiguous(), A.MIP_VOLUME, 0, opts)
            assert len(got) == len(plain)
            for g, m in zip(got, plain):
                assert g[0].cpu().numpy().tobytes() == m.cpu().numpy().tobytes()
        vol = _dev(_image(kind, (6, 40, 24), 4))
        for mk in (A.MIP_VOLUME, A.MIP_ARRAY):
            plain = product.generate_mip_chain_volume_device(ctx, vol, mk)
            for opts in (None, (0, 0.5)):
                got = product.generate_mip_chain_ex_device(ctx, vol, mk, 0, opts)
                for g, m in zip(got, plain):
                    assert g.cpu().numpy().tobytes() == m.cpu().numpy().tobytes()
    finally:
        product.context_free(ctx)


def _single_volume(lib, A, ctx, img, nbytes):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    types = {torch.uint8: A.TYPE_U8, torch.float16: A.TYPE_F16, torch.float32: A.TYPE_F32}
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), img.shape[2], img.shape[1], img.shape[0], types[img.dtype],
                                                     C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                     A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


@pytest.mark.parametrize("mip_kind,block,flags", [("2d", (6, 6), BOTH), ("array", (4, 4), P.ALPHA_COVERAGE),
                                                  ("volume", (4, 4, 4), P.NORMALIZE)])
def test_compressed_levels_equal_the_volume_call(product, A, mip_kind, block, flags):
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_FASTEST)
    try:
        shape = {"2d": (1, 130, 66), "array": (6, 64, 48), "volume": (12, 40, 24)}[mip_kind]
        mk = A.MIP_ARRAY if mip_kind == "array" else A.MIP_VOLUME
        img = _image("u8", shape, 11, "ties")
        levels, blocks = product.compress_mip_chain_ex_device(ctx, _dev(img), mk, 0, (flags, 0.5))
        torch.cuda.synchronize()
        assert product.last_kernel_ms > 0
        model = P.chain(img, mk, flags, 0.5)
        assert len(levels) == len(model)
        for i, (lv, bl, m) in enumerate(zip(levels, blocks, model)):
            assert _same(lv.cpu().numpy(), m), "level %d texels" % i
            want = _single_volume(product, A, ctx, _dev(m), bl.numel())
            bad = int((bl.cpu().numpy().reshape(-1, 16) != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
            assert bad == 0, "level %d: %d blocks differ from the volume call" % (i, bad)
    finally:
        product.context_free(ctx)


def test_small_chain_blocks_equal_the_reference(product, ref, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        img = _image("u8", (1, 48, 40), 12, "ties")
        levels, blocks = product.compress_mip_chain_ex_device(ctx, _dev(img), A.MIP_VOLUME, 0, (BOTH, 0.5))
        torch.cuda.synchronize()
        for i, (m, bl) in enumerate(zip(P.chain(img, P.VOLUME, BOTH, 0.5), blocks)):
            r = ref.compress(m[0], (6, 6), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
            bad = int((bl.cpu().numpy().reshape(-1, 16) != r).any(axis=1).sum())
            assert bad == 0, "level %d %s: %d blocks differ from the reference" % (i, m.shape, bad)
    finally:
        product.context_free(ctx)


def test_option_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_FASTEST)
    srgb = _ctx(product, A.PRF_LDR_SRGB, (6, 6), A.PRE_FASTEST)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        w, h, d = 100, 60, 1
        img = _dev(_image("u8", (d, h, w), 13))
        err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, 0)
        err, lay = product.mip_chain_volume_layout(cfg, w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0)
        store = torch.full((lay.texels_len,), 0xAB, dtype=torch.uint8, device="cuda")
        out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")
        swz = A.Swizzle(*A.SWZ_RGBA)

        def generate(opts, c=ctx):
            return product.lib.astcenc_amd_generate_mip_chain_ex_device(c, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0,
                                                                        C.byref(A.MipOptions(*opts)), store.data_ptr(), lay.texels_len, None)

        def compress(opts, c=ctx):
            return product.lib.astcenc_amd_compress_mip_chain_ex_device(c, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8, C.byref(swz), 0,
                                                                        C.byref(A.MipOptions(*opts)), store.data_ptr(), lay.texels_len,
                                                                        out.data_ptr(), lay.blocks_len, None, None)
        bad = [("unknown flag bits", (0x4, 0.5), ctx), ("unknown flag bits with valid ones", (0x3 | 0x100, 0.5), ctx),
               ("NaN cutoff", (A.MIP_ALPHA_COVERAGE, float("nan")), ctx), ("zero cutoff", (A.MIP_ALPHA_COVERAGE, 0.0), ctx),
               ("negative cutoff", (A.MIP_ALPHA_COVERAGE, -0.5), ctx), ("cutoff above 1", (A.MIP_ALPHA_COVERAGE, 1.0001), ctx),
               ("normalize in sRGB", (A.MIP_NORMALIZE, 0.5), srgb)]
        for what, opts, c in bad:
            for call in (generate, compress):
                logged.clear()
                assert call(opts, c) == A.ERR_BAD_PARAM, what
                torch.cuda.synchronize()
                assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), what + ": a buffer was written"
                assert any("options" in m for m in logged), (what, logged)
        # coverage alone is fine in sRGB (channel 3 is linear there), and the calls work with these buffers
        assert generate((A.MIP_ALPHA_COVERAGE, 0.5), srgb) == A.SUCCESS
        assert compress((BOTH, 1.0)) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)
        product.context_free(srgb)


def test_stream_order_on_a_side_stream(product, A):
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST)
    try:
        side = torch.cuda.Stream()
        src = _image("u8", (1, 512, 512), 14, "ties")
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            img = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            img.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_ex_device(ctx, img, A.MIP_VOLUME, 0, (BOTH, 0.5), stream=side)
            first = [lv.clone() for lv in levels]
        side.synchronize()
        assert product.last_kernel_ms > 0
        for lv, m in zip(first, P.chain(src, P.VOLUME, BOTH, 0.5)):
            assert _same(lv.cpu().numpy(), m)
    finally:
        product.context_free(ctx)
