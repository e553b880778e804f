# SPDX-License-Identifier: Apache-2.0
"""Alpha-weighted mip filtering on the GPU (astcenc_amd_generate_mip_chain_weighted_device / astcenc_amd_compress_mip_chain_weighted_device).

Every level equals the numpy model (tests/mip_weighted_model.py), 0 differing texels: the box and every windowed kind and edge,
U8, U8 sRGB, F16 and F32, on the shapes of tests/test_mip_filter.py and tests/test_mip_options.py (2D images, arrays with a cube
map among them, volumes, odd and 1-wide axes), a 4096^2 RGBA8 image (the even path and the tail) and an even 64 x 64 x 32
volume; float data with infinite and negative alphas compares NaN-aware.  A null weighting and WEIGHT_NONE give the _filtered_
calls' bytes; the options compose as post(levels); an opaque red disc on transparent green keeps R = 255, G = 0 wherever
alpha > 0; compressed levels equal the volume call on the model's levels (and the reference's on one small chain); a bad weight
writes nothing and is named in the log; the call keeps stream order on a side stream and reports kernel_ms."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_filter_model as F  # noqa: E402
import mip_options_model as P  # noqa: E402
import mip_weighted_model as W  # noqa: E402


def _ctx(lib, profile, block, quality=None):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality if quality is not None else 0.0, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(dtype, shape, seed, special=False):
    """Random texels; alpha is 0 in the low quarter of the image (whole footprints at every level), 0 in a random third of the
    rest, random elsewhere; special (floats): a few negative and infinite alphas and infinite colours too."""
    rng = np.random.default_rng(seed)
    z, h, w = shape
    if dtype == np.uint8:
        v = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    else:
        v = (rng.random(shape + (4,)) * 1.4 - 0.2).astype(dtype)
        v[..., 3] = np.abs(v[..., 3])
    a = v[..., 3]
    a[rng.random(shape) < 0.33] = 0
    a[:, :max(1, h // 2), :max(1, w // 2)] = 0
    if special:
        r = rng.random(shape)
        a[r < 0.05] *= -1
        a[(r >= 0.05) & (r < 0.07)] = np.inf
        a[(r >= 0.07) & (r < 0.08)] = -np.inf
        flat = v[..., :3].reshape(-1)
        pos = rng.choice(flat.size, size=max(1, flat.size // 60), replace=False)
        flat[pos] = np.where(rng.random(pos.size) < 0.5, np.inf, -np.inf).astype(dtype)
        v[..., :3] = flat.reshape(shape + (3,))
    return v


def _bad_texels(g, m):
    """Texels that differ: bytes for finite data, NaN-aware for floats (NaN payloads may differ between the GPU and x86)."""
    if g.shape != m.shape:
        return -1
    if g.dtype == np.uint8:
        return int((g.reshape(-1, 4) != m.reshape(-1, 4)).any(axis=1).sum())
    bits = np.uint16 if g.dtype == np.float16 else np.uint32
    same = (g.view(bits) == m.view(bits)) | (np.isnan(g) & np.isnan(m))
    return int((~same.reshape(-1, 4)).any(axis=1).sum())


def _check_chain(product, ctx, img, mip_kind, kind, edge, srgb=False, options=None):
    got = product.generate_mip_chain_weighted_device(ctx, _dev(img), mip_kind, 0, options, (kind, edge), weighting=W.ALPHA)
    torch.cuda.synchronize()
    want = W.chain(img, mip_kind, kind, edge, W.ALPHA, srgb=srgb)
    if options is not None:
        want = P.post(want, mip_kind, options[0], options[1])
    assert len(got) == len(want)
    got = [g.cpu().numpy() for g in got]
    for i, (g, m) in enumerate(zip(got, want)):
        bad = _bad_texels(g, m)
        print("%s %s kind %d filter %d edge %d srgb %d level %d: %d texels differ" % (img.dtype, img.shape, mip_kind, kind, edge, srgb, i, bad))
        assert bad == 0, (img.dtype, img.shape, mip_kind, kind, edge, srgb, options, "level %d: %d texels differ" % (i, bad))
    return got


# tests/test_mip_filter.py's shapes, then tests/test_mip_options.py's
SHAPES = [(F.VOLUME, (1, 1, 1)), (F.VOLUME, (1, 37, 1)), (F.VOLUME, (1, 5, 3)), (F.VOLUME, (1, 61, 97)), (F.VOLUME, (1, 256, 255)),
          (F.VOLUME, (1, 3, 1000)), (F.ARRAY, (6, 33, 33)), (F.ARRAY, (2, 20, 17)), (F.VOLUME, (9, 17, 33)),
          (F.VOLUME, (1, 37, 23)), (F.VOLUME, (1, 512, 256)), (F.ARRAY, (6, 33, 17)), (F.ARRAY, (3, 130, 66)), (F.VOLUME, (9, 33, 17)),
          (F.VOLUME, (32, 64, 48))]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]
FILTERS = [(F.BOX, F.CLAMP)] + [(k, e) for k in F.KINDS for e in (F.CLAMP, F.WRAP)]


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_levels_match_the_model(product, A, name, dtype, srgb):
    profile = A.PRF_LDR_SRGB if srgb else A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR
    ctx = _ctx(product, profile, (6, 6))
    try:
        for n, (mip_kind, shape) in enumerate(SHAPES):
            img = _image(dtype, shape, 100 + n)
            for kind, edge in FILTERS:
                _check_chain(product, ctx, img, mip_kind, kind, edge, srgb)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_infinite_and_negative_alpha_compare_nan_aware(product, A, dtype):
    ctx = _ctx(product, A.PRF_HDR, (6, 6))
    try:
        for n, (mip_kind, shape) in enumerate([(F.VOLUME, (1, 61, 97)), (F.ARRAY, (3, 40, 24)), (F.VOLUME, (9, 17, 33)), (F.VOLUME, (8, 64, 96))]):
            img = _image(dtype, shape, 200 + n, special=True)
            for kind, edge in FILTERS:
                _check_chain(product, ctx, img, mip_kind, kind, edge)
    finally:
        product.context_free(ctx)


def test_large_image_and_even_volume(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        big = _image(np.uint8, (1, 4096, 4096), 7)
        _check_chain(product, ctx, big, F.VOLUME, F.BOX, F.CLAMP)
        _check_chain(product, ctx, big, F.VOLUME, F.LANCZOS3, F.CLAMP)
        vol = _image(np.uint8, (32, 64, 64), 8)
        for kind, edge in FILTERS:
            _check_chain(product, ctx, vol, F.VOLUME, kind, edge)
    finally:
        product.context_free(ctx)
    for dtype in (np.float16, np.float32):
        ctx = _ctx(product, A.PRF_HDR, (6, 6))
        try:
            _check_chain(product, ctx, _image(dtype, (32, 64, 64), 9), F.VOLUME, F.BOX, F.CLAMP)
            _check_chain(product, ctx, _image(dtype, (6, 256, 128), 10), F.ARRAY, F.BOX, F.CLAMP)
        finally:
            product.context_free(ctx)
    ctx = _ctx(product, A.PRF_LDR_SRGB, (6, 6))
    try:
        _check_chain(product, ctx, _image(np.uint8, (32, 64, 64), 11), F.VOLUME, F.BOX, F.CLAMP, srgb=True)
        _check_chain(product, ctx, _image(np.uint8, (1, 512, 512), 12), F.VOLUME, F.BOX, F.CLAMP, srgb=True)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f32", np.float32)])
def test_no_weighting_is_the_filtered_call(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for mip_kind, shape in [(F.VOLUME, (1, 130, 66)), (F.ARRAY, (6, 40, 24)), (F.VOLUME, (6, 40, 24))]:
            img = _dev(_image(dtype, shape, 9))
            for opts in (None, (A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)):
                for flt in (None, (A.MIP_FILTER_BOX, A.MIP_EDGE_CLAMP), (A.MIP_FILTER_KAISER, A.MIP_EDGE_WRAP)):
                    plain = [t.cpu().numpy().tobytes() for t in product.generate_mip_chain_filtered_device(ctx, img, mip_kind, 0, opts, flt)]
                    for wt in (None, A.MIP_WEIGHT_NONE):
                        got = product.generate_mip_chain_weighted_device(ctx, img, mip_kind, 0, opts, flt, weighting=wt)
                        assert [t.cpu().numpy().tobytes() for t in got] == plain, (mip_kind, shape, opts, flt, wt)
                    got = product.generate_mip_chain_weighted_device(ctx, img, mip_kind, 0, opts, flt, weighting=A.MIP_WEIGHT_ALPHA)
                    assert [t.cpu().numpy().tobytes() for t in got] != plain, (mip_kind, shape, opts, flt, "the weighting changed nothing")
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f16", np.float16)])
def test_options_compose(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for mip_kind, shape in [(F.VOLUME, (1, 61, 97)), (F.ARRAY, (6, 33, 33)), (F.VOLUME, (9, 17, 33))]:
            img = _image(dtype, shape, 10)
            both = (P.NORMALIZE | P.ALPHA_COVERAGE, 0.5)
            _check_chain(product, ctx, img, mip_kind, F.BOX, F.CLAMP, options=both)
            _check_chain(product, ctx, img, mip_kind, F.LANCZOS3, F.CLAMP, options=both)
            _check_chain(product, ctx, img, mip_kind, F.MITCHELL, F.WRAP, options=both)
    finally:
        product.context_free(ctx)


def _disc():
    y, x = np.mgrid[0:128, 0:128]
    inside = (x - 63.5) ** 2 + (y - 63.5) ** 2 < 50.0 ** 2
    img = np.zeros((1, 128, 128, 4), np.uint8)
    img[0, inside] = (255, 0, 0, 255)
    img[0, ~inside] = (0, 255, 0, 0)
    return img


def test_disc_has_no_fringe(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        img = _dev(_disc())
        for kind, edge in FILTERS:
            plain = product.generate_mip_chain_filtered_device(ctx, img, A.MIP_VOLUME, 0, None, (kind, edge))
            got = product.generate_mip_chain_weighted_device(ctx, img, A.MIP_VOLUME, 0, None, (kind, edge), weighting=A.MIP_WEIGHT_ALPHA)
            torch.cuda.synchronize()
            fringe = sum(int(((p[..., 3] > 0) & (p[..., 1] > 0)).sum()) for p in plain[1:])
            assert fringe > 200, (kind, edge, fringe)
            for g in got[1:]:
                g = g.cpu().numpy()
                seen = g[..., 3] > 0
                assert (g[seen][:, 0] == 255).all() and (g[seen][:, 1] == 0).all(), (kind, edge, g.shape)
    finally:
        product.context_free(ctx)


def _single_volume(lib, A, ctx, img, nbytes):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), img.shape[2], img.shape[1], img.shape[0], A.TYPE_U8,
                                                     C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                     A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


@pytest.mark.parametrize("mip_kind,block,shape,flt", [(F.VOLUME, (6, 6), (1, 130, 66), (F.BOX, F.CLAMP)),
                                                      (F.VOLUME, (6, 6), (1, 130, 66), (F.KAISER, F.CLAMP)),
                                                      (F.VOLUME, (4, 4, 4), (12, 40, 24), (F.BOX, F.CLAMP)),
                                                      (F.VOLUME, (4, 4, 4), (12, 40, 24), (F.MITCHELL, F.WRAP))])
def test_compressed_levels_equal_the_volume_call(product, A, mip_kind, block, shape, flt):
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_FASTEST)
    try:
        img = _image(np.uint8, shape, 11)
        levels, blocks = product.compress_mip_chain_weighted_device(ctx, _dev(img), mip_kind, 0, None, flt, weighting=A.MIP_WEIGHT_ALPHA)
        torch.cuda.synchronize()
        assert product.last_kernel_ms > 0
        model = W.chain(img, mip_kind, flt[0], flt[1], W.ALPHA)
        assert len(levels) == len(model)
        for i, (lv, bl, m) in enumerate(zip(levels, blocks, model)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0, "level %d texels" % i
            want = _single_volume(product, A, ctx, _dev(m), bl.numel())
            bad = int((bl.cpu().numpy().reshape(-1, 16) != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
            assert bad == 0, "level %d: %d blocks differ from the volume call" % (i, bad)
    finally:
        product.context_free(ctx)


def test_small_chain_blocks_equal_the_reference(product, ref, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        img = _image(np.uint8, (1, 48, 40), 12)
        for flt in ((A.MIP_FILTER_BOX, A.MIP_EDGE_CLAMP), (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_WRAP)):
            _, blocks = product.compress_mip_chain_weighted_device(ctx, _dev(img), A.MIP_VOLUME, 0, None, flt, weighting=A.MIP_WEIGHT_ALPHA)
            torch.cuda.synchronize()
            for i, (m, bl) in enumerate(zip(W.chain(img, F.VOLUME, flt[0], flt[1], W.ALPHA), blocks)):
                r = ref.compress(m[0], (6, 6), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
                bad = int((bl.cpu().numpy().reshape(-1, 16) != r).any(axis=1).sum())
                assert bad == 0, "filter %s level %d %s: %d blocks differ from the reference" % (flt, i, m.shape, bad)
    finally:
        product.context_free(ctx)


def test_weighting_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_FASTEST)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        w, h, d = 100, 60, 1
        img = _dev(_image(np.uint8, (d, h, w), 13))
        err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, 0)
        err, lay = product.mip_chain_volume_layout(cfg, w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0)
        store = torch.full((lay.texels_len,), 0xAB, dtype=torch.uint8, device="cuda")
        out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")
        swz = A.Swizzle(*A.SWZ_RGBA)

        def generate(weight, flt, opts):
            o = C.byref(A.MipOptions(*opts)) if opts else None
            f = C.byref(A.MipFilter(*flt)) if flt else None
            return product.lib.astcenc_amd_generate_mip_chain_weighted_device(ctx, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0, o, f,
                                                                              C.byref(A.MipWeighting(weight)), store.data_ptr(),
                                                                              lay.texels_len, None)

        def compress(weight, flt, opts):
            o = C.byref(A.MipOptions(*opts)) if opts else None
            f = C.byref(A.MipFilter(*flt)) if flt else None
            return product.lib.astcenc_amd_compress_mip_chain_weighted_device(ctx, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8,
                                                                              C.byref(swz), 0, o, f, C.byref(A.MipWeighting(weight)),
                                                                              store.data_ptr(), lay.texels_len, out.data_ptr(),
                                                                              lay.blocks_len, None, None)
        for weight in (2, -1):
            for flt in (None, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP)):
                for opts in (None, (A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)):
                    for call in (generate, compress):
                        logged.clear()
                        assert call(weight, flt, opts) == A.ERR_BAD_PARAM, (weight, flt, opts)
                        torch.cuda.synchronize()
                        assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), (weight, flt, opts, "a buffer was written")
                        assert any("weighting" in m for m in logged), (weight, flt, opts, logged)
        assert generate(A.MIP_WEIGHT_ALPHA, (A.MIP_FILTER_MITCHELL, A.MIP_EDGE_WRAP), None) == A.SUCCESS
        assert compress(A.MIP_WEIGHT_ALPHA, None, (A.MIP_ALPHA_COVERAGE, 0.5)) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)


@pytest.mark.parametrize("flt", [(F.BOX, F.CLAMP), (F.LANCZOS3, F.CLAMP)], ids=["box", "lanczos3"])
def test_stream_order_on_a_side_stream(product, A, flt):
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST)
    try:
        side = torch.cuda.Stream()
        src = _image(np.uint8, (1, 512, 512), 14)
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            img = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            img.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_weighted_device(ctx, img, A.MIP_VOLUME, 0, None, flt, stream=side,
                                                                        weighting=A.MIP_WEIGHT_ALPHA)
            first = [lv.clone() for lv in levels]
        side.synchronize()
        assert product.last_kernel_ms > 0
        for lv, m in zip(first, W.chain(src, F.VOLUME, flt[0], flt[1], W.ALPHA)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0
    finally:
        product.context_free(ctx)
