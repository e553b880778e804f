# SPDX-License-Identifier: Apache-2.0
"""Windowed mip filters on the GPU (astcenc_amd_generate_mip_chain_filtered_device / astcenc_amd_compress_mip_chain_filtered_device).

Every level equals the numpy model (tests/mip_filter_model.py) for every kind and edge, U8, U8 sRGB, F16 and F32, 2D images,
arrays (a cube map among them) and volumes, on small awkward shapes, a 4096^2 image and a 16385-wide wrapped axis; float data
with infinities compares NaN-aware; a null filter and the box give the _ex_ calls' bytes; the options compose as post(levels);
compressed levels equal the volume call on the model's levels (and the reference's on one small chain); bad filters write
nothing and are named in the log; the call keeps stream order on a side stream and reports kernel_ms."""
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


def _ctx(lib, profile, block, quality=None):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality if quality is not None else 0.0, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _image(dtype, shape, seed, inf=False):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    v = (rng.random(shape + (4,)) * 1.4 - 0.2).astype(dtype)
    if inf:
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)
        flat[pos] = np.where(rng.random(pos.size) < 0.5, np.inf, -np.inf).astype(dtype)
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
    got = product.generate_mip_chain_filtered_device(ctx, _dev(img), mip_kind, 0, options, (kind, edge))
    torch.cuda.synchronize()
    want = F.chain(img, mip_kind, kind, edge, srgb=srgb)
    if options is not None:
        want = P.post(want, mip_kind, options[0], options[1])
    assert len(got) == len(want)
    got = [g.cpu().numpy() for g in got]
    for i, (g, m) in enumerate(zip(got, want)):
        bad = _bad_texels(g, m)
        assert bad == 0, (img.dtype, img.shape, mip_kind, kind, edge, srgb, options, "level %d: %d texels differ" % (i, bad))
    return got


SHAPES = [(F.VOLUME, (1, 1, 1)), (F.VOLUME, (1, 37, 1)), (F.VOLUME, (1, 5, 3)), (F.VOLUME, (1, 61, 97)), (F.VOLUME, (1, 256, 255)),
          (F.VOLUME, (1, 3, 1000)), (F.ARRAY, (6, 33, 33)), (F.ARRAY, (2, 20, 17)), (F.VOLUME, (9, 17, 33))]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_levels_match_the_model(product, A, name, dtype, srgb):
    profile = A.PRF_LDR_SRGB if srgb else A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR
    ctx = _ctx(product, profile, (6, 6))
    try:
        for n, (mip_kind, shape) in enumerate(SHAPES):
            img = _image(dtype, shape, 100 + n)
            for kind in F.KINDS:
                for edge in (F.CLAMP, F.WRAP):
                    _check_chain(product, ctx, img, mip_kind, kind, edge, srgb)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_infinities_compare_nan_aware(product, A, dtype):
    ctx = _ctx(product, A.PRF_HDR, (6, 6))
    try:
        for n, (mip_kind, shape) in enumerate([(F.VOLUME, (1, 61, 97)), (F.ARRAY, (3, 40, 24)), (F.VOLUME, (9, 17, 33))]):
            img = _image(dtype, shape, 200 + n, inf=True)
            for kind in F.KINDS:
                _check_chain(product, ctx, img, mip_kind, kind, F.WRAP if n % 2 else F.CLAMP)
    finally:
        product.context_free(ctx)


def test_large_image_and_wide_wrapped_axis(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        _check_chain(product, ctx, _image(np.uint8, (1, 4096, 4096), 7), F.VOLUME, F.LANCZOS3, F.CLAMP)
        _check_chain(product, ctx, _image(np.uint8, (1, 5, 16385), 8), F.VOLUME, F.KAISER, F.WRAP)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f32", np.float32)])
def test_box_is_the_ex_call(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for mip_kind, shape in [(F.VOLUME, (1, 130, 66)), (F.ARRAY, (6, 40, 24)), (F.VOLUME, (6, 40, 24))]:
            img = _dev(_image(dtype, shape, 9))
            for opts in (None, (A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)):
                plain = [t.cpu().numpy().tobytes() for t in product.generate_mip_chain_ex_device(ctx, img, mip_kind, 0, opts)]
                for flt in (None, (A.MIP_FILTER_BOX, A.MIP_EDGE_CLAMP), (A.MIP_FILTER_BOX, A.MIP_EDGE_WRAP)):
                    got = product.generate_mip_chain_filtered_device(ctx, img, mip_kind, 0, opts, flt)
                    assert [t.cpu().numpy().tobytes() for t in got] == plain, (mip_kind, shape, opts, flt)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f16", np.float16)])
def test_options_compose(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for mip_kind, shape in [(F.VOLUME, (1, 61, 97)), (F.ARRAY, (6, 33, 33)), (F.VOLUME, (9, 17, 33))]:
            img = _image(dtype, shape, 10)
            for flags in (P.NORMALIZE, P.ALPHA_COVERAGE, P.NORMALIZE | P.ALPHA_COVERAGE):
                _check_chain(product, ctx, img, mip_kind, F.LANCZOS3, F.CLAMP, options=(flags, 0.5))
                _check_chain(product, ctx, img, mip_kind, F.MITCHELL, F.WRAP, options=(flags, 0.5))
    finally:
        product.context_free(ctx)


def _single_volume(lib, A, ctx, img, nbytes):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), img.shape[2], img.shape[1], img.shape[0], A.TYPE_U8,
                                                     C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                     A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


@pytest.mark.parametrize("mip_kind,block,shape", [(F.VOLUME, (6, 6), (1, 130, 66)), (F.VOLUME, (4, 4, 4), (12, 40, 24))])
def test_compressed_levels_equal_the_volume_call(product, A, mip_kind, block, shape):
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_FASTEST)
    try:
        img = _image(np.uint8, shape, 11)
        levels, blocks = product.compress_mip_chain_filtered_device(ctx, _dev(img), mip_kind, 0, None, (A.MIP_FILTER_KAISER, A.MIP_EDGE_CLAMP))
        torch.cuda.synchronize()
        assert product.last_kernel_ms > 0
        model = F.chain(img, mip_kind, F.KAISER, F.CLAMP)
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
        _, blocks = product.compress_mip_chain_filtered_device(ctx, _dev(img), A.MIP_VOLUME, 0, None, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_WRAP))
        torch.cuda.synchronize()
        for i, (m, bl) in enumerate(zip(F.chain(img, F.VOLUME, F.LANCZOS3, F.WRAP), blocks)):
            r = ref.compress(m[0], (6, 6), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
            bad = int((bl.cpu().numpy().reshape(-1, 16) != r).any(axis=1).sum())
            assert bad == 0, "level %d %s: %d blocks differ from the reference" % (i, m.shape, bad)
    finally:
        product.context_free(ctx)


def test_filter_errors_write_nothing(product, A):
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

        def generate(flt, opts):
            o = C.byref(A.MipOptions(*opts)) if opts else None
            return product.lib.astcenc_amd_generate_mip_chain_filtered_device(ctx, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0, o,
                                                                              C.byref(A.MipFilter(*flt)), store.data_ptr(), lay.texels_len,
                                                                              None)

        def compress(flt, opts):
            o = C.byref(A.MipOptions(*opts)) if opts else None
            return product.lib.astcenc_amd_compress_mip_chain_filtered_device(ctx, img.data_ptr(), w, h, d, A.MIP_VOLUME, A.TYPE_U8,
                                                                              C.byref(swz), 0, o, C.byref(A.MipFilter(*flt)),
                                                                              store.data_ptr(), lay.texels_len, out.data_ptr(),
                                                                              lay.blocks_len, None, None)
        for flt in ((4, 0), (-1, 0), (2, 2), (1, -1), (0, 7)):
            for opts in (None, (A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)):
                for call in (generate, compress):
                    logged.clear()
                    assert call(flt, opts) == A.ERR_BAD_PARAM, (flt, opts)
                    torch.cuda.synchronize()
                    assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), (flt, opts, "a buffer was written")
                    assert any("filter" in m for m in logged), (flt, opts, logged)
        assert generate((A.MIP_FILTER_MITCHELL, A.MIP_EDGE_WRAP), None) == A.SUCCESS
        assert compress((A.MIP_FILTER_KAISER, A.MIP_EDGE_CLAMP), (A.MIP_ALPHA_COVERAGE, 0.5)) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)


def test_stream_order_on_a_side_stream(product, A):
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST)
    try:
        side = torch.cuda.Stream()
        src = _image(np.uint8, (1, 512, 512), 14)
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            img = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            img.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_filtered_device(ctx, img, A.MIP_VOLUME, 0, None, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP),
                                                                        stream=side)
            first = [lv.clone() for lv in levels]
        side.synchronize()
        assert product.last_kernel_ms > 0
        for lv, m in zip(first, F.chain(src, F.VOLUME, F.LANCZOS3, F.CLAMP)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0
    finally:
        product.context_free(ctx)
