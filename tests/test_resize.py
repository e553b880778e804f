# SPDX-License-Identifier: Apache-2.0
"""Resizing on the GPU (astcenc_amd_resize_image_device).

Every result equals the numpy model (tests/resize_model.py) bit for bit, NaN-aware for floats: every filter kind, both edges,
both weightings, U8, U8 sRGB, F16 and F32, arrays and volumes, on non-integer ratios, large ratios in both directions (the
chunked walk over a tile's source rows), an untouched axis, a source of one texel, a volume resized on all three axes, one
4096^2 -> 3000 x 1500 image and float data with infinities.  Resizing to max(1, s >> 1) on every axis equals level 1 of the
matching _weighted_ chain call byte for byte (there the existing kernels are the oracle); the same size returns the input's
bytes; channel 3 of a weighted resize is the plain one's; a resized image composes with the chain calls as their level 0; the
blocks of one small case equal the reference's; every error returns its code, writes nothing and is named in the log; the call
keeps stream order on a side stream and reports kernel_ms."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_weighted_model as W  # noqa: E402
import resize_model as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "resize_48x40_to_36x30_6x6_medium.npy")


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
        v = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
        v[..., 3][rng.random(shape) < 0.3] = 0
        return v
    v = (rng.random(shape + (4,)) * 1.4 - 0.2).astype(dtype)
    v[..., 3][rng.random(shape) < 0.3] = 0
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


def _check(product, ctx, img, size, mip_kind, kind, edge, weight=R.NONE, srgb=False):
    got = product.resize_image_device(ctx, _dev(img), size, mip_kind, (kind, edge), weight)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = R.resize(img, size, mip_kind, kind, edge, weight, srgb)
    bad = _bad_texels(got, want)
    assert bad == 0, (img.dtype, img.shape, size, mip_kind, kind, edge, weight, srgb, "%d texels differ" % bad)
    return got


# (mip kind, source [Z, H, W], destination (w, h[, d]))
SHAPES = [(R.VOLUME, (1, 61, 97), (40, 77)),           # non-integer ratios, down in x and up in y
          (R.VOLUME, (1, 3, 1000), (7, 200)),          # large ratios in both directions
          (R.VOLUME, (1, 1000, 5), (8, 7)),            # ... and down in y: a tile walks its 1000 source rows in chunks
          (R.VOLUME, (1, 130, 70), (300, 33)),         # two chunks to a tile
          (R.ARRAY, (3, 20, 17), (17, 31)),            # an untouched axis
          (R.VOLUME, (1, 1, 37), (50, 5)),             # s == 1
          (R.VOLUME, (9, 17, 33), (20, 9, 14)),        # a volume resized on all three axes
          (R.VOLUME, (5, 8, 8), (8, 8, 2)),            # ... and on z alone
          (R.ARRAY, (6, 33, 33), (64, 16))]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]


def _profile(A, dtype, srgb):
    return A.PRF_LDR_SRGB if srgb else A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
@pytest.mark.parametrize("weight", [R.NONE, R.ALPHA], ids=["plain", "alpha"])
def test_resized_images_match_the_model(product, A, weight, name, dtype, srgb):
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for n, (mip_kind, shape, size) in enumerate(SHAPES):
            img = _image(dtype, shape, 100 + n)
            for kind in R.FILTERS:
                for edge in (R.CLAMP, R.WRAP):
                    _check(product, ctx, img, size, mip_kind, kind, edge, weight, srgb)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("dtype", [np.float16, np.float32])
def test_infinities_compare_nan_aware(product, A, dtype):
    ctx = _ctx(product, A.PRF_HDR, (6, 6))
    try:
        for n, (mip_kind, shape, size) in enumerate([SHAPES[0], SHAPES[4], SHAPES[6]]):
            img = _image(dtype, shape, 200 + n, inf=True)
            for kind in R.FILTERS:
                for weight in (R.NONE, R.ALPHA):
                    _check(product, ctx, img, size, mip_kind, kind, R.WRAP if n % 2 else R.CLAMP, weight)
    finally:
        product.context_free(ctx)


def test_large_image(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        _check(product, ctx, _image(np.uint8, (1, 4096, 4096), 7), (3000, 1500), R.VOLUME, R.LANCZOS3, R.CLAMP)
    finally:
        product.context_free(ctx)


HALVING = [(R.VOLUME, (1, 61, 97)), (R.VOLUME, (1, 64, 128)), (R.ARRAY, (6, 33, 33)), (R.ARRAY, (2, 20, 16)), (R.VOLUME, (9, 17, 33)),
           (R.VOLUME, (8, 16, 32)), (R.VOLUME, (1, 1, 37)), (R.VOLUME, (1, 300, 260))]


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_halving_equals_the_chain(product, A, name, dtype, srgb):
    """Level 1 of astcenc_amd_generate_mip_chain_weighted_device, made by the chain's own kernels, is the oracle."""
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for n, (mip_kind, shape) in enumerate(HALVING):
            img = _dev(_image(dtype, shape, 300 + n))
            z, h, w = shape
            half = (max(1, w >> 1), max(1, h >> 1), max(1, z >> 1) if mip_kind == R.VOLUME else z)
            for kind in R.FILTERS:
                for weight in (R.NONE, R.ALPHA):
                    edge = R.WRAP if (n + kind) % 2 else R.CLAMP
                    chain = product.generate_mip_chain_weighted_device(ctx, img, mip_kind, 2, None, (kind, edge), weighting=weight)
                    got = product.resize_image_device(ctx, img, half, mip_kind, (kind, edge), weight)
                    torch.cuda.synchronize()
                    assert tuple(got.shape) == tuple(chain[1].shape)
                    assert got.cpu().numpy().tobytes() == chain[1].cpu().numpy().tobytes(), (dtype, srgb, mip_kind, shape, kind, edge, weight)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_same_size_returns_the_input(product, A, name, dtype, srgb):
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for mip_kind, shape in [(R.VOLUME, (1, 61, 97)), (R.ARRAY, (3, 20, 17)), (R.VOLUME, (5, 9, 7))]:
            img = _image(dtype, shape, 400, inf=dtype != np.uint8)
            z, h, w = shape
            for kind in R.FILTERS:
                got = product.resize_image_device(ctx, _dev(img), (w, h, z), mip_kind, (kind, R.CLAMP))
                torch.cuda.synchronize()
                assert got.cpu().numpy().tobytes() == img.tobytes(), (dtype, srgb, mip_kind, shape, kind)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_alpha_weighting_keeps_channel_3(product, A, name, dtype, srgb):
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for mip_kind, shape, size in [SHAPES[0], SHAPES[4], SHAPES[6]]:
            img = _dev(_image(dtype, shape, 500))
            for kind in R.FILTERS:
                plain = product.resize_image_device(ctx, img, size, mip_kind, (kind, R.CLAMP), R.NONE).cpu().numpy()
                alpha = product.resize_image_device(ctx, img, size, mip_kind, (kind, R.CLAMP), R.ALPHA).cpu().numpy()
                assert plain[..., 3].tobytes() == alpha[..., 3].tobytes(), (dtype, srgb, mip_kind, shape, kind)
                assert plain.tobytes() != alpha.tobytes()
    finally:
        product.context_free(ctx)


def _single_volume(lib, A, ctx, img, nbytes):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), img.shape[2], img.shape[1], img.shape[0], A.TYPE_U8,
                                                     C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                     A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


@pytest.mark.parametrize("mip_kind,block,shape,size", [(R.VOLUME, (6, 6), (1, 200, 150), (130, 66)), (R.VOLUME, (4, 4, 4), (9, 50, 30), (24, 40, 12))])
def test_resized_image_is_level_0_of_a_chain(product, A, mip_kind, block, shape, size):
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_FASTEST)
    try:
        img = _image(np.uint8, shape, 11)
        resized = product.resize_image_device(ctx, _dev(img), size, mip_kind, (A.MIP_FILTER_KAISER, A.MIP_EDGE_CLAMP), A.MIP_WEIGHT_ALPHA)
        levels, blocks = product.compress_mip_chain_weighted_device(ctx, resized, mip_kind, 0, None, (A.MIP_FILTER_KAISER, A.MIP_EDGE_CLAMP),
                                                                    weighting=A.MIP_WEIGHT_ALPHA)
        torch.cuda.synchronize()
        model = W.chain(R.resize(img, size, mip_kind, R.KAISER, R.CLAMP, R.ALPHA), mip_kind, W.KAISER, W.CLAMP, W.ALPHA)
        assert len(levels) == len(model)
        for i, (lv, bl, m) in enumerate(zip(levels, blocks, model)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0, "level %d texels" % i
            want = _single_volume(product, A, ctx, _dev(m), bl.numel())
            bad = int((bl.cpu().numpy().reshape(-1, 16) != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
            assert bad == 0, "level %d: %d blocks differ from the volume call" % (i, bad)
    finally:
        product.context_free(ctx)


def test_blocks_equal_the_reference(product, A):
    """The reference's blocks of the model's resized image: recorded in tests/golden, and compared live where the reference is built."""
    import oracle_libs as O
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        img = _image(np.uint8, (1, 48, 40), 12)
        resized = product.resize_image_device(ctx, _dev(img), (36, 30), A.MIP_VOLUME, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_WRAP))
        blocks = _single_volume(product, A, ctx, resized, 6 * 5 * 16).cpu().numpy().reshape(-1, 16)
        model = R.resize(img, (36, 30), R.VOLUME, R.LANCZOS3, R.WRAP)
        assert _bad_texels(resized.cpu().numpy(), model) == 0
        want = np.load(GOLDEN).reshape(-1, 16)
        assert int((blocks != want).any(axis=1).sum()) == 0
        if os.path.exists(O.LIB_REF_NONE):
            live = A.Library(O.LIB_REF_NONE).compress(model[0], (6, 6), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
            assert int((blocks != live).any(axis=1).sum()) == 0
    finally:
        product.context_free(ctx)


def test_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_FASTEST)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        w, h, d = 100, 60, 2
        img = _dev(_image(np.uint8, (d, h, w), 13))
        out = torch.full((5000001 * 4,), 0xAB, dtype=torch.uint8, device="cuda")
        lanczos, box = (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP), (A.MIP_FILTER_BOX, A.MIP_EDGE_CLAMP)

        def call(size, flt=lanczos, weight=A.MIP_WEIGHT_NONE, kind=A.MIP_ARRAY, dims=(w, h, d), dtype=A.TYPE_U8, out_len=None, null=False,
                 out_ptr=None):
            rz = A.Resize(size[0], size[1], size[2], A.MipFilter(*flt), A.MipWeighting(weight))
            return product.lib.astcenc_amd_resize_image_device(ctx, img.data_ptr(), dims[0], dims[1], dims[2], kind, dtype,
                                                               None if null else C.byref(rz), out.data_ptr() if out_ptr is None else out_ptr,
                                                               out.numel() if out_len is None else out_len, None, None)
        big = 4294967295
        # (what, the call, its code, named "resize" in the log).  The two overflow cases name sizes that no buffer has: they
        # pass an out_len of 0, so that even a missing check could launch nothing.
        cases = [("null resize", lambda: call((50, 30, d), null=True), A.ERR_BAD_PARAM, True),
                 ("zero destination x", lambda: call((0, 30, d)), A.ERR_BAD_PARAM, True),
                 ("zero destination y", lambda: call((50, 0, d)), A.ERR_BAD_PARAM, True),
                 ("zero destination z", lambda: call((50, 30, 0)), A.ERR_BAD_PARAM, True),
                 ("zero source dimension", lambda: call((50, 30, d), dims=(0, h, d)), A.ERR_BAD_PARAM, False),
                 ("unknown mip kind", lambda: call((50, 30, d), kind=2), A.ERR_BAD_PARAM, False),
                 ("unknown data type", lambda: call((50, 30, d), dtype=3), A.ERR_BAD_PARAM, False),
                 ("unknown filter kind", lambda: call((50, 30, d), flt=(4, 0)), A.ERR_BAD_PARAM, True),
                 ("negative filter kind", lambda: call((50, 30, d), flt=(-1, 0)), A.ERR_BAD_PARAM, True),
                 ("unknown edge", lambda: call((50, 30, d), flt=(2, 3)), A.ERR_BAD_PARAM, True),
                 ("cube edge", lambda: call((50, 30, d), flt=(2, A.MIP_EDGE_CUBE)), A.ERR_BAD_PARAM, True),
                 ("unknown weight", lambda: call((50, 30, d), weight=2), A.ERR_BAD_PARAM, True),
                 ("an array's layers change", lambda: call((50, 30, d + 1)), A.ERR_BAD_PARAM, True),
                 ("bytes beyond size_t", lambda: call((big, big, big), kind=A.MIP_VOLUME, out_len=0), A.ERR_BAD_PARAM, True),
                 ("integer box beyond 64 bits", lambda: call((1, 1, 1), flt=box, kind=A.MIP_VOLUME, dims=(60000, 60000, 60000), out_len=0),
                  A.ERR_BAD_PARAM, True),
                 ("null output", lambda: call((50, 30, d), out_ptr=0), A.ERR_BAD_CONTEXT, False),
                 ("out_len too short", lambda: call((50, 30, d), out_len=50 * 30 * d * 4 - 1), A.ERR_OUT_OF_MEM, True),
                 ("taps beyond the scratch bound", lambda: call((5000001, 1, 1), kind=A.MIP_VOLUME, dims=(3, 1, 1)), A.ERR_OUT_OF_MEM, True)]
        for what, fn, code, named in cases:
            logged.clear()
            assert fn() == code, what
            torch.cuda.synchronize()
            assert bool((out == 0xAB).all()), (what, "the output was written")
            assert logged, what
            assert not named or any("resize" in m for m in logged), (what, logged)
        # the integer box bound is exact: one factor less passes the check (and is then refused for its out_len)
        z = -(-(1 << 63) // (60000 * 60000 * 65025))            # the least depth with 60000 * 60000 * z * 65025 >= 2^63
        assert call((1, 1, 1), flt=box, kind=A.MIP_VOLUME, dims=(60000, 60000, z), out_len=0) == A.ERR_BAD_PARAM
        assert call((1, 1, 1), flt=box, kind=A.MIP_VOLUME, dims=(60000, 60000, z - 1), out_len=0) == A.ERR_OUT_OF_MEM
        assert call((50, 30, d)) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:50 * 30 * d * 4] == 0xAB).all()) and bool((out[50 * 30 * d * 4:] == 0xAB).all())
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
            got = product.resize_image_device(ctx, img, (300, 217), A.MIP_VOLUME, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP), stream=side)
            first = got.clone()
        side.synchronize()
        assert product.last_kernel_ms > 0
        assert _bad_texels(first.cpu().numpy(), R.resize(src, (300, 217), R.VOLUME, R.LANCZOS3, R.CLAMP)) == 0
    finally:
        product.context_free(ctx)


def test_kernel_ms(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        product.last_kernel_ms = 0.0
        product.resize_image_device(ctx, _dev(_image(np.uint8, (1, 256, 256), 15)), (100, 100), A.MIP_VOLUME)
        assert product.last_kernel_ms > 0
    finally:
        product.context_free(ctx)
