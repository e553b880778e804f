# SPDX-License-Identifier: Apache-2.0
"""Mip chains on the GPU (astcenc_amd_generate_mip_chain_device / astcenc_amd_compress_mip_chain_device).

Generated levels equal the numpy model of the filter (tests/mip_model.py) bit for bit; every level's blocks equal the single
call's on that level's texels (and the reference's on the model's levels); the chain round-trips through the set decoder; bad
arguments write nothing; the call keeps stream order, progress and cancel; the KTX writer stores every level."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402

SIZES = [(1, 1), (5, 3), (17, 4096), (255, 190), (1000, 1000), (4096, 4096)]      # (w, h)


def _ctx(lib, profile, block, quality, tweak=None, flags=0):
    err, cfg = lib.config_init(profile, block[0], block[1], 1, quality, flags)
    assert err == 0
    if tweak:
        tweak(cfg)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def _image(A, w, h, kind, seed=0):
    rng = np.random.default_rng(seed + w * 7 + h)
    if kind == "u8":
        im = A.synthetic_image(w, h, 0x9E3779B1 + seed).copy()
        im[rng.random((h, w)) < 0.1] = rng.integers(0, 256, 4, dtype=np.uint8)      # some hard edges
        return im
    if kind == "f16":
        return A.synthetic_hdr_image(w, h, seed).astype(np.float16)
    return (rng.standard_normal((h, w, 4)) * 50).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("profile,kind", [("ldr", "u8"), ("srgb", "u8"), ("hdr", "f16"), ("ldr", "f32")])
def test_levels_match_numpy_model(product, A, profile, kind):
    prf = {"ldr": A.PRF_LDR, "srgb": A.PRF_LDR_SRGB, "hdr": A.PRF_HDR}[profile]
    ctx = _ctx(product, prf, (6, 6), A.PRE_FASTEST)
    try:
        for w, h in SIZES:
            img = _image(A, w, h, kind)
            full = M.full_levels(w, h)
            for levels in (0, min(3, full)):
                got = product.generate_mip_chain_device(ctx, _dev(img), levels)
                torch.cuda.synchronize()
                want = M.chain(img, levels, srgb=profile == "srgb")
                assert len(got) == len(want)
                for i, (g, m) in enumerate(zip(got, want)):
                    g = g.cpu().numpy()
                    bad = int((g.view(np.uint8).reshape(g.shape[0], g.shape[1], -1) != m.view(np.uint8).reshape(g.shape[0], g.shape[1], -1)).any(axis=2).sum())
                    assert bad == 0, (profile, kind, (w, h), levels, "level %d: %d texels differ" % (i, bad))
    finally:
        product.context_free(ctx)


def _single(lib, A, ctx, img, nbytes, swz):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    types = {torch.uint8: A.TYPE_U8, torch.float16: A.TYPE_F16, torch.float32: A.TYPE_F32}
    err = lib.lib.astcenc_amd_compress_image_device(ctx, img.data_ptr(), img.shape[1], img.shape[0], types[img.dtype], C.byref(A.Swizzle(*swz)),
                                                    out.data_ptr(), out.numel(), A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


def _chain_vs_single(product, A, ctx, img, swz, ref=None, profile=None, quality=None, block=None, tweak=None, srgb=False):
    levels, blocks = product.compress_mip_chain_device(ctx, _dev(img), 0, swz)
    torch.cuda.synchronize()
    assert product.last_kernel_ms > 0
    model = M.chain(img, srgb=srgb)
    for i, (lv, bl) in enumerate(zip(levels, blocks)):
        assert lv.cpu().numpy().tobytes() == model[i].tobytes(), "level %d texels" % i
        want = _single(product, A, ctx, lv, bl.numel(), swz)
        got = bl.cpu().numpy().reshape(-1, 16)
        bad = int((got != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
        assert bad == 0, "level %d %s: %d blocks differ from the single call" % (i, tuple(lv.shape), bad)
        if ref is not None:
            r = ref.compress(model[i], block, quality, profile=profile, swizzle=swz, tweak=tweak).reshape(-1, 16)
            bad = int((got != r).any(axis=1).sum())
            assert bad == 0, "level %d %s: %d blocks differ from the reference" % (i, tuple(lv.shape), bad)
    return levels, blocks


@pytest.mark.parametrize("profile,block,quality,kernel", [
    ("ldr", (6, 6), "medium", "astc_compress_blocks_ldr_6x6m"),
    ("srgb", (6, 6), "medium", None),
    ("ldr", (4, 4), "fast", None),
    ("srgb", (4, 4), "fast", None),
])
def test_blocks_match_single_calls_and_reference(product, ref, A, profile, block, quality, kernel):
    prf = A.PRF_LDR_SRGB if profile == "srgb" else A.PRF_LDR
    q = {"medium": A.PRE_MEDIUM, "fast": A.PRE_FAST}[quality]
    ctx = _ctx(product, prf, block, q)
    try:
        if kernel:
            assert product.lib.astcenc_amd_context_kernel_name(ctx).decode() == kernel
        for w, h in ((255, 190), (300, 64)):
            _chain_vs_single(product, A, ctx, _image(A, w, h, "u8"), A.SWZ_RGBA, ref, prf, q, block, srgb=profile == "srgb")
    finally:
        product.context_free(ctx)


def test_generic_build_hdr_swizzle_and_alpha_scale(product, ref, A, monkeypatch):
    # the generic build of the same context
    monkeypatch.setenv("ASTCENC_AMD_KERNEL", "generic")
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        assert not product.lib.astcenc_amd_context_kernel_name(ctx).decode().endswith("6x6m")
        _chain_vs_single(product, A, ctx, _image(A, 130, 77, "u8", 1), A.SWZ_RGBA, ref, A.PRF_LDR, A.PRE_MEDIUM, (6, 6))
    finally:
        product.context_free(ctx)
    monkeypatch.delenv("ASTCENC_AMD_KERNEL")
    # HDR: F16 levels
    ctx = _ctx(product, A.PRF_HDR, (6, 6), A.PRE_MEDIUM)
    try:
        _chain_vs_single(product, A, ctx, _image(A, 200, 150, "f16", 2), A.SWZ_RGBA)
    finally:
        product.context_free(ctx)
    # a non-identity swizzle: the levels hold the stored channels, the swizzle applies when they are compressed
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        swz = (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_1)
        _chain_vs_single(product, A, ctx, _image(A, 97, 64, "u8", 3), swz, ref, A.PRF_LDR, A.PRE_MEDIUM, (6, 6))
    finally:
        product.context_free(ctx)

    # the alpha-scale pre-pass, per level
    def radius(cfg):
        cfg.a_scale_radius = 3
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM, tweak=radius)
    try:
        img = _image(A, 150, 100, "u8", 4)
        img[:50, :75, 3] = 0
        img[50:53, :, 3] = 9
        _chain_vs_single(product, A, ctx, img, A.SWZ_RGBA, ref, A.PRF_LDR, A.PRE_MEDIUM, (6, 6), tweak=radius)
    finally:
        product.context_free(ctx)


def test_round_trip_through_the_set_decoder(product, ref, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        levels, blocks = product.compress_mip_chain_device(ctx, _dev(_image(A, 512, 384, "u8", 5)))
        back = [torch.zeros(lv.shape, dtype=torch.uint8, device="cuda") for lv in levels]
        assert product.decompress_images_device(ctx, list(zip(back, blocks))) == A.SUCCESS
        torch.cuda.synchronize()
        for lv, bl, b in zip(levels, blocks, back):
            want = ref.decompress(bl.cpu().numpy(), lv.shape[1], lv.shape[0], (6, 6))
            assert np.array_equal(b.cpu().numpy(), want), tuple(lv.shape)
    finally:
        product.context_free(ctx)


def test_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        w, h = 100, 60
        img = _dev(_image(A, w, h, "u8", 6))
        err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, 0)
        err, lay = product.mip_chain_layout(cfg, w, h, A.TYPE_U8, 0)
        store = torch.full((lay.texels_len,), 0xAB, dtype=torch.uint8, device="cuda")
        out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")
        swz = A.Swizzle(*A.SWZ_RGBA)

        def compress(image=img.data_ptr(), levels=0, levels_len=lay.texels_len, blocks_len=lay.blocks_len, s=swz):
            return product.lib.astcenc_amd_compress_mip_chain_device(ctx, image, w, h, A.TYPE_U8, C.byref(s), levels, store.data_ptr(),
                                                                     levels_len, out.data_ptr(), blocks_len, None, None)

        def generate(image=img.data_ptr(), levels=0, levels_len=lay.texels_len):
            return product.lib.astcenc_amd_generate_mip_chain_device(ctx, image, w, h, A.TYPE_U8, levels, store.data_ptr(), levels_len, None)
        cases = [
            ("short levels_len", lambda: compress(levels_len=lay.texels_len - 1), A.ERR_OUT_OF_MEM, "levels_len"),
            ("short levels_len (generate)", lambda: generate(levels_len=lay.texels_len - 1), A.ERR_OUT_OF_MEM, "levels_len"),
            ("short blocks_len", lambda: compress(blocks_len=lay.blocks_len - 1), A.ERR_OUT_OF_MEM, "blocks_len"),
            ("bad swizzle", lambda: compress(s=A.Swizzle(A.SWZ_R, A.SWZ_G, A.SWZ_Z, A.SWZ_A)), A.ERR_BAD_SWIZZLE, "entry"),
            ("too many levels", lambda: compress(levels=lay.level_count + 1), A.ERR_BAD_PARAM, "level_count"),
            ("too many levels (generate)", lambda: generate(levels=lay.level_count + 1), A.ERR_BAD_PARAM, "level_count"),
            ("null image", lambda: compress(image=None), A.ERR_BAD_CONTEXT, "device_image"),
            ("null image (generate)", lambda: generate(image=None), A.ERR_BAD_CONTEXT, "device_image"),
        ]
        for what, call, want, word in cases:
            logged.clear()
            assert call() == want, what
            torch.cuda.synchronize()
            assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), what + ": a buffer was written"
            assert any(word in m for m in logged), (what, logged)
        # the null-buffer code is the single call's
        assert product.lib.astcenc_amd_compress_image_device(ctx, None, w, h, A.TYPE_U8, C.byref(swz), out.data_ptr(), out.numel(),
                                                             None, None) == A.ERR_BAD_CONTEXT
        # one level needs no levels buffer
        assert product.lib.astcenc_amd_generate_mip_chain_device(ctx, img.data_ptr(), w, h, A.TYPE_U8, 1, None, 0, None) == A.SUCCESS
        assert product.lib.astcenc_amd_generate_mip_chain_device(ctx, img.data_ptr(), w, h, A.TYPE_U8, 2, None, 1 << 20, None) == A.ERR_BAD_CONTEXT
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)


def test_stream_order_progress_and_cancel(product, A):
    seen = []
    cb = A.PROGRESS_CB(lambda p: seen.append(p))

    def with_progress(cfg):
        cfg.progress_callback = cb
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST, tweak=with_progress)
    try:
        # work queued on a side stream before the call: the image is written there, the call on the same stream sees it
        side = torch.cuda.Stream()
        src = _image(A, 2048, 2048, "u8", 7)
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            img = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            img.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_device(ctx, img, 0, A.SWZ_RGBA, stream=side)
            first = blocks[0].clone()
        side.synchronize()
        model = M.chain(src)
        for lv, m in zip(levels, model):
            assert lv.cpu().numpy().tobytes() == m.tobytes()
        want = _single(product, A, ctx, img, first.numel(), A.SWZ_RGBA)
        assert torch.equal(first, want)
        # progress: monotonic over the whole chain's blocks (more than one chunk: 2^18 blocks)
        assert sum(b.numel() for b in blocks) // 16 > 1 << 18
        assert len(seen) >= 2 and seen == sorted(seen) and seen[-1] == pytest.approx(100.0), seen
    finally:
        product.context_free(ctx)

    holder = {}
    cb2 = A.PROGRESS_CB(lambda p: product.lib.astcenc_compress_cancel(holder["ctx"]))

    def with_cancel(cfg):
        cfg.progress_callback = cb2
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST, tweak=with_cancel)
    holder["ctx"] = ctx
    try:
        # three chunks: a cancel from the first report stops the chain before its last chunk, as for a set
        img = _dev(_image(A, 3000, 2400, "u8", 8))
        err, cfg = product.config_init(A.PRF_LDR, 4, 4, 1, A.PRE_FASTEST, 0)
        err, lay = product.mip_chain_layout(cfg, 3000, 2400, A.TYPE_U8, 0)
        assert lay.blocks_len // 16 > 2 << 18
        store = torch.empty((lay.texels_len,), dtype=torch.uint8, device="cuda")
        out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")
        e = product.lib.astcenc_amd_compress_mip_chain_device(ctx, img.data_ptr(), 3000, 2400, A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), 0,
                                                              store.data_ptr(), lay.texels_len, out.data_ptr(), lay.blocks_len, None, None)
        torch.cuda.synchronize()
        n = _single_err(product, A, ctx)
        assert e == n
        untouched = int((out.cpu().numpy().reshape(-1, 16) == 0xAB).all(axis=1).sum())
        assert untouched == lay.blocks_len // 16 - (2 << 18)
    finally:
        product.context_free(ctx)


def _single_err(product, A, ctx):
    """What the single call returns on a cancelling context: a 3000 x 3000 image (three chunks)."""
    img = _dev(_image(A, 3000, 3000, "u8", 9))
    out = torch.full((750 * 750 * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    return product.lib.astcenc_amd_compress_image_device(ctx, img.data_ptr(), 3000, 3000, A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)),
                                                         out.data_ptr(), out.numel(), None, None)


def test_ktx_with_every_level(product, A, tmp_path):
    ctx = _ctx(product, A.PRF_LDR_SRGB, (6, 6), A.PRE_FASTEST)
    try:
        levels, blocks = product.compress_mip_chain_device(ctx, _dev(_image(A, 300, 130, "u8", 10)))
    finally:
        product.context_free(ctx)
    path = str(tmp_path / "chain.ktx")
    A.write_ktx_mips(path, blocks, 300, 130, (6, 6), srgb=True)
    got, w, h, block, srgb = A.read_ktx_mips(path)
    assert (w, h, block, srgb) == (300, 130, (6, 6, 1), True) and len(got) == len(blocks) == 9
    for g, b in zip(got, blocks):
        assert np.array_equal(g, b.cpu().numpy())
    first, w0, h0, d0, block0, srgb0 = A.read_ktx(path)
    assert np.array_equal(first, blocks[0].cpu().numpy()) and (w0, h0, d0, block0, srgb0) == (300, 130, 1, (6, 6, 1), True)
