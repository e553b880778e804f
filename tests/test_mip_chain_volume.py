# SPDX-License-Identifier: Apache-2.0
"""Mip chains of texture arrays, cube maps and volumes on the GPU (astcenc_amd_generate_mip_chain_volume_device /
astcenc_amd_compress_mip_chain_volume_device).

VOLUME levels equal the numpy model (tests/mip_model_3d.py) bit for bit; every ARRAY layer equals the 2D call on that layer
alone; a VOLUME of depth 1 equals the 2D call; every level's blocks equal astcenc_amd_compress_volume_device on that level (and
the reference's on one small volume); the chain round-trips through the set decoder; bad arguments write nothing and are
named in the log; the call keeps stream order on a side stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402

VOLUME_SIZES = [(1, 1, 9), (5, 3, 7), (64, 64, 64), (130, 66, 33), (256, 256, 256), (1024, 1024, 4)]      # (w, h, d)


def _ctx(lib, profile, block, quality, tweak=None):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality, 0)
    assert err == 0
    if tweak:
        tweak(cfg)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def _volume(A, w, h, d, kind, seed=0):
    rng = np.random.default_rng(seed + w * 7 + h * 3 + d)
    if kind == "u8":
        # smooth content with some hard edges, slice by slice
        base = A.synthetic_image(w, h * d, 0x9E3779B1 + seed).reshape(d, h, w, 4).copy()
        base[rng.random((d, h, w)) < 0.1] = rng.integers(0, 256, 4, dtype=np.uint8)
        return base
    if kind == "f16":
        return A.synthetic_hdr_image(w, h * d, seed).reshape(d, h, w, 4).astype(np.float16)
    return (rng.standard_normal((d, h, w, 4)) * 50).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bad_texels(g, m):
    """The texels of g and m (same shape) whose bytes differ."""
    n = 4 * m.dtype.itemsize
    return int((np.ascontiguousarray(g).view(np.uint8).reshape(-1, n) != np.ascontiguousarray(m).view(np.uint8).reshape(-1, n)).any(axis=1).sum())


@pytest.mark.parametrize("profile,kind", [("ldr", "u8"), ("srgb", "u8"), ("hdr", "f16"), ("ldr", "f32")])
def test_volume_levels_match_numpy_model(product, A, profile, kind):
    prf = {"ldr": A.PRF_LDR, "srgb": A.PRF_LDR_SRGB, "hdr": A.PRF_HDR}[profile]
    ctx = _ctx(product, prf, (4, 4, 4), A.PRE_FASTEST)
    try:
        for w, h, d in VOLUME_SIZES:
            vol = _volume(A, w, h, d, kind)
            full = V.full_levels(w, h, d)
            want_full = V.chain_volume(vol, 0, srgb=profile == "srgb")
            for levels in (0, min(3, full)):
                got = product.generate_mip_chain_volume_device(ctx, _dev(vol), A.MIP_VOLUME, levels)
                torch.cuda.synchronize()
                want = want_full if levels == 0 else want_full[:levels]
                assert len(got) == len(want)
                for i, (g, m) in enumerate(zip(got, want)):
                    g = g.cpu().numpy()
                    assert g.shape == m.shape, ((w, h, d), i, g.shape, m.shape)
                    bad = _bad_texels(g, m)
                    assert bad == 0, (profile, kind, (w, h, d), levels, "level %d: %d texels differ" % (i, bad))
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("kind,profile", [("u8", "ldr"), ("u8", "srgb"), ("f16", "hdr"), ("f32", "ldr")])
def test_array_layers_equal_the_2d_call(product, A, kind, profile):
    prf = {"ldr": A.PRF_LDR, "srgb": A.PRF_LDR_SRGB, "hdr": A.PRF_HDR}[profile]
    ctx = _ctx(product, prf, (6, 6), A.PRE_FASTEST)
    try:
        sizes = [(255, 255, 6), (256, 256, 64), (4096, 4096, 3)] if kind == "u8" else [(255, 255, 6), (256, 256, 64), (1000, 600, 3)]
        for w, h, layers in sizes:
            arr = _dev(_volume(A, w, h, layers, kind, 1))
            got = product.generate_mip_chain_volume_device(ctx, arr, A.MIP_ARRAY)
            assert len(got) == M.full_levels(w, h)
            for l in range(layers):
                want = product.generate_mip_chain_device(ctx, arr[l].contiguous())
                assert len(want) == len(got)
                for i, (g, m) in enumerate(zip(got, want)):
                    assert g.shape[0] == layers and g[l].cpu().numpy().tobytes() == m.cpu().numpy().tobytes(), \
                        ((w, h, layers), "layer %d level %d" % (l, i))
        # the model agrees on a small array (cube faces)
        cube = _volume(A, 37, 37, 6, kind, 2)
        got = product.generate_mip_chain_volume_device(ctx, _dev(cube), A.MIP_ARRAY)
        for i, m in enumerate(V.chain_array(cube, srgb=profile == "srgb")):
            assert _bad_texels(got[i].cpu().numpy(), m) == 0, i
    finally:
        product.context_free(ctx)


def test_volume_of_depth_one_equals_the_2d_call(product, A):
    for prf, kind in ((A.PRF_LDR, "u8"), (A.PRF_LDR_SRGB, "u8"), (A.PRF_HDR, "f16"), (A.PRF_LDR, "f32")):
        ctx = _ctx(product, prf, (6, 6), A.PRE_FASTEST)
        try:
            for w, h in ((1, 1), (5, 3), (17, 4096), (255, 190), (1000, 1000), (4096, 4096)):
                img = _dev(_volume(A, w, h, 1, kind, 3))
                got = product.generate_mip_chain_volume_device(ctx, img, A.MIP_VOLUME)
                want = product.generate_mip_chain_device(ctx, img[0])
                assert len(got) == len(want)
                for i, (g, m) in enumerate(zip(got, want)):
                    assert g.shape[0] == 1 and g[0].cpu().numpy().tobytes() == m.cpu().numpy().tobytes(), ((w, h), kind, i)
        finally:
            product.context_free(ctx)


def _single_volume(lib, A, ctx, img, nbytes, swz):
    out = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    types = {torch.uint8: A.TYPE_U8, torch.float16: A.TYPE_F16, torch.float32: A.TYPE_F32}
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), img.shape[2], img.shape[1], img.shape[0], types[img.dtype],
                                                     C.byref(A.Swizzle(*swz)), out.data_ptr(), out.numel(),
                                                     A.torch_stream(), None)
    assert err == A.SUCCESS
    return out


@pytest.mark.parametrize("mip_kind,block,quality", [
    ("array", (6, 6), "fastest"), ("array", (4, 4), "medium"),
    ("volume", (4, 4, 4), "fastest"), ("volume", (4, 4, 4), "medium"), ("volume", (6, 6, 6), "fastest"), ("volume", (6, 6), "medium"),
])
def test_blocks_equal_the_volume_call(product, A, mip_kind, block, quality):
    q = {"fastest": A.PRE_FASTEST, "medium": A.PRE_MEDIUM}[quality]
    kind = A.MIP_ARRAY if mip_kind == "array" else A.MIP_VOLUME
    ctx = _ctx(product, A.PRF_LDR, block, q)
    try:
        for w, h, d in ((130, 66, 6), (64, 48, 12)):
            vol = _volume(A, w, h, d, "u8", 4)
            levels, blocks = product.compress_mip_chain_volume_device(ctx, _dev(vol), kind)
            torch.cuda.synchronize()
            assert product.last_kernel_ms > 0
            model = V.chain_volume(vol) if kind == A.MIP_VOLUME else V.chain_array(vol)
            assert len(levels) == len(model)
            for i, (lv, bl) in enumerate(zip(levels, blocks)):
                assert lv.cpu().numpy().tobytes() == model[i].tobytes(), "level %d texels" % i
                want = _single_volume(product, A, ctx, lv, bl.numel(), A.SWZ_RGBA)
                bad = int((bl.cpu().numpy().reshape(-1, 16) != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
                assert bad == 0, "level %d %s: %d blocks differ from the volume call" % (i, tuple(lv.shape), bad)
    finally:
        product.context_free(ctx)


def test_small_volume_blocks_equal_the_reference(product, ref, A):
    ctx = _ctx(product, A.PRF_LDR, (4, 4, 4), A.PRE_MEDIUM)
    try:
        vol = _volume(A, 24, 20, 12, "u8", 5)
        levels, blocks = product.compress_mip_chain_volume_device(ctx, _dev(vol), A.MIP_VOLUME)
        torch.cuda.synchronize()
        for i, (m, bl) in enumerate(zip(V.chain_volume(vol), blocks)):
            r = ref.compress(m, (4, 4, 4), A.PRE_MEDIUM, profile=A.PRF_LDR).reshape(-1, 16)
            bad = int((bl.cpu().numpy().reshape(-1, 16) != r).any(axis=1).sum())
            assert bad == 0, "level %d %s: %d blocks differ from the reference" % (i, m.shape, bad)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("mip_kind,block", [("array", (6, 6)), ("volume", (4, 4, 4))])
def test_round_trip_through_the_set_decoder(product, ref, A, mip_kind, block):
    kind = A.MIP_ARRAY if mip_kind == "array" else A.MIP_VOLUME
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_MEDIUM)
    try:
        levels, blocks = product.compress_mip_chain_volume_device(ctx, _dev(_volume(A, 96, 80, 6, "u8", 6)), kind)
        back = [torch.zeros(lv.shape, dtype=torch.uint8, device="cuda") for lv in levels]
        assert product.decompress_images_device(ctx, list(zip(back, blocks))) == A.SUCCESS
        torch.cuda.synchronize()
        for lv, bl, b in zip(levels, blocks, back):
            want = ref.decompress(bl.cpu().numpy(), lv.shape[2], lv.shape[1], block, depth=lv.shape[0])
            assert np.array_equal(b.cpu().numpy(), want), tuple(lv.shape)
    finally:
        product.context_free(ctx)


def test_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    ctx3 = _ctx(product, A.PRF_LDR, (4, 4, 4), A.PRE_MEDIUM)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        w, h, d = 100, 60, 6
        img = _dev(_volume(A, w, h, d, "u8", 7))
        err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, 0)
        err, lay = product.mip_chain_volume_layout(cfg, w, h, d, A.MIP_VOLUME, A.TYPE_U8, 0)
        assert err == A.SUCCESS
        store = torch.full((lay.texels_len,), 0xAB, dtype=torch.uint8, device="cuda")
        out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")
        swz = A.Swizzle(*A.SWZ_RGBA)

        def compress(image=img.data_ptr(), levels=0, levels_ptr=store.data_ptr(), levels_len=lay.texels_len, blocks_ptr=out.data_ptr(),
                     blocks_len=lay.blocks_len, s=swz, kind=A.MIP_VOLUME, c=ctx, dz=d):
            return product.lib.astcenc_amd_compress_mip_chain_volume_device(c, image, w, h, dz, kind, A.TYPE_U8, C.byref(s), levels, levels_ptr,
                                                                            levels_len, blocks_ptr, blocks_len, None, None)

        def generate(image=img.data_ptr(), levels=0, levels_ptr=store.data_ptr(), levels_len=lay.texels_len, kind=A.MIP_VOLUME, dz=d, c=ctx):
            return product.lib.astcenc_amd_generate_mip_chain_volume_device(c, image, w, h, dz, kind, A.TYPE_U8, levels, levels_ptr,
                                                                            levels_len, None)
        cases = [
            ("short levels_len", lambda: compress(levels_len=lay.texels_len - 1), A.ERR_OUT_OF_MEM, "levels_len"),
            ("short levels_len (generate)", lambda: generate(levels_len=lay.texels_len - 1), A.ERR_OUT_OF_MEM, "levels_len"),
            ("short blocks_len", lambda: compress(blocks_len=lay.blocks_len - 1), A.ERR_OUT_OF_MEM, "blocks_len"),
            ("bad swizzle", lambda: compress(s=A.Swizzle(A.SWZ_R, A.SWZ_G, A.SWZ_Z, A.SWZ_A)), A.ERR_BAD_SWIZZLE, "entry"),
            ("too many levels", lambda: compress(levels=lay.level_count + 1), A.ERR_BAD_PARAM, "level_count"),
            ("too many levels (generate)", lambda: generate(levels=lay.level_count + 1), A.ERR_BAD_PARAM, "level_count"),
            ("null image", lambda: compress(image=None), A.ERR_BAD_CONTEXT, "device_image"),
            ("null image (generate)", lambda: generate(image=None), A.ERR_BAD_CONTEXT, "device_image"),
            ("null levels", lambda: compress(levels_ptr=None), A.ERR_BAD_CONTEXT, "device_levels"),
            ("null levels (generate)", lambda: generate(levels_ptr=None), A.ERR_BAD_CONTEXT, "device_levels"),
            ("null blocks", lambda: compress(blocks_ptr=None), A.ERR_BAD_CONTEXT, "device_blocks"),
            ("bad kind", lambda: compress(kind=2), A.ERR_BAD_PARAM, "kind"),
            ("bad kind (generate)", lambda: generate(kind=7), A.ERR_BAD_PARAM, "kind"),
            ("zero depth", lambda: generate(dz=0), A.ERR_BAD_PARAM, "dim_z"),
            ("array with a 3D footprint", lambda: compress(kind=A.MIP_ARRAY, c=ctx3), A.ERR_BAD_PARAM, "3D footprint"),
            ("array with a 3D footprint (generate)", lambda: generate(kind=A.MIP_ARRAY, c=ctx3), A.ERR_BAD_PARAM, "3D footprint"),
        ]
        for what, call, want, word in cases:
            logged.clear()
            assert call() == want, what
            torch.cuda.synchronize()
            assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), what + ": a buffer was written"
            assert any(word in m for m in logged), (what, logged)
        # one level needs no levels buffer
        assert generate(levels=1, levels_ptr=None, levels_len=0) == A.SUCCESS
        # a null context or swizzle
        assert product.lib.astcenc_amd_compress_mip_chain_volume_device(ctx, img.data_ptr(), w, h, d, 1, A.TYPE_U8, None, 0, store.data_ptr(),
                                                                        lay.texels_len, out.data_ptr(), lay.blocks_len, None, None) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((store == 0xAB).all()) and bool((out == 0xAB).all())
        # and the calls work with these very buffers
        assert compress() == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)
        product.context_free(ctx3)


def test_stream_order_on_a_side_stream(product, A):
    ctx = _ctx(product, A.PRF_LDR, (4, 4, 4), A.PRE_FASTEST)
    try:
        side = torch.cuda.Stream()
        src = _volume(A, 256, 256, 32, "u8", 8)
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            vol = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            vol.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_volume_device(ctx, vol, A.MIP_VOLUME, 0, A.SWZ_RGBA, stream=side)
            first = blocks[0].clone()
        side.synchronize()
        assert product.last_kernel_ms > 0
        for lv, m in zip(levels, V.chain_volume(src)):
            assert lv.cpu().numpy().tobytes() == m.tobytes()
        want = _single_volume(product, A, ctx, vol, first.numel(), A.SWZ_RGBA)
        assert torch.equal(first, want)
    finally:
        product.context_free(ctx)


def test_ktx_of_a_compressed_cube_map_and_volume(product, A, tmp_path):
    ctx = _ctx(product, A.PRF_LDR_SRGB, (6, 6), A.PRE_FASTEST)
    try:
        levels, blocks = product.compress_mip_chain_volume_device(ctx, _dev(_volume(A, 64, 64, 12, "u8", 9)), A.MIP_ARRAY)
    finally:
        product.context_free(ctx)
    path = str(tmp_path / "cube_array.ktx")
    A.write_ktx_chain(path, blocks, 64, 64, (6, 6), layers=2, faces=6, srgb=True)
    got = A.read_ktx_chain(path)
    assert (got["layers"], got["faces"], got["srgb"], len(got["levels"])) == (2, 6, True, 7)
    for g, b in zip(got["levels"], blocks):
        assert np.array_equal(g, b.cpu().numpy())
    ctx = _ctx(product, A.PRF_LDR, (4, 4, 4), A.PRE_FASTEST)
    try:
        levels, blocks = product.compress_mip_chain_volume_device(ctx, _dev(_volume(A, 32, 16, 8, "u8", 10)), A.MIP_VOLUME)
    finally:
        product.context_free(ctx)
    path = str(tmp_path / "volume.ktx")
    A.write_ktx_chain(path, blocks, 32, 16, (4, 4, 4), depth=8)
    got = A.read_ktx_chain(path)
    assert (got["w"], got["h"], got["depth"], got["block"], len(got["levels"])) == (32, 16, 8, (4, 4, 4), 6)
    for g, b in zip(got["levels"], blocks):
        assert np.array_equal(g, b.cpu().numpy())
