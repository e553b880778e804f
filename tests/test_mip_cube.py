# SPDX-License-Identifier: Apache-2.0
"""Seamless cube-map edges of the windowed mip filters on the GPU (ASTCENC_AMD_MIP_EDGE_CUBE through the _filtered_ and
_weighted_ mip chain calls).

Every level equals the numpy model (tests/mip_cube_model.py) bit for bit: faces 1, 2, 3, 5, 33, 64, 100, 255 and 256 (the sizes
where CLAMP's chain crosses into its tail kernel or starts there; CUBE has one launch per level), one and two cubes, the three filters, U8, U8 sRGB, F16 and F32; a
6 x 1024^2 chain (interior tiles, border tiles and the grid-stride loop); alpha-weighted chains, whose channel 3 is the plain
CUBE chain's; the options compose as post(levels); CUBE with the box is the _ex_ call; compressed levels equal the volume call on
the model's levels and the chain reads back from a KTX cube map; invalid uses write nothing and are named in the log; CLAMP and
WRAP on the cube shapes still equal tests/mip_filter_model.py; the call keeps stream order on a side stream and reports
kernel_ms."""
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
import mip_cube_model as CM  # noqa: E402
from test_mip_filter import _bad_texels, _ctx, _dev, _image, _single_volume  # noqa: E402
from test_mip_weighted import _image as _image_alpha  # noqa: E402

FACES = [1, 2, 3, 5, 33, 64, 100, 255, 256]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]


def _profile(A, dtype, srgb):
    return A.PRF_LDR_SRGB if srgb else A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR


def _check_cube_chain(product, A, ctx, img, kind, weight=CM.NONE, srgb=False, options=None):
    flt = (kind, A.MIP_EDGE_CUBE)
    if weight == CM.NONE:
        got = product.generate_mip_chain_filtered_device(ctx, _dev(img), A.MIP_ARRAY, 0, options, flt)
    else:
        got = product.generate_mip_chain_weighted_device(ctx, _dev(img), A.MIP_ARRAY, 0, options, flt, weighting=A.MIP_WEIGHT_ALPHA)
    torch.cuda.synchronize()
    want = CM.chain(img, kind, weight, srgb=srgb)
    if options is not None:
        want = P.post(want, F.ARRAY, options[0], options[1])
    assert len(got) == len(want)
    got = [g.cpu().numpy() for g in got]
    for i, (g, m) in enumerate(zip(got, want)):
        bad = _bad_texels(g, m)
        print("%s %s filter %d weight %d srgb %d level %d: %d texels differ" % (img.dtype, img.shape, kind, weight, srgb, i, bad))
        assert bad == 0, (img.dtype, img.shape, kind, weight, srgb, options, "level %d: %d texels differ" % (i, bad))
    return got


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_levels_match_the_model(product, A, name, dtype, srgb):
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for n, s in enumerate(FACES):
            for cubes in (1, 2):
                img = _image(dtype, (6 * cubes, s, s), 300 + 2 * n + cubes, inf=dtype != np.uint8 and s in (33, 100))
                for kind in F.KINDS:
                    _check_cube_chain(product, A, ctx, img, kind, CM.NONE, srgb)
    finally:
        product.context_free(ctx)


def test_large_cube(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        _check_cube_chain(product, A, ctx, _image(np.uint8, (6, 1024, 1024), 21), F.LANCZOS3)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
def test_weighted_levels_match_the_model(product, A, name, dtype, srgb):
    ctx = _ctx(product, _profile(A, dtype, srgb), (6, 6))
    try:
        for n, (z, s) in enumerate([(6, 1), (6, 2), (6, 3), (12, 5), (6, 33), (6, 64), (12, 100), (6, 255), (6, 256), (6, 600)]):
            img = _image_alpha(dtype, (z, s, s), 400 + n, special=dtype != np.uint8 and s in (33, 100))
            for kind in F.KINDS if s < 600 else (F.LANCZOS3,):
                got = _check_cube_chain(product, A, ctx, img, kind, CM.ALPHA, srgb)
                plain = product.generate_mip_chain_filtered_device(ctx, _dev(img), A.MIP_ARRAY, 0, None, (kind, A.MIP_EDGE_CUBE))
                for i, (g, p) in enumerate(zip(got, plain)):
                    assert _bad_texels(g[..., 3:4].repeat(4, -1), p.cpu().numpy()[..., 3:4].repeat(4, -1)) == 0, (dtype, s, kind, i, "channel 3")
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f16", np.float16)])
def test_options_compose(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for z, s in [(6, 33), (12, 100)]:
            img = _image(dtype, (z, s, s), 30)
            for flags in (P.NORMALIZE, P.ALPHA_COVERAGE, P.NORMALIZE | P.ALPHA_COVERAGE):
                _check_cube_chain(product, A, ctx, img, F.LANCZOS3, CM.NONE, options=(flags, 0.5))
                _check_cube_chain(product, A, ctx, img, F.MITCHELL, CM.ALPHA, options=(flags, 0.5))
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("name,dtype", [("u8", np.uint8), ("f32", np.float32)])
def test_box_is_the_ex_call(product, A, name, dtype):
    ctx = _ctx(product, A.PRF_LDR if dtype == np.uint8 else A.PRF_HDR, (6, 6))
    try:
        for z, s in [(6, 40), (12, 33)]:
            img = _dev(_image(dtype, (z, s, s), 31))
            for opts in (None, (A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)):
                plain = [t.cpu().numpy().tobytes() for t in product.generate_mip_chain_ex_device(ctx, img, A.MIP_ARRAY, 0, opts)]
                got = product.generate_mip_chain_filtered_device(ctx, img, A.MIP_ARRAY, 0, opts, (A.MIP_FILTER_BOX, A.MIP_EDGE_CUBE))
                assert [t.cpu().numpy().tobytes() for t in got] == plain, (z, s, opts)
    finally:
        product.context_free(ctx)


@pytest.mark.parametrize("block", [(6, 6), (4, 4)])
def test_compressed_levels_equal_the_volume_call(product, A, block, tmp_path):
    ctx = _ctx(product, A.PRF_LDR, block, A.PRE_FASTEST)
    try:
        img = _image(np.uint8, (6, 72, 72), 32)
        levels, blocks = product.compress_mip_chain_filtered_device(ctx, _dev(img), A.MIP_ARRAY, 0, None, (A.MIP_FILTER_KAISER, A.MIP_EDGE_CUBE))
        torch.cuda.synchronize()
        assert product.last_kernel_ms > 0
        model = CM.chain(img, F.KAISER)
        assert len(levels) == len(model)
        for i, (lv, bl, m) in enumerate(zip(levels, blocks, model)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0, "level %d texels" % i
            want = _single_volume(product, A, ctx, _dev(m), bl.numel())
            bad = int((bl.cpu().numpy().reshape(-1, 16) != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
            assert bad == 0, "level %d: %d blocks differ from the volume call" % (i, bad)
    finally:
        product.context_free(ctx)
    path = str(tmp_path / "cube.ktx")
    A.write_ktx_chain(path, blocks, 72, 72, block, faces=6)
    got = A.read_ktx_chain(path)
    assert (got["w"], got["h"], got["layers"], got["faces"], got["block"][:2], len(got["levels"])) == (72, 72, 0, 6, block, 7)
    for g, b in zip(got["levels"], blocks):
        assert np.array_equal(g, b.cpu().numpy())


def test_cube_errors_write_nothing(product, A):
    ctx = _ctx(product, A.PRF_LDR, (6, 6), A.PRE_FASTEST)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    swz = A.Swizzle(*A.SWZ_RGBA)
    try:
        err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, 0)
        # (w, h, d, kind, edge): CUBE with a VOLUME of depth 1 and 6, with dim_x != dim_y, with 5 and 7 layers; an unknown edge
        cases = [(40, 40, 1, A.MIP_VOLUME, A.MIP_EDGE_CUBE), (40, 40, 6, A.MIP_VOLUME, A.MIP_EDGE_CUBE), (40, 36, 6, A.MIP_ARRAY, A.MIP_EDGE_CUBE),
                 (40, 40, 5, A.MIP_ARRAY, A.MIP_EDGE_CUBE), (40, 40, 7, A.MIP_ARRAY, A.MIP_EDGE_CUBE), (40, 40, 6, A.MIP_ARRAY, 3)]
        for w, h, d, mip_kind, edge in cases:
            img = _dev(_image(np.uint8, (d, h, w), 33))
            err, lay = product.mip_chain_volume_layout(cfg, w, h, d, mip_kind, A.TYPE_U8, 0)
            assert err == 0
            store = torch.full((lay.texels_len,), 0xAB, dtype=torch.uint8, device="cuda")
            out = torch.full((lay.blocks_len,), 0xAB, dtype=torch.uint8, device="cuda")

            def generate(flt, wt):
                return product.lib.astcenc_amd_generate_mip_chain_weighted_device(ctx, img.data_ptr(), w, h, d, mip_kind, A.TYPE_U8, 0, None,
                                                                                  C.byref(A.MipFilter(*flt)), wt, store.data_ptr(),
                                                                                  lay.texels_len, None)

            def compress(flt, wt):
                return product.lib.astcenc_amd_compress_mip_chain_weighted_device(ctx, img.data_ptr(), w, h, d, mip_kind, A.TYPE_U8,
                                                                                  C.byref(swz), 0, None, C.byref(A.MipFilter(*flt)), wt,
                                                                                  store.data_ptr(), lay.texels_len, out.data_ptr(),
                                                                                  lay.blocks_len, None, None)

            def generate_filtered(flt, wt):
                return product.lib.astcenc_amd_generate_mip_chain_filtered_device(ctx, img.data_ptr(), w, h, d, mip_kind, A.TYPE_U8, 0, None,
                                                                                  C.byref(A.MipFilter(*flt)), store.data_ptr(),
                                                                                  lay.texels_len, None)
            for kind in (A.MIP_FILTER_LANCZOS3, A.MIP_FILTER_MITCHELL, A.MIP_FILTER_BOX):
                for wt in (None, C.byref(A.MipWeighting(A.MIP_WEIGHT_ALPHA))):
                    for call in (generate, compress, generate_filtered):
                        logged.clear()
                        assert call((kind, edge), wt) == A.ERR_BAD_PARAM, (w, h, d, mip_kind, edge, kind)
                        torch.cuda.synchronize()
                        assert bool((store == 0xAB).all()) and bool((out == 0xAB).all()), (w, h, d, mip_kind, edge, kind, "a buffer was written")
                        assert any("filter" in m for m in logged), (w, h, d, mip_kind, edge, kind, logged)
        # ... and the valid form of the last shape goes through
        flt = C.byref(A.MipFilter(A.MIP_FILTER_KAISER, A.MIP_EDGE_CUBE))
        assert product.lib.astcenc_amd_compress_mip_chain_filtered_device(ctx, img.data_ptr(), 40, 40, 6, A.MIP_ARRAY, A.TYPE_U8, C.byref(swz), 0,
                                                                          None, flt, store.data_ptr(), lay.texels_len, out.data_ptr(),
                                                                          lay.blocks_len, None, None) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out == 0xAB).all()) and not bool((store == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)


def test_clamp_and_wrap_on_cube_shapes(product, A):
    """The edges next to the new one, on the shapes of this file: still the model of tests/mip_filter_model.py, and not CUBE's."""
    ctx = _ctx(product, A.PRF_LDR, (6, 6))
    try:
        for z, s in [(6, 5), (12, 33), (6, 100), (6, 256)]:
            img = _image(np.uint8, (z, s, s), 34)
            cube = CM.chain(img, F.LANCZOS3)
            for edge in (F.CLAMP, F.WRAP):
                got = product.generate_mip_chain_filtered_device(ctx, _dev(img), A.MIP_ARRAY, 0, None, (F.LANCZOS3, edge))
                torch.cuda.synchronize()
                for i, (g, m) in enumerate(zip(got, F.chain(img, F.ARRAY, F.LANCZOS3, edge))):
                    assert _bad_texels(g.cpu().numpy(), m) == 0, (z, s, edge, i)
                assert _bad_texels(got[1].cpu().numpy(), cube[1]) > 0, (z, s, edge)
    finally:
        product.context_free(ctx)


def test_stream_order_on_a_side_stream(product, A):
    ctx = _ctx(product, A.PRF_LDR, (4, 4), A.PRE_FASTEST)
    try:
        side = torch.cuda.Stream()
        src = _image(np.uint8, (6, 320, 320), 35)
        host = torch.from_numpy(src).pin_memory()
        with torch.cuda.stream(side):
            img = torch.empty(src.shape, dtype=torch.uint8, device="cuda")
            torch.cuda._sleep(20_000_000)
            img.copy_(host, non_blocking=True)
            levels, blocks = product.compress_mip_chain_filtered_device(ctx, img, A.MIP_ARRAY, 0, None, (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CUBE),
                                                                        stream=side)
            first = [lv.clone() for lv in levels]
        side.synchronize()
        assert product.last_kernel_ms > 0
        for lv, m in zip(first, CM.chain(src, F.LANCZOS3)):
            assert _bad_texels(lv.cpu().numpy(), m) == 0
    finally:
        product.context_free(ctx)
