# SPDX-License-Identifier: Apache-2.0
"""Image sets on the GPU (astcenc_amd_compress_images_device / astcenc_amd_decompress_images_device).

Every entry of a set must come out exactly as one call of the single-image entry point on that entry writes it
(astcenc_amd_compress_volume_device / astcenc_amd_decompress_image_device), and every 2D entry exactly as the reference
writes it (oracle/_ref, host API).  Then: a mip chain, a set larger than one chunk of launches (progress, cancel), the
alpha-scale pre-pass per entry, bad entries (nothing written), and the decoder."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES_2D = [(1, 1), (5, 3), (17, 4096), (255, 190), (1024, 1024)]     # (w, h)


def _ctx(lib, A, profile, block, quality, flags=0, tweak=None, threads=1, options=None):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality, flags)
    assert err == 0
    if tweak:
        tweak(cfg)
    err, ctx = lib.context_alloc(cfg, threads)
    assert err == 0, err
    for opt, v in (options or {}).items():
        assert lib.lib.astcenc_amd_context_set_option(ctx, opt, v) == 0
    return ctx, cfg


def _blocks(dims, block):
    w, h = dims[0], dims[1]
    d = dims[2] if len(dims) > 2 else 1
    bz = block[2] if len(block) > 2 else 1
    return -(-w // block[0]) * -(-h // block[1]) * -(-d // bz)


def _image(A, w, h, d=1, kind="u8", seed=0):
    """[H, W, 4] (d == 1) or [D, H, W, 4] numpy image of the given kind."""
    slices = []
    for z in range(d):
        if kind == "hdr":
            im = A.synthetic_hdr_image(w, h, seed + 7 * z).astype(np.float16)
        else:
            im = A.synthetic_image(w, h, 0x9E3779B1 + seed + 13 * z)
            if kind == "transparent":
                im = im.copy()
                im[: h // 2, : w // 2, 3] = 0              # fully transparent quadrant, partly transparent edge
                im[h // 2: h // 2 + 3, :, 3] = 9
            elif kind in ("f16", "f32"):
                im = (im.astype(np.float32) / 255.0).astype(np.float16 if kind == "f16" else np.float32)
        slices.append(im)
    return slices[0] if d == 1 else np.stack(slices)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _single(lib, A, ctx, img, nblocks, swz):
    """The entry through astcenc_amd_compress_volume_device."""
    out = torch.full((nblocks * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    d = img.shape[0] if img.dim() == 4 else 1
    h, w = img.shape[-3], img.shape[-2]
    types = {torch.uint8: A.TYPE_U8, torch.float16: A.TYPE_F16, torch.float32: A.TYPE_F32}
    err = lib.lib.astcenc_amd_compress_volume_device(ctx, img.data_ptr(), w, h, d, types[img.dtype], C.byref(A.Swizzle(*swz)),
                                                     out.data_ptr(), out.numel(), A.torch_stream(), None)
    return err, out


def _set_vs_single(lib, A, ctx, entries, block, ref=None, profile=None, quality=None, tweak=None, after_set=None):
    """entries: [(numpy image, swizzle)].  One set call (then after_set()), then every entry through the single call (and 2D
    ones through the reference): byte-identical."""
    imgs = [_dev(im) for im, _ in entries]
    outs = [torch.full((_blocks((im.shape[-2], im.shape[-3]) + ((im.shape[0],) if im.ndim == 4 else ()), block) * 16,), 0xAB,
                       dtype=torch.uint8, device="cuda") for im, _ in entries]
    err = lib.compress_images_device(ctx, [(i, o, swz) for i, o, (_, swz) in zip(imgs, outs, entries)])
    assert err == A.SUCCESS, err
    torch.cuda.synchronize()
    if after_set:
        after_set()
    for k, ((im, swz), d_img, d_out) in enumerate(zip(entries, imgs, outs)):
        e, want = _single(lib, A, ctx, d_img, d_out.numel() // 16, swz)
        assert e == A.SUCCESS
        got = d_out.cpu().numpy().reshape(-1, 16)
        bad = int((got != want.cpu().numpy().reshape(-1, 16)).any(axis=1).sum())
        assert bad == 0, ("entry %d %s: %d blocks differ from the single call" % (k, im.shape, bad))
        if ref is not None and im.ndim == 3:
            r = ref.compress(im, block, quality, profile=profile, swizzle=swz, tweak=tweak).reshape(-1, 16)
            bad = int((got != r).any(axis=1).sum())
            assert bad == 0, ("entry %d %s: %d blocks differ from the reference" % (k, im.shape, bad))
    return outs


def _mixed_set(A, hdr=False):
    """The sizes of SIZES_2D in U8 / F16 / F32, non-identity swizzles, a transparent entry."""
    kinds = ["hdr", "f32", "f16", "hdr", "u8"] if hdr else ["u8", "f16", "f32", "transparent", "u8"]
    swz = [A.SWZ_RGBA, (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A), A.SWZ_RGBA, (A.SWZ_R, A.SWZ_R, A.SWZ_R, A.SWZ_G),
           (A.SWZ_R, A.SWZ_G, A.SWZ_B, A.SWZ_1)]
    return [(_image(A, w, h, kind=k, seed=i), s) for i, ((w, h), k, s) in enumerate(zip(SIZES_2D, kinds, swz))]


@pytest.mark.parametrize("profile,block,quality,kernel", [
    ("ldr", (6, 6), "medium", "astc_compress_blocks_ldr_6x6m"),
    ("ldr", (8, 8), "thorough", "astc_compress_blocks_ldr_8x8t"),
    ("hdr", (6, 6), "medium", "astc_compress_blocks_hdr_6x6m"),
    ("ldr", (5, 5), "medium", "astc_compress_blocks_ldr64"),
    ("ldr", (10, 8), "medium", "astc_compress_blocks_ldr"),
])
def test_set_matches_single_calls_and_reference(product, ref, A, profile, block, quality, kernel):
    prf = A.PRF_HDR if profile == "hdr" else A.PRF_LDR
    q = {"medium": A.PRE_MEDIUM, "thorough": A.PRE_THOROUGH}[quality]
    ctx, _ = _ctx(product, A, prf, block, q)
    try:
        assert product.lib.astcenc_amd_context_kernel_name(ctx).decode() == kernel
        _set_vs_single(product, A, ctx, _mixed_set(A, hdr=profile == "hdr"), block, ref, prf, q)
    finally:
        product.context_free(ctx)


def test_set_of_volumes_and_of_multi_slice_entries(product, A):
    # 3D footprint: volume entries
    ctx, _ = _ctx(product, A, A.PRF_LDR, (4, 4, 4), A.PRE_MEDIUM)
    try:
        vols = [(_image(A, 1, 1, 1), A.SWZ_RGBA), (_image(A, 5, 3, 2, seed=1), A.SWZ_RGBA),
                (_image(A, 33, 17, 9, seed=2), (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A)), (_image(A, 64, 64, 8, kind="f16", seed=3), A.SWZ_RGBA)]
        _set_vs_single(product, A, ctx, vols, (4, 4, 4))
    finally:
        product.context_free(ctx)
    # 2D footprint: multi-slice entries, per-slice default and the reference's slice-0 fast load
    for options in ({}, {A.OPT_PER_SLICE_FAST_LOAD: 0}):
        ctx, _ = _ctx(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM, options=options)
        try:
            stacks = [(_image(A, 40, 30, 3, seed=4), A.SWZ_RGBA), (_image(A, 7, 7, 1, seed=5), A.SWZ_RGBA),
                      (_image(A, 100, 61, 4, seed=6), (A.SWZ_R, A.SWZ_G, A.SWZ_B, A.SWZ_1)), (_image(A, 13, 200, 2, seed=7), A.SWZ_RGBA)]
            _set_vs_single(product, A, ctx, stacks, (6, 6))
        finally:
            product.context_free(ctx)


def test_set_through_a_run_time_build(product, ref, A, tmp_path, monkeypatch):
    from jit_builds import prewarm
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    prewarm(str(tmp_path / "cache"), [(A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0)])       # (compiled on the CPU, found in the cache)
    ctx, _ = _ctx(product, A, A.PRF_LDR, (6, 6), A.PRE_THOROUGH)
    try:
        assert product.lib.astcenc_amd_context_kernel_name(ctx).decode().startswith("astc_compress_blocks_jit_")
        _set_vs_single(product, A, ctx, _mixed_set(A), (6, 6), ref, A.PRF_LDR, A.PRE_THOROUGH)
    finally:
        product.context_free(ctx)


def _mip_chain(A, size):
    levels = [A.synthetic_image(size, size)]
    while levels[-1].shape[0] > 1:
        a = levels[-1].astype(np.uint32)
        levels.append(((a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2] + 2) // 4).astype(np.uint8))
    return levels


def test_mip_chain_in_one_call_and_back(product, ref, A):
    levels = _mip_chain(A, 1024)
    assert len(levels) == 11
    ctx, _ = _ctx(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        outs = _set_vs_single(product, A, ctx, [(lv, A.SWZ_RGBA) for lv in levels], (6, 6), ref, A.PRF_LDR, A.PRE_MEDIUM)
        # round trip: the set decoder on the set's blocks gives the reference decoder's images
        back = [torch.zeros(lv.shape, dtype=torch.uint8, device="cuda") for lv in levels]
        assert product.decompress_images_device(ctx, list(zip(back, outs))) == A.SUCCESS
        torch.cuda.synchronize()
        for lv, o, b in zip(levels, outs, back):
            want = ref.decompress(o.cpu().numpy(), lv.shape[1], lv.shape[0], (6, 6))
            assert np.array_equal(b.cpu().numpy(), want), lv.shape
    finally:
        product.context_free(ctx)


def test_set_larger_than_a_chunk_progress_and_cancel(product, A):
    entries = [(_image(A, 1000, 1000, seed=1), A.SWZ_RGBA), (_image(A, 2048, 1100, seed=2), A.SWZ_RGBA),
               (_image(A, 1500, 1500, seed=3), (A.SWZ_G, A.SWZ_R, A.SWZ_B, A.SWZ_A))]
    counts = [_blocks((im.shape[1], im.shape[0]), (4, 4)) for im, _ in entries]
    assert sum(counts) > 1 << 18 and counts[0] + counts[1] < 1 << 18          # the first chunk ends inside entry 2
    seen = []
    cb = A.PROGRESS_CB(lambda p: seen.append(p))

    def with_progress(cfg):
        cfg.progress_callback = cb
    ctx, _ = _ctx(product, A, A.PRF_LDR, (4, 4), A.PRE_FASTEST, tweak=with_progress)
    set_reports = []
    try:
        _set_vs_single(product, A, ctx, entries, (4, 4), after_set=lambda: set_reports.extend(seen))
    finally:
        product.context_free(ctx)
    assert len(set_reports) == 2 and set_reports == sorted(set_reports) and set_reports[-1] == pytest.approx(100.0), set_reports

    # cancel from the progress callback: the set call returns what the single call returns, and stops early
    ctx_holder = {}

    def cancel_now(p):
        product.lib.astcenc_compress_cancel(ctx_holder["ctx"])
    cb2 = A.PROGRESS_CB(cancel_now)

    def with_cancel(cfg):
        cfg.progress_callback = cb2
    ctx, _ = _ctx(product, A, A.PRF_LDR, (4, 4), A.PRE_FASTEST, tweak=with_cancel)
    ctx_holder["ctx"] = ctx
    try:
        # three chunks each: the cancel from the first report (chunk 1 is queued by then) stops them before chunk 2
        big = _dev(_image(A, 3000, 3000, seed=9))
        n = _blocks((3000, 3000), (4, 4))
        e_single, out_single = _single(product, A, ctx, big, n, A.SWZ_RGBA)
        assert bool((out_single[-16:] == 0xAB).all())
        entries = [(_image(A, 2048, 2048, seed=5), A.SWZ_RGBA)] + entries + [(_image(A, 1100, 900, seed=6), A.SWZ_RGBA)]
        counts = [_blocks((im.shape[1], im.shape[0]), (4, 4)) for im, _ in entries]
        assert sum(counts) > 2 << 18
        imgs = [_dev(im) for im, _ in entries]
        outs = [torch.full((c * 16,), 0xAB, dtype=torch.uint8, device="cuda") for c in counts]
        e_set = product.compress_images_device(ctx, [(i, o, s) for i, o, (_, s) in zip(imgs, outs, entries)])
        torch.cuda.synchronize()
        assert e_set == e_single
        untouched = sum(int((o.cpu().numpy().reshape(-1, 16) == 0xAB).all(axis=1).sum()) for o in outs)
        assert untouched == sum(counts) - (2 << 18), "a cancel from the first progress report stops the set before its last chunk"
    finally:
        product.context_free(ctx)


def test_alpha_scale_per_entry(product, ref, A):
    def radius(cfg):
        cfg.a_scale_radius = 3
    ctx, _ = _ctx(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM, tweak=radius)
    try:
        entries = [(_image(A, 97, 64, kind="transparent", seed=1), A.SWZ_RGBA), (_image(A, 5, 3, kind="transparent"), A.SWZ_RGBA),
                   (_image(A, 300, 301, kind="transparent", seed=2), (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A)),
                   (_image(A, 64, 64, kind="f16", seed=3), A.SWZ_RGBA), (_image(A, 40, 30, 3, kind="transparent", seed=4), A.SWZ_RGBA)]
        _set_vs_single(product, A, ctx, entries, (6, 6), ref, A.PRF_LDR, A.PRE_MEDIUM, tweak=radius)
    finally:
        product.context_free(ctx)


def test_bad_entries_write_nothing(product, A):
    ctx, _ = _ctx(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        imgs = [_dev(_image(A, w, h, seed=i)) for i, (w, h) in enumerate([(64, 64), (30, 20), (100, 50)])]
        outs = [torch.full((_blocks((i.shape[1], i.shape[0]), (6, 6)) * 16,), 0xAB, dtype=torch.uint8, device="cuda") for i in imgs]

        def entries():
            return [A.image_set_entry(i, o) for i, o in zip(imgs, outs)]

        def single(e):
            return product.lib.astcenc_amd_compress_volume_device(ctx, e.image, e.dim_x, e.dim_y, e.dim_z, e.data_type, C.byref(e.swizzle),
                                                                  e.blocks, e.blocks_len, None, None)
        cases = {"null image": lambda e: setattr(e, "image", None), "null blocks": lambda e: setattr(e, "blocks", None),
                 "short blocks_len": lambda e: setattr(e, "blocks_len", e.blocks_len - 1),
                 "bad swizzle": lambda e: setattr(e, "swizzle", A.Swizzle(A.SWZ_R, A.SWZ_G, A.SWZ_Z, A.SWZ_A)),
                 "zero dimension": lambda e: setattr(e, "dim_y", 0)}
        for what, spoil in cases.items():
            ents = entries()
            spoil(ents[1])
            want = single(ents[1])
            assert want != A.SUCCESS, what
            logged.clear()
            assert product.compress_images_device(ctx, ents) == want, what
            torch.cuda.synchronize()
            for o in outs:
                assert bool((o == 0xAB).all()), what + ": an output was written"
            assert any("entry 1" in m for m in logged), (what, logged)
        # the argument rules with a context
        assert product.lib.astcenc_amd_compress_images_device(ctx, None, 0, None, None) == A.SUCCESS
        assert product.lib.astcenc_amd_compress_images_device(ctx, None, 2, None, None) == A.ERR_BAD_PARAM
        # more than 2^32 - 1 blocks in all: refused before any buffer is looked at (the pointers are never dereferenced)
        huge = [A.ImageSetEntry(0x1000, 0x2000, 1 << 40, 65535, 65535, 1, A.TYPE_U8, A.Swizzle(*A.SWZ_RGBA)) for _ in range(40)]
        assert _blocks((65535, 65535), (6, 6)) * 40 > 0xFFFFFFFF
        assert product.compress_images_device(ctx, huge) == A.ERR_BAD_PARAM
        for o in outs:
            assert bool((o == 0xAB).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
        product.context_free(ctx)


@pytest.mark.parametrize("profile", ["ldr", "hdr"])
def test_decompress_set_matches_single_calls(product, A, profile):
    prf = A.PRF_HDR if profile == "hdr" else A.PRF_LDR
    for block in ((6, 6), (4, 4, 4)) if profile == "ldr" else ((6, 6),):
        ctx, _ = _ctx(product, A, prf, block, A.PRE_FASTEST)
        try:
            dims = [(1, 1, 1), (5, 3, 1), (17, 700, 1), (255, 190, 1), (1000, 37, 1), (33, 17, 5)]
            kind = "hdr" if profile == "hdr" else "u8"
            srcs = [_dev(_image(A, w, h, d, kind=kind, seed=i)) for i, (w, h, d) in enumerate(dims)]
            blocks = [torch.zeros(_blocks(dm, block) * 16, dtype=torch.uint8, device="cuda") for dm in dims]
            assert product.compress_images_device(ctx, list(zip(srcs, blocks))) == A.SUCCESS
            out_types = [torch.uint8, torch.float16, torch.float32, torch.uint8, torch.float16, torch.uint8]
            swz = [A.SWZ_RGBA, (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A), (A.SWZ_R, A.SWZ_G, A.SWZ_Z, A.SWZ_1), A.SWZ_RGBA,
                   (A.SWZ_A, A.SWZ_0, A.SWZ_G, A.SWZ_R), (A.SWZ_R, A.SWZ_G, A.SWZ_Z, A.SWZ_A)]
            shape = [((d, h, w, 4) if d > 1 else (h, w, 4)) for w, h, d in dims]
            got = [torch.full(s, 7, dtype=t, device="cuda") for s, t in zip(shape, out_types)]
            assert product.decompress_images_device(ctx, [(g, b, s) for g, b, s in zip(got, blocks, swz)]) == A.SUCCESS
            torch.cuda.synchronize()
            for k, (g, b, s, (w, h, d)) in enumerate(zip(got, blocks, swz, dims)):
                want = torch.full_like(g, 7)
                e = A.image_set_entry(want, b, s)
                assert product.lib.astcenc_amd_decompress_image_device(ctx, e.blocks, e.blocks_len, e.image, w, h, d, e.data_type,
                                                                       C.byref(e.swizzle), None) == A.SUCCESS
                torch.cuda.synchronize()
                assert g.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (profile, block, k)
            # a bad entry: its error, nothing written
            ents = [A.image_set_entry(g, b, s) for g, b, s in zip(got, blocks, swz)]
            before = [g.clone() for g in got]
            ents[2].blocks_len -= 1
            assert product.decompress_images_device(ctx, ents) == A.ERR_OUT_OF_MEM
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(before, got))
        finally:
            product.context_free(ctx)
