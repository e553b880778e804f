# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_lod_grad_device on the GPU: the gradients of the level-of-detail sampler with respect to the coordinates and
the levels of detail, for upstream gradients in the forward call's format.

Every case is bit for bit against the numpy model of the header's comment (tests/sample_lod_grad_model.py) applied to what the
REFERENCE decoder writes for every whole level (the `ref` fixture) -- never to anything the library produced.  All three buffers
of a grid that the call writes or could write -- grad_coords, grad_lod and, because it must stay as it is, grad_out -- start
guard-filled or NaN-padded and are compared whole; padded and tight pitches alternate for grad_out, grad_coords, grad_lod, coords
and lod, and the padding of every input holds NaNs.  The chain is the full mip chain of the 17 x 17-block image (6x6: 102, 51, 25,
12, 6, 3, 1) of tests/test_decode_lod.py."""
import ctypes as C

import numpy as np
import pytest

import sample_lod_grad_model as G
import sample_lod_model as L
import sample_model as S
import tensor_model as M
from test_decode_regions import reference_decode
from test_decode_scaled import FOOTPRINTS, GUARD, NP_TYPES, dev, type_of
from test_decode_sample import MODES, FILTERS, contexts  # noqa: F401  (contexts: the fixture)
from test_decode_lod import MIPS, chains, entries_of, grid_message, log_names, make_chain, random_points, texels_of  # noqa: F401  (chains: the fixture)

pytestmark = pytest.mark.gpu

# (non-trivial and exact in binary32; the bias is not used by the call and must not matter)
SCALE = (0.75, -2.0, 1.0 / 255.0, 3.5)
BIAS = (5.0, -7.0, 0.25, 1e6)
SHAPES = [(64, 1), (13, 5), (33, 9), (1, 1)]
GUARD32 = np.frombuffer(bytes([GUARD]) * 4, dtype=np.uint32)[0]


def upstream_values(seed, shape, channels, ttype, special=False):
    """[shape[1], shape[0], channels] float32 values that the tensor type holds exactly; special: a NaN and an infinity among them."""
    rng = np.random.default_rng(seed)
    g = rng.normal(0.0, 2.0, size=(shape[1], shape[0], channels)).astype(np.float32)
    if ttype == M.F16:
        g = g.astype(np.float16).astype(np.float32)
    elif ttype == M.BF16:
        g = (g.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    if special and g.size >= 8:
        flat = g.reshape(-1)
        flat[1] = np.nan
        flat[flat.size // 2] = np.inf
        flat[flat.size - 2] = -np.inf
    return g


def upstream_bits(g, ttype):
    if ttype == M.F32:
        return g.view(np.uint32)
    if ttype == M.F16:
        return g.astype(np.float16).view(np.uint16)
    return (g.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


class Case:
    """The device buffers of one grid: coords, lod and grad_out (inputs, NaN in their padding), grad_coords and grad_lod
    (guard-filled), tight or with padded pitches."""

    def __init__(self, coords, lod, g, ttype, layout, want_lod=True, pad=0, front=64):
        import torch
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        oy, ox = coords.shape[:2]
        ch = g.shape[-1]
        self.coords, self.lod, self.g, self.out, self.want_lod, self.front = coords, lod, g, (ox, oy), want_lod, front
        self.ttype, self.layout, self.channels = ttype, layout, ch
        go_padded, gc_padded, gl_padded, c_padded, l_padded = (bool(pad & (1 << k)) for k in range(5))
        self.tight = dict(go=not go_padded, gc=not gc_padded, gl=not gl_padded, c=not c_padded, l=not l_padded)
        # grad_out, placed as the forward output; every other element a NaN of the type
        self.row = (ox if layout == M.PLANAR else ox * ch) + (3 if go_padded else 0)
        self.plane = self.row * oy + (5 if go_padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * ch if layout == M.PLANAR else self.row * oy
        held = np.full(elements, M.CANONICAL_NAN[ttype], dtype=M.BITS_DTYPE[ttype])
        M.scatter(held, 0, upstream_bits(g, ttype)[None], layout, 0, self.row, self.row * oy, self.plane)
        self.go_bits = held
        self.go = dev(held)
        held = np.full((oy, ox + (3 if c_padded else 0), 2), np.nan, dtype=np.float32)
        held[:, :ox] = coords
        self.cbuf, self.crow = dev(held), held.shape[1] * 2
        self.lbuf, self.lrow = None, 0
        if lod is not None:
            held = np.full((oy, ox + (5 if l_padded else 0)), np.nan, dtype=np.float32)
            held[:, :ox] = lod
            self.lbuf, self.lrow = dev(held), held.shape[1]
        self.gcrow = 2 * (ox + (2 if gc_padded else 0))
        self.glrow = ox + (7 if gl_padded else 0)
        self.gc = torch.full((front + self.gcrow * oy * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.gl = torch.full((front + self.glrow * oy * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda")

    def grid(self, A, first_entry, level_count, z, bias, zero_pitches=False):
        def pitch(v, key):
            return 0 if zero_pitches and self.tight[key] else v
        row, plane = (0, 0) if zero_pitches and self.tight["go"] else (self.row, self.plane)
        return A.LodGradGrid(first_entry, level_count, z, self.out[0], self.out[1], self.cbuf.data_ptr(), pitch(self.crow, "c"),
                             self.lbuf.data_ptr() if self.lbuf is not None else None, pitch(self.lrow, "l"), bias, self.go.data_ptr(), row, plane,
                             self.gc.data_ptr() + self.front, pitch(self.gcrow, "gc"), self.gl.data_ptr() + self.front if self.want_lod else None, pitch(self.glrow, "gl"))

    def want(self, chain, sampler, bias, scale):
        ox, oy = self.out
        a = G.upstream(self.g, scale)
        gc, gl = G.grad(chain, sampler[0], sampler[1], sampler[2], sampler[3], self.coords, self.lod, bias, a, self.want_lod)
        want_gc = np.full(self.gc.numel() // 4, GUARD32, dtype=np.uint32)
        rows = want_gc[self.front // 4: self.front // 4 + self.gcrow * oy].reshape(oy, self.gcrow)
        rows[:, :2 * ox] = gc.reshape(oy, 2 * ox).view(np.uint32)
        want_gl = np.full(self.gl.numel() // 4, GUARD32, dtype=np.uint32)
        if self.want_lod:
            rows = want_gl[self.front // 4: self.front // 4 + self.glrow * oy].reshape(oy, self.glrow)
            rows[:, :ox] = gl.view(np.uint32)
        return want_gc, want_gl

    def got(self):
        return self.gc.cpu().numpy().view(np.uint32), self.gl.cpu().numpy().view(np.uint32)


def run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, cases, turn=0, what="", special=False):
    """cases: [(first entry, levels, z, coords, lod or None, lod_bias, want_lod)], all in one call.  Returns the (grad_coords,
    grad_lod) bits of every grid."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32 = [float(v) for v in fmt.scale]
    held, grids = [], []
    for i, (first, count, z, coords, lod, bias, want_lod) in enumerate(cases):
        g = upstream_values(1000 * turn + i, (coords.shape[1], coords.shape[0]), channels, ttype, special=special)
        # (five pitches, tight or padded: a different subset for every grid and turn)
        c = Case(coords, lod, g, ttype, layout, want_lod=want_lod, pad=(5 * i + 3 * turn + 1) * 11 % 32)
        held.append(c)
        grids.append(c.grid(A, first, count, z, bias, zero_pitches=(i + turn) % 2 == 0))
    err = product.sample_lod_grad_device(ctx, entries, fmt, A.LodSampler(*sampler), grids)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    out = []
    for c, (first, count, z, coords, lod, bias, want_lod) in zip(held, cases):
        chain = [texels[first + l][z] for l in range(count)]
        (got_gc, got_gl), (want_gc, want_gl) = c.got(), c.want(chain, sampler, bias, scale32)
        for name, got, want in (("grad_coords", got_gc, want_gc), ("grad_lod", got_gl, want_gl)):
            if not np.array_equal(got, want):
                at = int(np.argwhere(got != want)[0][0])
                raise AssertionError("%s sampler %r format %r grid %dx%d of entries %d..%d: %s: first differing float at %d: got 0x%08x, want 0x%08x; %d differ" %
                                     (what, sampler, fmt_args, c.out[0], c.out[1], first, first + count - 1, name, at - c.front // 4, got[at], want[at], int((got != want).sum())))
        assert np.array_equal(c.go.cpu().numpy(), c.go_bits), "grad_out changed"
        out.append((got_gc, got_gl))
    return out


_SWIZZLED = {}


def swizzled(ref, A, source, tname, swz):
    """What the reference decodes `source` to under the HDR profile with the swizzle `swz`, once per module."""
    key = (id(source), tname, swz)
    if key not in _SWIZZLED:
        w, h = source.dims[:2]
        _SWIZZLED[key] = reference_decode(ref, A, source.data, (w, h, 1), source.block + (1,), A.PRF_HDR, NP_TYPES[tname], swz)
    return _SWIZZLED[key]


def shaped_cases(seed, n, first=0, z=0, bias=0.0, want_lod=True):
    return [(first, n, z) + random_points(seed + i, s, n) + (bias, want_lod) for i, s in enumerate(SHAPES)]


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_every_filter_mip_filter_and_address_mode(product, A, contexts, chains, name):
    """Grids of 64 x 1, 13 x 5, 33 x 9 and 1 x 1 of random (u, v) in [-0.25, 1.25] with lambda in [-1, L + 0.5]: both filters x both
    mip filters x the four address modes, mixed per axis; a U8 chain next to the same streams as F16 under the HDR profile (whose
    reserved-mode blocks are NaN)."""
    chain = chains(name)
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_HDR)
    entries = entries_of(chain, "u8") + entries_of(chain, "f16")
    texels = texels_of(chain, A.PRF_HDR, "u8") + texels_of(chain, A.PRF_HDR, "f16")
    for filt in FILTERS:
        for k, mode in enumerate(MODES):
            for mip in MIPS:
                ay = MODES[(k + 1 + mip) % 4]
                cases = shaped_cases(100 * filt + 10 * k + 2 * mip, n, first=((k + mip) % 2) * n)
                run_and_check(product, A, ctx, entries, texels, (filt, mode, ay, mip), (M.F32, M.PLANAR, 3), cases, turn=k + filt + 2 * mip, what=name)


def test_special_coordinates_and_levels_of_detail(product, A, contexts, chains):
    """special_coordinates() x special_lambdas(): texel centres, edges, integer and half lambdas, the top level and beyond,
    infinities, and every invalid point next to valid neighbours."""
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    su, sl = L.special_coordinates(), L.special_lambdas(n)
    grid = np.stack(np.meshgrid(su, su, indexing="xy"), axis=-1)
    for filt in FILTERS:
        for k, mode in enumerate(MODES):
            for mip in MIPS:
                lod = sl[(np.arange(grid.shape[0])[:, None] * 7 + np.arange(grid.shape[1])[None, :] + k) % len(sl)]
                run_and_check(product, A, ctx, entries, texels, (filt, mode, MODES[(k + 2) % 4], mip), (M.F32, M.INTERLEAVED, 4), [(0, n, 0, grid, lod, 0.0, True)],
                              turn=k + mip, what="special")


def test_texel_centres_read_the_right_hand_neighbour(product, A, contexts, chains):
    """Every texel centre of level 1 (51 x 51) at lambda' = 1: f = 0 on both axes, the forward call reads one texel a point and
    the gradient is the right-hand difference."""
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    w, h = chain[1].dims
    k = np.arange(0, 32, dtype=np.float64)
    uv = np.stack(np.meshgrid((k + 0.5) / w, (k[:9] * 5 + 0.5) / h, indexing="xy"), axis=-1).astype(np.float32)
    lod = np.full(uv.shape[:2], 1.0, dtype=np.float32)
    got = run_and_check(product, A, ctx, entries, texels, (S.BILINEAR, S.CLAMP, S.REPEAT, L.MIP_LINEAR), (M.F32, M.PLANAR, 4), [(0, n, 0, uv, lod, 0.0, True)], what="centres")
    assert (got[0][0][16:16 + 32 * 9 * 2] != 0).any()


@pytest.mark.parametrize("ttype,layout", [(t, l) for t in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED)])
def test_formats_sources_and_upstream_specials(product, ref, A, contexts, chains, ttype, layout):
    """Every tensor type with both layouts, channels 1 to 4, a non-trivial scale; a chain whose levels are U8, F16 and F32 in turn
    with swizzles that use constants; a NaN and the infinities in grad_out."""
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_HDR)
    names = [("u8", "f16", "f32")[l % 3] for l in range(n)]
    swizzles = [(A.SWZ_R, A.SWZ_G, A.SWZ_B, A.SWZ_A), (A.SWZ_B, A.SWZ_1, A.SWZ_R, A.SWZ_0), (A.SWZ_A, A.SWZ_A, A.SWZ_0, A.SWZ_G)]
    entries = [A.compressed_entry(s.blocks, s.dims, type_of(A, t), swizzles[l % 3]) for l, (s, t) in enumerate(zip(chain, names))]
    texels = [swizzled(ref, A, s, t, swizzles[l % 3]) for l, (s, t) in enumerate(zip(chain, names))]
    for channels in range(1, 5):
        for filt in FILTERS:
            mip = (channels + filt) % 2
            cases = shaped_cases(31 * channels + filt, n, bias=0.25 * channels)
            run_and_check(product, A, ctx, entries, texels, (filt, MODES[channels % 4], MODES[(channels + filt) % 4], mip), (ttype, layout, channels), cases,
                          turn=channels + filt, what="formats", special=(channels + filt) % 2 == 0)


def test_null_grad_lod_null_lod_and_two_chains_in_one_call(product, ref, A, contexts, chains):
    """Grids over the full chain, over its levels 2 .. 4 as a chain of their own, over another image's chain of two levels and over
    one level alone, in one call; grad_lod NULL among them, and lod NULL with a lod_bias that moves the points across a level."""
    chain = chains("6x6")
    n = len(chain)
    other = make_chain(product, ref, A, (6, 6), [(40, 30), (13, 50)], seed=60)
    ctx = contexts((6, 6), A.PRF_LDR)
    entries = entries_of(chain, "u8") + entries_of(other, "f32")
    texels = texels_of(chain, A.PRF_LDR, "u8") + texels_of(other, A.PRF_LDR, "f32")
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, n, 0) + random_points(1, (33, 9), n) + (0.0, False),
                     (2, 3, 0) + random_points(2, (13, 5), 3) + (0.5, True),
                     (n, 2, 0) + random_points(3, (64, 1), 2) + (0.0, True),
                     (n + 1, 1, 0) + random_points(4, (13, 5), 5) + (0.0, True),
                     (0, n, 0, random_points(5, (33, 9), n)[0], None, 1.625, True),
                     (0, n, 0, random_points(6, (13, 5), n)[0], None, 2.0, True),
                     (n, 2, 0, random_points(7, (1, 1), 2)[0], None, 0.5, False)]
            run_and_check(product, A, ctx, entries, texels, (filt, S.REPEAT, S.BORDER, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + 2 * mip, what="chains")


def test_autograd_function_is_the_two_calls(product, A, contexts, chains):
    """sample_lod(...) through torch.autograd.grad: the forward bitwise the lod call's, the gradients bitwise the direct call's."""
    import torch
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries = entries_of(chain, "u8")
    uv, lod = random_points(77, (33, 9), n)
    for layout, ttype, dtype in ((A.TENSOR_PLANAR, A.TENSOR_F32, torch.float32), (A.TENSOR_INTERLEAVED, A.TENSOR_F16, torch.float16)):
        fmt = A.tensor_format(ttype, layout, 3, SCALE, BIAS)
        sampler = (A.SAMPLE_BILINEAR, A.ADDRESS_REPEAT, A.ADDRESS_CLAMP, A.MIP_LINEAR)
        coords = dev(uv).requires_grad_(True)
        lods = dev(lod).requires_grad_(True)
        out = product.sample_lod(ctx, entries, fmt, sampler, 0, n, 0, coords, lods, lod_bias=0.25)
        assert out.dtype == dtype and tuple(out.shape) == ((3, 9, 33) if layout == A.TENSOR_PLANAR else (9, 33, 3))
        direct = torch.zeros_like(out)
        assert product.sample_lod_tensors_device(ctx, entries, fmt, sampler, [(0, n, 0, coords.detach(), lods.detach(), direct, 0.25)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(out.detach().view(torch.uint8), direct.view(torch.uint8))
        upstream = dev(upstream_values(5, (33, 9), 3, M.F32 if ttype == A.TENSOR_F32 else M.F16))
        upstream = (upstream.permute(2, 0, 1) if layout == A.TENSOR_PLANAR else upstream).to(dtype).contiguous()
        gc, gl = torch.autograd.grad(out, (coords, lods), upstream)
        want_gc, want_gl = torch.full_like(gc, 7.0), torch.full_like(gl, 7.0)
        assert product.sample_lod_grad_device(ctx, entries, fmt, sampler, [(0, n, 0, coords.detach(), lods.detach(), upstream, want_gc, want_gl, 0.25)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(gc.view(torch.int32), want_gc.view(torch.int32)) and torch.equal(gl.view(torch.int32), want_gl.view(torch.int32))
        assert bool((gc != 0).any()) and bool((gl != 0).any())
        # coordinates alone: no lod tensor, no gradient for it
        out = product.sample_lod(ctx, entries, fmt, sampler, 0, n, 0, coords, None, lod_bias=1.5)
        (only,) = torch.autograd.grad(out, (coords,), upstream)
        assert product.sample_lod_grad_device(ctx, entries, fmt, sampler, [(0, n, 0, coords.detach(), None, upstream, want_gc, None, 1.5)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(only.view(torch.int32), want_gc.view(torch.int32))


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, chains):
    """Every new error path: the error code, the message through the log callback ("grid i of n") and all guard bytes intact.
    (Not among the cases: a gradient buffer on another device than entry 0's blocks -- on one GPU there is no such pointer to
    give; the backend's map from a grid's five buffers to the ownership check runs on every successful call, with and without
    `lod` and `grad_lod`.)"""
    import torch
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((2, 2, 40 * 40 * 2 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        uv, lod = random_points(1, (40, 40), n)
        coords, lods = dev(uv), dev(lod)
        upstream = dev(np.ones((3, 40, 40), dtype=np.float16))
        cptr, lptr, uptr = coords.data_ptr(), lods.data_ptr(), upstream.data_ptr()
        gc0, gl0, gc1, gl1 = out[0, 0].data_ptr(), out[0, 1].data_ptr(), out[1, 0].data_ptr(), out[1, 1].data_ptr()
        good = [A.LodGradGrid(0, n, 0, 30, 20, cptr, 80, lptr, 40, 0.0, uptr, 40, 1600, gc0, 0, gl0, 0),
                A.LodGradGrid(2, 3, 0, 40, 40, cptr, 0, None, 0, 1.0, uptr, 0, 0, gc1, 80, None, 0)]

        def call(fmt, grids, sampler=A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, A.MIP_LINEAR)):
            en = entries_of(chain, "u8")
            arr = (A.ImageSetEntry * len(en))(*en)
            garr = (A.LodGradGrid * len(grids))(*grids)
            return product.lib.astcenc_amd_sample_lod_grad_device(ctx, arr, len(en), C.byref(fmt) if fmt is not None else None,
                                                                  C.byref(sampler) if sampler is not None else None, garr, len(grids), None)

        def grid(index, **change):
            g = [A.LodGradGrid.from_buffer_copy(x) for x in good]
            for k, v in change.items():
                setattr(g[index], k, v)
            return g

        fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, SCALE, BIAS)
        cases = [
            ("a null grad_out", grid(1, grad_out=None), A.ERR_BAD_CONTEXT, ("grid 1 of 2", "grad_out")),
            ("a null grad_coords", grid(0, grad_coords=None), A.ERR_BAD_CONTEXT, ("grid 0 of 2", "grad_coords")),
            ("a grad_coords not aligned to 8 bytes", grid(1, grad_coords=gc1 + 4), A.ERR_BAD_PARAM, ("grid 1 of 2", "grad_coords")),
            ("a grad_out not aligned to its element", grid(0, grad_out=uptr + 1), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_out")),
            ("a grad_lod not aligned to 4 bytes", grid(0, grad_lod=gl0 + 2), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_lod")),
            ("a grad_out row pitch below the tight one", grid(0, row_pitch=29), A.ERR_BAD_PARAM, ("grid 0 of 2", "row_pitch")),
            ("a grad_out plane pitch below the tight one", grid(0, plane_pitch=40 * 20 - 1), A.ERR_BAD_PARAM, ("grid 0 of 2", "plane_pitch")),
            ("a grad_coord_row_pitch below the tight one", grid(1, grad_coord_row_pitch=78), A.ERR_BAD_PARAM, ("grid 1 of 2", "grad_coord_row_pitch")),
            ("an odd grad_coord_row_pitch", grid(0, grad_coord_row_pitch=81), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_coord_row_pitch")),
            ("a grad_lod_row_pitch below the tight one", grid(0, grad_lod_row_pitch=29), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_lod_row_pitch")),
            # ... and what the lod call checks is checked here, with its codes
            ("null coordinates", grid(1, coords=None), A.ERR_BAD_CONTEXT, (grid_message(1, 2, "coords is null"),)),
            ("33 levels", grid(0, level_count=33), A.ERR_BAD_PARAM, ("grid 0 of 2",)),
            ("a NaN lod_bias", grid(1, lod_bias=float("nan")), A.ERR_BAD_PARAM, ("grid 1 of 2", "lod_bias")),
        ]
        for what, grids, code, named in cases:
            del logged[:]
            assert call(fmt, grids) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(all(log_names(w, m) for w in named) for m in logged), (what, logged)
        del logged[:]
        assert call(fmt, good, sampler=None) == A.ERR_BAD_PARAM and any("sampler" in m for m in logged)
        assert call(None, good) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        # the good call is good, writes the gradients it was asked for and nothing else
        assert call(fmt, good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[0, 0, :64] == GUARD).all()) and not bool((out[0, 1, :64] == GUARD).all()) and not bool((out[1, 0, :64] == GUARD).all())
        assert bool((out[1, 1] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
