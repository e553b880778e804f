# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_volume_grad_device on the GPU: the gradients of the volume sampler with respect to the coordinates and the
levels of detail, for upstream gradients in the forward call's format.

Every case is bit for bit against the numpy model of the header's comment (tests/sample_volume_grad_model.py) applied to what the
REFERENCE decoder writes for every whole level (the `ref` fixture) -- never to anything the library produced.  All three buffers
of a grid that the call writes or could write -- grad_coords, grad_lod and, because it must stay as it is, grad_out -- start
guard-filled or NaN-padded and are compared whole; padded and tight pitches alternate for grad_out, grad_coords, grad_lod, coords
and lod, and the padding of every input holds NaNs.  The chains, the footprints and the grids are those of
tests/test_decode_volume.py (its builders, imported): five levels from 20 x 14 x 9 down to 1 x 1 x 1, the footprints 4x4, 6x6 and
8x5 over slices and 3x3x3, 4x4x3, 5x5x4 and 6x6x6, grids of 70 x 1, 33 x 3 and 19 x 11 points in one call.

Library.sample_volume_grad has no row in tests/test_stream_order.py (it takes no stream argument: see its docstring); its
ordering under torch's default stream and under a side stream is tested at the end of this file with that module's helpers."""
import ctypes as C
import time

import numpy as np
import pytest

import sample_lod_model as L
import sample_model as S
import sample_volume_grad_model as G
import sample_volume_model as K
import tensor_model as M
import test_stream_order as SO
from test_decode_regions import reference_decode
from test_decode_scaled import GUARD, dev, type_of
from test_decode_sample import contexts  # noqa: F401  (contexts: the fixture)
from test_decode_lod import grid_message, log_names
from test_decode_lod_grad import GUARD32, SCALE, BIAS, upstream_bits, upstream_values
from test_decode_volume import FOOTPRINTS, FILTERS, MIPS, chains, entries_of, make_volume_chain, pow2, texels_of  # noqa: F401  (chains, pow2: the fixtures)

pytestmark = pytest.mark.gpu

MODES = (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER)
FORMATS = [(M.F16, M.PLANAR, 3), (M.F32, M.INTERLEAVED, 4), (M.BF16, M.PLANAR, 1), (M.F32, M.PLANAR, 2), (M.F16, M.INTERLEAVED, 4), (M.BF16, M.INTERLEAVED, 3)]


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
        held = np.full((oy, 3 * ox + (5 if c_padded else 0)), np.nan, dtype=np.float32)
        held[:, :3 * ox] = coords.reshape(oy, 3 * ox)
        self.cbuf, self.crow = dev(held), held.shape[1]
        self.lbuf, self.lrow = None, 0
        if lod is not None:
            held = np.full((oy, ox + (5 if l_padded else 0)), np.nan, dtype=np.float32)
            held[:, :ox] = lod
            self.lbuf, self.lrow = dev(held), held.shape[1]
        # (an odd padding: the pitch of triples need not be even; and grad_coords starts 4 bytes past an 8-byte boundary)
        self.gcrow = 3 * ox + (1 if gc_padded else 0)
        self.glrow = ox + (7 if gl_padded else 0)
        self.gc_front = front + 4
        self.gc = torch.full((self.gc_front + self.gcrow * oy * 4 + 60,), GUARD, dtype=torch.uint8, device="cuda")
        self.gl = torch.full((front + self.glrow * oy * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda")

    def grid(self, A, first_entry, level_count, bias, zero_pitches=False):
        def pitch(v, key):
            return 0 if zero_pitches and self.tight[key] else v
        row, plane = (0, 0) if zero_pitches and self.tight["go"] else (self.row, self.plane)
        return A.VolumeGradGrid(first_entry, level_count, self.out[0], self.out[1], self.cbuf.data_ptr(), pitch(self.crow, "c"),
                                self.lbuf.data_ptr() if self.lbuf is not None else None, pitch(self.lrow, "l"), bias, self.go.data_ptr(), row, plane,
                                self.gc.data_ptr() + self.gc_front, pitch(self.gcrow, "gc"), self.gl.data_ptr() + self.front if self.want_lod else None, pitch(self.glrow, "gl"))

    def model(self, chain, sampler, bias, scale):
        return G.grad(chain, sampler[0], sampler[1:4], sampler[4], self.coords, self.lod, bias, G.upstream(self.g, scale), self.want_lod)

    def want(self, chain, sampler, bias, scale):
        ox, oy = self.out
        gc, gl = self.model(chain, sampler, bias, scale)
        want_gc = np.full(self.gc.numel() // 4, GUARD32, dtype=np.uint32)
        rows = want_gc[self.gc_front // 4: self.gc_front // 4 + self.gcrow * oy].reshape(oy, self.gcrow)
        rows[:, :3 * ox] = gc.reshape(oy, 3 * ox).view(np.uint32)
        want_gl = np.full(self.gl.numel() // 4, GUARD32, dtype=np.uint32)
        if self.want_lod:
            rows = want_gl[self.front // 4: self.front // 4 + self.glrow * oy].reshape(oy, self.glrow)
            rows[:, :ox] = gl.view(np.uint32)
        return want_gc, want_gl

    def got(self):
        return self.gc.cpu().numpy().view(np.uint32), self.gl.cpu().numpy().view(np.uint32)

    def triples(self):
        """grad_coords [H, W, 3] as uint32, without the guards and the padding."""
        ox, oy = self.out
        flat = self.got()[0][self.gc_front // 4: self.gc_front // 4 + self.gcrow * oy]
        return flat.reshape(oy, self.gcrow)[:, :3 * ox].reshape(oy, ox, 3)

    def lods(self):
        ox, oy = self.out
        return self.got()[1][self.front // 4: self.front // 4 + self.glrow * oy].reshape(oy, self.glrow)[:, :ox]


def run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, cases, turn=0, what="", special=False):
    """sampler: (filter, address_x, address_y, address_z, mip_filter); cases: [(first entry, levels, coords [H, W, 3], lod [H, W] or
    None, lod_bias, want_lod)], all in one call.  Returns the Cases."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32 = [float(v) for v in fmt.scale]
    held, grids = [], []
    for i, (first, count, coords, lod, bias, want_lod) in enumerate(cases):
        g = upstream_values(1000 * turn + i, (coords.shape[1], coords.shape[0]), channels, ttype, special=special)
        # (five pitches, tight or padded: a different subset for every grid and turn)
        c = Case(coords, lod, g, ttype, layout, want_lod=want_lod, pad=(5 * i + 3 * turn + 1) * 11 % 32)
        held.append(c)
        grids.append(c.grid(A, first, count, bias, zero_pitches=(i + turn) % 2 == 0))
    err = product.sample_volume_grad(ctx, entries, fmt, A.VolumeSampler(*sampler), grids)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    for c, (first, count, coords, lod, bias, want_lod) in zip(held, cases):
        chain = [texels[first + l] for l in range(count)]
        (got_gc, got_gl), (want_gc, want_gl) = c.got(), c.want(chain, sampler, bias, scale32)
        for name, got, want, front in (("grad_coords", got_gc, want_gc, c.gc_front), ("grad_lod", got_gl, want_gl, c.front)):
            if not np.array_equal(got, want):
                at = int(np.argwhere(got != want)[0][0])
                raise AssertionError("%s sampler %r format %r grid %dx%d of entries %d..%d: %s: first differing float at %d: got 0x%08x, want 0x%08x; %d differ" %
                                     (what, sampler, fmt_args, c.out[0], c.out[1], first, first + count - 1, name, at - front // 4, got[at], want[at], int((got != want).sum())))
        assert np.array_equal(c.go.cpu().numpy(), c.go_bits), "grad_out changed"
    return held


def turning(turn):
    """Three address modes that turn through every mode on every axis as `turn` counts."""
    return (MODES[turn % 4], MODES[(3 * turn + 1) % 4], MODES[(turn + 2) % 4])


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_generated_grids(product, A, contexts, chains, name):
    """The three grid shapes in one call -- a partial tile of each tile shape, the points whose second tap has weight zero on each
    axis, a point whose eight taps lie in eight blocks of a 3D footprint, coordinates at +-2^14, beyond and non-finite, lambdas at
    integers, clamped, NaN and +-inf (sample_volume_model.grid_inputs) -- under both filters and both mip filters, the address
    modes turning so that every axis has every mode, grad_lod wanted and not, a NaN and the infinities in grad_out."""
    footprint = FOOTPRINTS[name]
    chain = chains(name)
    n = len(chain)
    ctx = contexts(footprint, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    assert [t.shape[:3][::-1] for t in texels] == K.CHAIN
    inputs = [K.grid_inputs(k, ox, oy, footprint) for k, (ox, oy) in enumerate(K.GRIDS)]
    seen = [set(), set(), set()]
    moved = False
    for filt in FILTERS:
        for mip in MIPS:
            turn = 2 * filt + mip
            address = turning(turn)
            for axis in range(3):
                seen[axis].add(address[axis])
            cases = [(0, n, coords, lod, 0.25 * k, (k + turn) % 3 != 0) for k, (coords, lod) in enumerate(inputs)]
            held = run_and_check(product, A, ctx, entries, texels, (filt,) + address + (mip,), FORMATS[turn], cases, turn=turn, what=name + " generated", special=turn % 2 == 1)
            moved = moved or (filt == S.BILINEAR and any(c.triples()[..., 2].any() for c in held))
    assert all(s == {0, 1, 2, 3} for s in seen), seen
    assert moved, "no gradient along w anywhere"


def test_special_points_and_texel_centres(product, A, contexts, chains):
    """The special coordinates of the lod tests on two axes at once with the third turning through them, against the special
    lambdas; then every texel centre of level 1 on all three axes and on each axis alone, at lambda' = 1: the forward call has
    one tap on that axis and the gradient along it is the right-hand difference."""
    name = "4x4x3"
    chain = chains(name)
    n = len(chain)
    ctx = contexts(FOOTPRINTS[name], A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    su, sl = L.special_coordinates(), L.special_lambdas(n)
    m = len(su)
    grid = np.empty((m, m, 3), dtype=np.float32)
    w, h, d = K.CHAIN[1]
    centres = K.texel_centres(texels[1])                                     # [D * H, W, 3]
    rng = np.random.default_rng(9)
    for k in range(3):
        grid[..., k], grid[..., (k + 1) % 3] = su[None, :], su[:, None]
        grid[..., (k + 2) % 3] = su[(np.arange(m)[:, None] * 3 + np.arange(m)[None, :] * 5 + k) % m]
        lod = sl[(np.arange(m)[:, None] * 7 + np.arange(m)[None, :] + k) % len(sl)]
        alone = rng.uniform(-0.1, 1.1, size=centres.shape).astype(np.float32)
        alone[..., k] = centres[..., k]
        ones = np.full(centres.shape[:2], 1.0, dtype=np.float32)
        cases = [(0, n, grid.copy(), lod, 0.0, True), (0, n, alone, ones, 0.0, True)] + ([(0, n, centres, ones, 0.0, True)] if k == 0 else [])
        for filt in FILTERS:
            for mip in MIPS:
                held = run_and_check(product, A, ctx, entries, texels, (filt,) + turning(k + 2 * mip) + (mip,), FORMATS[(k + filt) % 6], cases, turn=k + mip, what="special",
                                     special=mip == 1)
                if filt == S.BILINEAR:
                    assert held[1].triples()[..., k].any(), "no right-hand difference along axis %d" % k


@pytest.mark.parametrize("ttype,layout", [(t, l) for t in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED)])
def test_formats_sources_and_profiles(product, ref, A, contexts, chains, ttype, layout):
    """Every tensor type with both layouts, channels 1 to 4, a non-trivial scale, a bias that must not matter; a chain whose levels
    are U8, F16 and F32 in turn; the four profiles (under HDR the reserved-mode block of an F16 level is NaN); a NaN and the
    infinities in grad_out; then a BGRA swizzle on every level."""
    name = ("6x6", "3x3x3", "8x5", "5x5x4", "4x4", "6x6x6")[2 * ttype + layout]
    footprint = FOOTPRINTS[name]
    chain = chains(name)
    n = len(chain)
    names = [("u8", "f16", "f32")[l % 3] for l in range(n)]
    entries = [s.entry(t) for s, t in zip(chain, names)]
    for channels, profile in zip(range(1, 5), (A.PRF_LDR, A.PRF_LDR_SRGB, A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)):
        ctx = contexts(footprint, profile)
        texels = [s.texels(profile, t) for s, t in zip(chain, names)]
        filt, mip = channels % 2, (channels // 2) % 2
        cases = [(0, n) + K.grid_inputs(20 + channels, ox, oy, footprint) + (0.25 * channels, i == 0) for i, (ox, oy) in enumerate(K.GRIDS[1:])]
        run_and_check(product, A, ctx, entries, texels, (filt,) + turning(channels + ttype) + (mip,), (ttype, layout, channels), cases, turn=channels, what="formats " + name,
                      special=channels % 2 == 0)
    ctx = contexts(footprint, A.PRF_LDR)
    swz = (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A)
    entries = [A.compressed_entry(s.blocks, s.dims, type_of(A, "u8"), swz) for s in chain]
    texels = [reference_decode(ref, A, s.data, s.dims, footprint, A.PRF_LDR, np.uint8, swz) for s in chain]
    cases = [(0, n) + K.grid_inputs(40, 19, 11, footprint) + (0.0, True)]
    run_and_check(product, A, ctx, entries, texels, (S.BILINEAR, S.MIRROR, S.BORDER, S.CLAMP, L.MIP_LINEAR), (ttype, layout, 3), cases, what="swizzle " + name)


def test_null_grad_lod_null_lod_and_two_chains_in_one_call(product, A, contexts, chains, pow2):
    """Grids over the full chain, over its levels 1 .. 3 as a chain of their own, over another volume's chain and over one level
    alone, in one call; grad_lod NULL among them, and lod NULL with a lod_bias that moves the points across a level."""
    a, b = chains("3x3x3"), pow2("3x3x3")
    ctx = contexts((3, 3, 3), A.PRF_LDR)
    entries = entries_of(a, "u8") + entries_of(b, "f16")
    texels = texels_of(a, A.PRF_LDR, "u8") + texels_of(b, A.PRF_LDR, "f16")
    na, fp = len(a), (3, 3, 3)
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, na) + K.grid_inputs(50, 33, 3, fp) + (0.0, False),
                     (na, 3) + K.grid_inputs(51, 19, 11, fp, levels=3) + (0.5, True),
                     (1, 3) + K.grid_inputs(52, 70, 1, fp, levels=3) + (-0.25, True),
                     (na + 2, 1) + K.grid_inputs(53, 19, 11, fp, levels=1) + (0.0, True),
                     (0, na, K.grid_inputs(54, 33, 3, fp)[0], None, 1.625, True),
                     (0, na, K.grid_inputs(55, 19, 11, fp)[0], None, 2.0, True),
                     (na, 3, K.grid_inputs(56, 70, 1, fp)[0], None, 0.5, False)]
            run_and_check(product, A, ctx, entries, texels, (filt, S.REPEAT, S.BORDER, S.MIRROR, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + 2 * mip, what="chains")


def test_one_z_tap_is_the_lod_gradient_call_byte_for_byte(product, ref, A, contexts):
    """A 2D-footprint context and a chain whose levels all have four slices: at w = (kz + 0.5) / 4 every point has one z tap, of
    slice kz, in every level; du, dv and grad_lod are the bytes astcenc_amd_sample_lod_grad_device writes for z = kz."""
    import torch
    block = (6, 6, 1)
    chain = make_volume_chain(product, ref, A, block, [(20, 14, 4), (10, 7, 4), (5, 3, 4)], 120)
    ctx = contexts(block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    rng = np.random.default_rng(3)
    fmt_args = (M.F32, M.PLANAR, 3)
    fmt = A.tensor_format(*fmt_args, SCALE, BIAS)
    for turn, (ox, oy) in enumerate(K.GRIDS):
        kz = turn + 1
        uv = rng.uniform(-0.25, 1.25, size=(oy, ox, 2)).astype(np.float32)
        lod = K.seeded_lods(rng, (oy, ox), 3)
        coords = np.concatenate([uv, np.full((oy, ox, 1), (kz + 0.5) / 4, dtype=np.float32)], axis=-1)
        for filt in FILTERS:
            ax, ay, az = turning(turn + filt)
            sampler = (filt, ax, ay, az, L.MIP_LINEAR)
            (c,) = run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, [(0, 3, coords, lod, 0.25, True)], turn=turn, what="one z tap")
            gc = torch.full((oy, ox, 2), 7.0, dtype=torch.float32, device="cuda")
            gl = torch.full((oy, ox), 7.0, dtype=torch.float32, device="cuda")
            upstream = dev(np.ascontiguousarray(np.moveaxis(c.g, -1, 0)))
            err = product.sample_lod_grad_device(ctx, entries, fmt, (filt, ax, ay, L.MIP_LINEAR), [(0, 3, kz, dev(uv), dev(lod), upstream, gc, gl, 0.25)])
            assert err == A.SUCCESS, product.error_string(err)
            torch.cuda.synchronize()
            assert np.array_equal(c.triples()[..., :2], gc.cpu().numpy().view(np.uint32)), (turn, filt)
            assert np.array_equal(c.lods(), gl.cpu().numpy().view(np.uint32)), (turn, filt)
            assert gc.cpu().numpy().any() == (filt == S.BILINEAR) and gl.cpu().numpy().any()


def test_autograd_function_is_the_two_calls(product, A, contexts, chains):
    """sample_volume(...) through torch.autograd.grad: the forward bitwise the volume call's, the gradients bitwise the direct
    call's; gradients for `coords` and `lod` only."""
    import torch
    name = "4x4x3"
    chain = chains(name)
    n = len(chain)
    ctx = contexts(FOOTPRINTS[name], A.PRF_LDR)
    entries = entries_of(chain, "u8")
    uvw, lod = K.grid_inputs(77, 33, 3, FOOTPRINTS[name])
    for layout, ttype, dtype in ((A.TENSOR_PLANAR, A.TENSOR_F32, torch.float32), (A.TENSOR_INTERLEAVED, A.TENSOR_F16, torch.float16)):
        fmt = A.tensor_format(ttype, layout, 3, SCALE, BIAS)
        sampler = (A.SAMPLE_BILINEAR, A.ADDRESS_REPEAT, A.ADDRESS_CLAMP, A.ADDRESS_MIRROR, A.MIP_LINEAR)
        coords = dev(uvw).requires_grad_(True)
        lods = dev(lod).requires_grad_(True)
        out = product.sample_volume(ctx, entries, fmt, sampler, 0, n, coords, lods, lod_bias=0.25)
        assert out.dtype == dtype and tuple(out.shape) == ((3, 3, 33) if layout == A.TENSOR_PLANAR else (3, 33, 3))
        direct = torch.zeros_like(out)
        assert product.sample_volume_tensors_device(ctx, entries, fmt, sampler, [(0, n, coords.detach(), lods.detach(), direct, 0.25)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(out.detach().view(torch.uint8), direct.view(torch.uint8))
        upstream = dev(upstream_values(5, (33, 3), 3, M.F32 if ttype == A.TENSOR_F32 else M.F16))
        upstream = (upstream.permute(2, 0, 1) if layout == A.TENSOR_PLANAR else upstream).to(dtype).contiguous()
        gc, gl = torch.autograd.grad(out, (coords, lods), upstream)
        assert tuple(gc.shape) == (3, 33, 3) and gc.dtype == torch.float32 and tuple(gl.shape) == (3, 33)
        want_gc, want_gl = torch.full_like(gc, 7.0), torch.full_like(gl, 7.0)
        assert product.sample_volume_grad(ctx, entries, fmt, sampler, [(0, n, coords.detach(), lods.detach(), upstream, want_gc, want_gl, 0.25)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(gc.view(torch.int32), want_gc.view(torch.int32)) and torch.equal(gl.view(torch.int32), want_gl.view(torch.int32))
        assert bool((gc != 0).any()) and bool((gl != 0).any())
        # coordinates alone: no lod tensor, no gradient for it
        out = product.sample_volume(ctx, entries, fmt, sampler, 0, n, coords, None, lod_bias=1.5)
        (only,) = torch.autograd.grad(out, (coords,), upstream)
        assert product.sample_volume_grad(ctx, entries, fmt, sampler, [(0, n, coords.detach(), None, upstream, want_gc, None, 1.5)]) == A.SUCCESS
        torch.cuda.synchronize()
        assert torch.equal(only.view(torch.int32), want_gc.view(torch.int32))
        # (autograd checks that backward returns one value per input of forward: the eight that are no tensors got None)
        out = product.sample_volume(ctx, entries, fmt, sampler, 0, n, coords, lods)
        out.float().sum().backward()
        assert coords.grad is not None and lods.grad is not None and tuple(coords.grad.shape) == (3, 33, 3)


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, chains):
    """Every new error path: the error code, the message through the log callback ("grid i of n") and all guard bytes intact.
    (Not among the cases: a gradient buffer on another device than entry 0's blocks -- on one GPU there is no such pointer to
    give; the backend's map from a grid's five buffers to the ownership check runs on every successful call, with and without
    `lod` and `grad_lod`.)"""
    import torch
    name = "3x3x3"
    chain = chains(name)
    n = len(chain)
    ctx = contexts(FOOTPRINTS[name], A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((2, 2, 41 * 40 * 3 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        rng = np.random.default_rng(1)
        coords = dev(rng.uniform(-0.25, 1.25, size=(40, 40, 3)).astype(np.float32))
        lods = dev(rng.uniform(-1.0, n + 0.5, size=(40, 40)).astype(np.float32))
        upstream = dev(np.ones((3, 40, 40), dtype=np.float16))
        cptr, lptr, uptr = coords.data_ptr(), lods.data_ptr(), upstream.data_ptr()
        gc0, gl0, gc1, gl1 = out[0, 0].data_ptr(), out[0, 1].data_ptr(), out[1, 0].data_ptr(), out[1, 1].data_ptr()
        # (grid 1: grad_coords 4 bytes past an 8-byte boundary and an odd pitch are legal here)
        good = [A.VolumeGradGrid(0, n, 30, 20, cptr, 120, lptr, 40, 0.0, uptr, 40, 1600, gc0, 0, gl0, 0),
                A.VolumeGradGrid(1, 3, 40, 40, cptr, 0, None, 0, 1.0, uptr, 0, 0, gc1 + 4, 121, None, 0)]

        def call(fmt, grids, sampler=A.VolumeSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, A.ADDRESS_BORDER, A.MIP_LINEAR)):
            en = entries_of(chain, "u8")
            arr = (A.ImageSetEntry * len(en))(*en)
            garr = (A.VolumeGradGrid * len(grids))(*grids)
            return product.lib.astcenc_amd_sample_volume_grad_device(ctx, arr, len(en), C.byref(fmt) if fmt is not None else None,
                                                                     C.byref(sampler) if sampler is not None else None, garr, len(grids), None)

        def grid(index, **change):
            g = [A.VolumeGradGrid.from_buffer_copy(x) for x in good]
            for k, v in change.items():
                setattr(g[index], k, v)
            return g

        fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, SCALE, BIAS)
        cases = [
            ("a null grad_out", grid(1, grad_out=None), A.ERR_BAD_CONTEXT, ("grid 1 of 2", "grad_out")),
            ("a null grad_coords", grid(0, grad_coords=None), A.ERR_BAD_CONTEXT, ("grid 0 of 2", "grad_coords")),
            ("a grad_coords not aligned to 4 bytes", grid(1, grad_coords=gc1 + 2), A.ERR_BAD_PARAM, ("grid 1 of 2", "grad_coords")),
            ("a grad_out not aligned to its element", grid(0, grad_out=uptr + 1), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_out")),
            ("a grad_lod not aligned to 4 bytes", grid(0, grad_lod=gl0 + 2), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_lod")),
            ("a grad_out row pitch below the tight one", grid(0, row_pitch=29), A.ERR_BAD_PARAM, ("grid 0 of 2", "row_pitch")),
            ("a grad_out plane pitch below the tight one", grid(0, plane_pitch=40 * 20 - 1), A.ERR_BAD_PARAM, ("grid 0 of 2", "plane_pitch")),
            ("a grad_coord_row_pitch below the tight one", grid(1, grad_coord_row_pitch=119), A.ERR_BAD_PARAM, ("grid 1 of 2", "grad_coord_row_pitch")),
            ("a grad_lod_row_pitch below the tight one", grid(0, grad_lod_row_pitch=29), A.ERR_BAD_PARAM, ("grid 0 of 2", "grad_lod_row_pitch")),
            # ... and what the volume call checks is checked here, with its codes
            ("null coordinates", grid(1, coords=None), A.ERR_BAD_CONTEXT, (grid_message(1, 2, "coords is null"),)),
            ("coordinates not aligned to 4 bytes", grid(0, coords=cptr + 2), A.ERR_BAD_PARAM, ("grid 0 of 2", "coords")),
            ("a coord_row_pitch below the tight one", grid(0, coord_row_pitch=89), A.ERR_BAD_PARAM, ("grid 0 of 2", "coord_row_pitch")),
            ("33 levels", grid(0, level_count=33), A.ERR_BAD_PARAM, ("grid 0 of 2",)),
            ("levels beyond the entries", grid(1, first_entry=n - 1), A.ERR_BAD_PARAM, ("grid 1 of 2",)),
            ("no points", grid(1, out_x=0), A.ERR_BAD_PARAM, ("grid 1 of 2",)),
            ("a NaN lod_bias", grid(1, lod_bias=float("nan")), A.ERR_BAD_PARAM, ("grid 1 of 2", "lod_bias")),
            ("a lod_row_pitch below the tight one", grid(0, lod_row_pitch=29), A.ERR_BAD_PARAM, ("grid 0 of 2", "lod_row_pitch")),
        ]
        for what, grids, code, named in cases:
            del logged[:]
            assert call(fmt, grids) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(all(log_names(w, m) for w in named) for m in logged), (what, logged)
        del logged[:]
        assert call(fmt, good, sampler=None) == A.ERR_BAD_PARAM and any("sampler" in m for m in logged)
        del logged[:]
        bad_z = A.VolumeSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, 7, A.MIP_LINEAR)
        assert call(fmt, good, sampler=bad_z) == A.ERR_BAD_PARAM and any("along z" in m for m in logged)
        assert call(None, good) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        # the good call is good, writes the gradients it was asked for and nothing else
        assert call(fmt, good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[0, 0, :64] == GUARD).all()) and not bool((out[0, 1, :64] == GUARD).all()) and not bool((out[1, 0, 4:68] == GUARD).all())
        assert bool((out[1, 0, :4] == GUARD).all()) and bool((out[1, 1] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)


# ---- ordering: the method has no stream argument, so modes (a) and (b) of tests/test_stream_order.py are the ones it has ----

VOLUME_SAMPLER = (1, 1, 0, 2, 1)      # bilinear, repeat, clamp, mirror, linear between levels
ORDER_MODES = ("a", "b")
ORDER_INPUTS = ("blocks", "coords", "lod", "grad_out")
_ORDER_ROWS = {}


def order_row(product, A, twin):
    """tests/test_stream_order.py's row for sample_volume_grad, over its World's compressed volume chain."""
    import torch
    if twin not in _ORDER_ROWS:
        w = SO.world(product, A, twin)
        blocks, coords, lod = w.blocks(w.chain_volume), w.points(3, -0.25, 1.25), w.lods()
        grad_out = SO.Buf(*[np.random.default_rng(s).normal(0.0, 2.0, size=(3, SO.GRID[1], SO.GRID[0])).astype(np.float32) for s in (41, 42)])
        grad_coords, grad_lod = w.out((SO.GRID[1], SO.GRID[0], 3), torch.float32), w.out((SO.GRID[1], SO.GRID[0]), torch.float32)
        entries, held = w.entries(w.chain_volume, blocks)

        def call(stream, held=held):
            assert stream is None
            SO.ok(w, w.product.sample_volume_grad(w.dec3, entries, w.fmt(), VOLUME_SAMPLER, [(0, SO.LEVELS, coords.t, lod.t, grad_out.t, grad_coords, grad_lod, 0.25)]))
            return []
        row = SO.Row({"blocks": blocks, "coords": coords, "lod": lod, "grad_out": grad_out}, [grad_coords, grad_lod], call)
        assert tuple(row.inputs) == ORDER_INPUTS
        _ORDER_ROWS[twin] = row
    return SO.world(product, A, twin), _ORDER_ROWS[twin]


@pytest.mark.parametrize("mode", ORDER_MODES)
@pytest.mark.parametrize("which", ORDER_INPUTS)
def test_inputs_arrive_in_time(product, A, which, mode):
    import torch
    for twin in range(SO.TWINS):
        w, row = order_row(product, A, twin)
        want_a, want_b = row.synchronised(), row.synchronised(which)
        assert want_a != want_b, "the call gives the same on both contents of %s: the case proves nothing" % which
        row.reset()
        buf = row.inputs[which]

        def queue():
            torch.cuda._sleep(SO.SLEEP)
            buf.put("B")
        extra, prefix_ms = SO.in_mode(w, mode, queue, row.call)
        got = row.results(extra)
        SO.check_delay("sample_volume_grad", prefix_ms, row.wall_ms)
        assert got != want_a, "the call read %s before the copy queued ahead of it had landed (contexts %d)" % (which, twin)
        assert got == want_b, "neither the old nor the new content of %s (contexts %d)" % (which, twin)


@pytest.mark.parametrize("mode", ORDER_MODES)
def test_outputs_are_not_overwritten(product, A, mode):
    import torch
    for twin in range(SO.TWINS):
        w, row = order_row(product, A, twin)
        want = row.synchronised()
        row.reset(fill=False)
        filled = [bytes([SO.GUARD]) * (o.numel() * o.element_size()) for o in row.outputs]
        assert all(g != f for g, f in zip(want, filled)), "an output the call does not write"

        def queue():
            torch.cuda._sleep(SO.SLEEP)
            row.fill()
        extra, prefix_ms = SO.in_mode(w, mode, queue, row.call)
        got = row.results(extra)
        SO.check_delay("sample_volume_grad", prefix_ms, row.wall_ms)
        assert all(g != f for g, f in zip(got, filled)), "the guard fill queued ahead of the call landed over what it wrote (contexts %d)" % twin
        assert got == want, twin


def test_complete_on_return(product, A):
    """Under torch's default stream the hip_stream is NULL: what the call wrote is there for a stream that waits for nothing."""
    import torch
    for twin in range(SO.TWINS):
        _, row = order_row(product, A, twin)
        want = row.synchronised()
        row.reset()
        row.call(None)
        fresh = torch.cuda.Stream()
        with torch.cuda.stream(fresh):
            held = [torch.empty(r.shape, dtype=r.dtype).pin_memory().copy_(r, non_blocking=True) for r in row.outputs]
        fresh.synchronize()
        assert [SO.bits(h) for h in held] == want, twin


def test_autograd_function_under_the_default_stream(product, A):
    """sample_volume and its backward read what torch kernels queued behind sleeps are still to write."""
    import torch
    shape = (SO.GRID[1], SO.GRID[0])
    for twin in range(SO.TWINS):
        w = SO.world(product, A, twin)
        fmt = w.fmt()
        blocks = w.blocks(w.chain_volume)
        entries, held = w.entries(w.chain_volume, blocks)
        blocks.put("A")
        a_coords = w.fixed(w.rng.uniform(-0.25, 1.25, size=shape + (3,)).astype(np.float32))
        a_lod = w.fixed(w.rng.uniform(0.0, 1.0, size=shape).astype(np.float32))
        a_up = w.fixed(w.rng.normal(0.0, 1.0, size=(3,) + shape).astype(np.float32))

        def produce():
            return (a_coords * -1.0 + 1.0).requires_grad_(True), (a_lod * 1.5 + 0.25).requires_grad_(True)

        def through_autograd(coords, lod, upstream):
            """On synchronised tensors: (bits of the output and both gradients, the host's time for forward and backward)."""
            coords, lod = coords.clone().requires_grad_(True), lod.clone().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = product.sample_volume(w.dec3, entries, fmt, VOLUME_SAMPLER, 0, SO.LEVELS, coords, lod, lod_bias=0.25)
            gc, gl = torch.autograd.grad(out, (coords, lod), upstream)
            wall_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            return [SO.bits(t) for t in (out.detach(), gc, gl)], wall_ms

        def direct(coords, lod, upstream):
            out, gc, gl = w.out((3,) + shape, torch.float32), w.out(shape + (3,), torch.float32), w.out(shape, torch.float32)
            torch.cuda.synchronize()
            SO.ok(w, product.sample_volume_tensors_device(w.dec3, entries, fmt, VOLUME_SAMPLER, [(0, SO.LEVELS, coords, lod, out, 0.25)]))
            SO.ok(w, product.sample_volume_grad(w.dec3, entries, fmt, VOLUME_SAMPLER, [(0, SO.LEVELS, coords, lod, upstream, gc, gl, 0.25)]))
            torch.cuda.synchronize()
            return [SO.bits(t) for t in (out, gc, gl)]

        # on the inputs A: what a stale read would give; the first pass pays for what torch and the context set up once, the
        # second is how long the host takes over forward and backward
        through_autograd(a_coords, a_lod, a_up)
        other, wall_ms = through_autograd(a_coords, a_lod, a_up)
        assert other == direct(a_coords, a_lod, a_up)
        # (the blocks the allocator hands out next hold NaNs until the queued kernels have run)
        poison = [torch.full_like(t, float("nan")) for t in (a_coords, a_lod, a_up) for _ in range(8)]
        del poison
        torch.cuda.synchronize()
        start, mid, end = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        start.record()
        torch.cuda._sleep(SO.SLEEP)
        coords, lod = produce()
        mid.record()
        out = product.sample_volume(w.dec3, entries, fmt, VOLUME_SAMPLER, 0, SO.LEVELS, coords, lod, lod_bias=0.25)
        torch.cuda._sleep(SO.SLEEP)
        upstream = a_up * 2.0 - 0.5
        end.record()
        gc, gl = torch.autograd.grad(out, (coords, lod), upstream)
        torch.cuda.synchronize()
        SO.check_delay("sample_volume", min(start.elapsed_time(mid), mid.elapsed_time(end)), wall_ms)
        # the same tensors, materialised and synchronised, through the two calls
        want = direct(coords.detach().clone(), lod.detach().clone(), upstream.clone())
        assert all(x != y for x, y in zip(want, other)), "the calls give the same on A and on B: the case proves nothing"
        assert [SO.bits(t) for t in (out.detach(), gc, gl)] == want, twin
