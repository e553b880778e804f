# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_cube_tensors_device on the GPU: device-resident compressed cube maps sampled at buffers of directions with
a level of detail per point into tensors.

Every case is bit for bit against the numpy model of the header's comment (tests/sample_cube_model.py) applied to what the
REFERENCE decoder writes for every whole level (the `ref` fixture, through the C ABI) -- never to anything the new call produced.
Every output buffer starts guard-filled and is compared whole; padded and tight pitches alternate, for the outputs, the directions
and the levels of detail (whose padding holds NaNs).  A chain is five levels of faces 20, 10, 5, 2, 1 with two cubes (12 layers),
every level a stream of its own with a constant-colour and a reserved-mode block where it has three blocks; the footprints are
4x4, 6x6, 8x5 and 12x12: several blocks a face with a partial last one, down to faces smaller than a block."""
import ctypes as C

import numpy as np
import pytest

import sample_cube_model as K
import sample_model as S
import tensor_model as M
from test_decode_scaled import GUARD, SCALE, BIAS, dev
from test_decode_sample import contexts  # noqa: F401  (the fixture)
from test_decode_lod import grid_message, log_names, make_chain

pytestmark = pytest.mark.gpu

FOOTPRINTS = {"4x4": (4, 4), "6x6": (6, 6), "8x5": (8, 5), "12x12": (12, 12)}
FILTERS = (K.NEAREST, K.BILINEAR)
MIPS = (K.MIP_NEAREST, K.MIP_LINEAR)
FACE_SIZES = (20, 10, 5, 2, 1)
SHAPES = ((70, 1), (33, 3), (19, 11))


@pytest.fixture(scope="module")
def chains(product, ref, A):
    """Per footprint: the chain of faces 20, 10, 5, 2, 1, two cubes."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_chain(product, ref, A, FOOTPRINTS[name], [(s, s) for s in FACE_SIZES], depth=12, seed=70 + len(made))
        return made[name]
    return get


@pytest.fixture(scope="module")
def pow2(product, ref, A):
    """4x4: faces of 16, 8 and 4 texels, two cubes."""
    return make_chain(product, ref, A, (4, 4), [(16, 16), (8, 8), (4, 4)], depth=12, seed=90)


class Out:
    """A guard-filled device buffer for one grid's tensor and device buffers of its directions and levels of detail, tight or with
    padded pitches."""

    def __init__(self, dirs, lod, ttype, layout, channels, padded=False, dirs_padded=False, lod_padded=False, front=64):
        import torch
        dirs = np.ascontiguousarray(dirs, dtype=np.float32)
        oy, ox = dirs.shape[:2]
        self.dirs, self.lod, self.out, self.ttype, self.layout, self.channels, self.front, self.padded = dirs, lod, (ox, oy), ttype, layout, channels, front, padded
        self.element = 4 if ttype == M.F32 else 2
        self.row = (ox if layout == M.PLANAR else ox * channels) + (3 if padded else 0)
        self.plane = self.row * oy + (5 if padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * channels if layout == M.PLANAR else self.row * oy
        self.buf = torch.full((front + elements * self.element + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + front
        # (the padding of a row of directions or of levels of detail holds NaNs: read into a point they would show)
        held = np.full((oy, 3 * ox + (5 if dirs_padded else 0)), np.nan, dtype=np.float32)
        held[:, :3 * ox] = dirs.reshape(oy, 3 * ox)
        self.dbuf = dev(held)
        self.drow = held.shape[1]
        self.dirs_padded, self.lod_padded = dirs_padded, lod_padded
        self.lbuf, self.lrow = None, 0
        if lod is not None:
            held = np.full((oy, ox + (5 if lod_padded else 0)), np.nan, dtype=np.float32)
            held[:, :ox] = lod
            self.lbuf = dev(held)
            self.lrow = held.shape[1]

    def grid(self, A, first_entry, level_count, cube, bias, zero_pitches=False):
        pitches = (0, 0) if zero_pitches and not self.padded else (self.row, self.plane)
        drow = 0 if zero_pitches and not self.dirs_padded else self.drow
        lrow = 0 if zero_pitches and not self.lod_padded else self.lrow
        return A.CubeGrid(first_entry, level_count, cube, self.out[0], self.out[1], self.dbuf.data_ptr(), drow, self.lbuf.data_ptr() if self.lbuf is not None else None, lrow,
                          bias, self.ptr, *pitches)

    def want(self, chain, cube, sampler, bias, scale, fbias):
        want = np.full(self.buf.numel(), GUARD, dtype=np.uint8).view(M.BITS_DTYPE[self.ttype])
        bits = K.convert(chain, cube, sampler[0], sampler[1], self.dirs, self.lod, bias, self.ttype, self.channels, scale, fbias)
        M.scatter(want, self.front // self.element, bits, self.layout, 0, self.row, self.row * self.out[1], self.plane)
        return want

    def got(self):
        return self.buf.cpu().numpy().view(M.BITS_DTYPE[self.ttype])


def run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, cases, turn=0, what=""):
    """entries: ImageSetEntry per entry, texels: the reference's [12, s, s, 4] per entry; cases: [(first entry, levels, cube, dirs
    [H, W, 3], lod [H, W] or None, lod_bias)], all in one call.  Returns the outputs' bits."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    outs, grids = [], []
    for i, (first, count, cube, dirs, lod, bias) in enumerate(cases):
        o = Out(dirs, lod, ttype, layout, channels, padded=(i + turn) % 2 == 1, dirs_padded=(i + turn) % 4 >= 2, lod_padded=(i + turn) % 3 == 1)
        outs.append(o)
        grids.append(o.grid(A, first, count, cube, bias, zero_pitches=(i + turn) % 3 == 0))
    err = product.sample_cube_tensors_device(ctx, entries, fmt, A.CubeSampler(*sampler), grids)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    got_all = []
    for o, (first, count, cube, dirs, lod, bias) in zip(outs, cases):
        chain = [texels[first + l] for l in range(count)]
        got, want = o.got(), o.want(chain, cube, sampler, bias, scale32, bias32)
        if not np.array_equal(got, want):
            at = int(np.argwhere(got != want)[0][0])
            raise AssertionError("%s sampler %r grid %dx%d of entries %d..%d cube %d%s: first differing element at %d (row %d, plane %d): got 0x%x, want 0x%x; %d differ" %
                                 (what, sampler, o.out[0], o.out[1], first, first + count - 1, cube, " padded" if o.padded else "", at - o.front // o.element, o.row, o.plane,
                                  got[at], want[at], int((got != want).sum())))
        got_all.append(got)
    return got_all


def random_points(seed, shape, levels):
    """Seeded directions -- half of them near the cube corner (1, 1, 1) and its edges, the rest anywhere -- and lambda over
    [-1, levels + 0.5] with integers and infinities among them: [shape[1], shape[0], 3] and [shape[1], shape[0]]."""
    rng = np.random.default_rng(seed)
    n = shape[0] * shape[1]
    near = np.array([1.0, 1.0, 1.0]) * rng.choice([-1.0, 1.0], size=(n // 2, 3)) + rng.uniform(-0.3, 0.3, size=(n // 2, 3))
    dirs = np.concatenate([near, rng.normal(size=(n - n // 2, 3))]).astype(np.float32)
    lod = rng.uniform(-1.0, levels + 0.5, size=n).astype(np.float32)
    special = np.array([0.0, 1.0, levels - 1.0, np.inf, -np.inf, 2.0, float(levels), -1.0], dtype=np.float32)
    lod[rng.permutation(n)[:len(special)]] = special
    return dirs.reshape(shape[1], shape[0], 3), lod.reshape(shape[1], shape[0])


def entries_of(chain, tname):
    return [s.entry(tname) for s in chain]


def texels_of(chain, profile, tname):
    return [s.texels(profile, tname) for s in chain]


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_random_directions_and_levels(product, A, contexts, chains, name):
    """The three grid shapes under both filters and both mip filters, cubes 0 and 1 of a U8 chain; the 33 x 3 grid again scaled by
    1e-30 and by 1e30, which gives the unscaled bytes wherever the model's samples are equal."""
    chain = chains(name)
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    assert [t.shape[:3] for t in texels] == [(12, s, s) for s in FACE_SIZES]
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, n, (i + filt) % 2) + random_points(100 * filt + 10 * mip + i, shape, n) + (0.0,) for i, shape in enumerate(SHAPES)]
            d, lod = cases[1][3], cases[1][4]
            cases += [(0, n, cases[1][2], d * np.float32(1e-30), lod, 0.0), (0, n, cases[1][2], d * np.float32(1e30), lod, 0.0)]
            got = run_and_check(product, A, ctx, entries, texels, (filt, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + 2 * mip, what=name + " random")
            assert len(got) == 5
            # (every buffer has been compared with the model; the scaled directions are not vacuous: most of their samples are the
            #  unscaled ones' -- the components round on their own when scaled by a value that is no power of two, which moves a
            #  face coordinate by a few units in its last place -- and where the model's are equal the bytes are)
            model = [K.sample(texels, cases[k][2], filt, mip, cases[k][3], lod, 0.0) for k in (1, 3, 4)]
            same = sum(int((m.view(np.uint32) == model[0].view(np.uint32)).all(axis=-1).sum()) for m in model[1:])
            assert same > 33 * 3


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_constructed_directions(product, A, contexts, chains, name):
    """The CPU test's constructed directions (the edges and corners of every face size, the ties, the axes, zeros of either sign,
    subnormal and huge components, the invalid ones) as one 19-wide grid, lambda' from a lod that turns through the levels."""
    chain = chains(name)
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    made = K.constructed_directions()
    grid = np.concatenate([made, np.tile(made[:1], (-len(made) % 19, 1))]).reshape(-1, 19, 3)
    lod = (np.arange(grid.shape[0] * 19, dtype=np.float32).reshape(-1, 19) * np.float32(0.375)) % np.float32(n)
    run_and_check(product, A, ctx, entries, texels, (K.BILINEAR, K.MIP_LINEAR), (M.F32, M.PLANAR, 4), [(0, n, 1, grid, lod, -0.25)], turn=1, what=name + " constructed")
    run_and_check(product, A, ctx, entries, texels, (K.NEAREST, K.MIP_NEAREST), (M.BF16, M.INTERLEAVED, 2), [(0, n, 0, grid, None, 1.0)], turn=0, what=name + " constructed")


@pytest.mark.parametrize("ttype,layout", [(t, l) for t in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED)])
def test_formats_profiles_and_a_chain_of_mixed_data_types(product, A, contexts, chains, ttype, layout):
    """Every tensor type with both layouts; 1, 3 and 4 channels; U8, F16 and F32 levels in one chain and one call; the LDR, sRGB
    and HDR profiles (under HDR the reserved-mode block of an F16 level is NaN)."""
    chain = chains("6x6")
    n = len(chain)
    names = [("u8", "f16", "f32")[l % 3] for l in range(n)]
    entries = [s.entry(t) for s, t in zip(chain, names)]
    for k, channels in enumerate((1, 3, 4)):
        profile = (A.PRF_LDR, A.PRF_LDR_SRGB, A.PRF_HDR)[(k + ttype + layout) % 3]
        ctx = contexts(chain[0].block, profile)
        texels = [s.texels(profile, t) for s, t in zip(chain, names)]
        cases = [(0, n, i % 2) + random_points(31 * channels + i, shape, n) + (0.25 * i,) for i, shape in enumerate(SHAPES[1:])]
        # (a chain of one level with a null lod: a cube without mips)
        cases.append((1, 1, 1, random_points(5 + channels, (33, 3), 1)[0], None, 0.0))
        filt = (channels + layout) % 2
        run_and_check(product, A, ctx, entries, texels, (filt, (channels + ttype) % 2), (ttype, layout, channels), cases, turn=channels + ttype, what="formats")


def centres(s, faces=range(6)):
    """The directions through the texel centres of the faces: [len(faces) * s, s, 3], row f * s + y."""
    return np.array([[K.direction(f, x + 0.5, y + 0.5, s) for x in range(s)] for f in faces for y in range(s)], dtype=np.float32)


def test_texel_centres_give_the_tensors_call_bytes(product, A, contexts, pow2):
    """s = 16 at 4x4: the directions through the texel centres of face f give, under either filter, the bytes that
    astcenc_amd_decompress_tensors_device writes for layer 6 cube + f."""
    import torch
    ctx = contexts((4, 4), A.PRF_HDR)
    entries, texels = entries_of(pow2, "f16"), texels_of(pow2, A.PRF_HDR, "f16")
    assert np.isnan(texels[0].astype(np.float32)).any()
    fmt = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 4, SCALE, BIAS)
    for cube in (0, 1):
        whole = torch.full((4, 6, 16, 16), 7.0, dtype=torch.float32, device="cuda")
        err = product.decompress_tensors_device(ctx, entries, fmt, [(0, (0, 0, 6 * cube), (16, 16, 6), whole)])
        assert err == A.SUCCESS, product.error_string(err)
        torch.cuda.synchronize()
        whole = whole.cpu().numpy().view(np.uint32)
        for filt in FILTERS:
            for mip in MIPS:
                got = run_and_check(product, A, ctx, entries, texels, (filt, mip), (M.F32, M.PLANAR, 4), [(0, 3, cube, centres(16), None, 0.0)], what="centres")[0]
                got = got[16:16 + 4 * 96 * 16].reshape(4, 6, 16, 16)
                assert np.array_equal(got, whole), (cube, filt, mip)


def test_inside_one_face_gives_the_lod_call_bytes_under_clamp(product, A, contexts, pow2):
    """Faces of 16, 8 and 4 texels: points at dyadic face coordinates (x, y) in [2, 14] of level 0 have all their taps inside the
    face on every level (the model confirms it), so the bytes are those astcenc_amd_sample_lod_tensors_device writes for layer
    6 cube + f under CLAMP at u = x / 16, v = y / 16 and the same lambda: every step on either side is exact."""
    import torch
    ctx = contexts((4, 4), A.PRF_LDR)
    entries, texels = entries_of(pow2, "u8"), texels_of(pow2, A.PRF_LDR, "u8")
    rng = np.random.default_rng(8)
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_INTERLEAVED, 3, SCALE, BIAS)
    for f, cube in ((0, 1), (3, 0), (5, 1)):
        xy = rng.integers(16, 113, size=(11, 19, 2)).astype(np.float32) / np.float32(8.0)
        xy[0, 0], xy[0, 1] = (2.0, 14.0), (14.0, 2.5)
        lod = rng.uniform(-0.5, 2.5, size=(11, 19)).astype(np.float32)
        lod[1, :3] = (0.0, 1.0, 2.0)
        dirs = np.array([[K.direction(f, float(x), float(y), 16) for x, y in row] for row in xy], dtype=np.float32)
        uv = xy / np.float32(16.0)
        for d, (x, y) in zip(dirs.reshape(-1, 3), xy.reshape(-1, 2)):
            ff, sc, tc, ma = K.face_of(d)
            p, q = K.quotients(sc, tc, ma)
            assert ff == f
            for s in (16, 8, 4):
                assert (K.face_coordinate(p, s), K.face_coordinate(q, s)) == (float(x) * s / 16, float(y) * s / 16)
                for _, row in K.point_taps(K.BILINEAR, ff, K.face_coordinate(p, s), K.face_coordinate(q, s), s):
                    assert all(0 <= ix < s and 0 <= iy < s for _, _, (ix, iy) in row)
        for filt in FILTERS:
            for mip in MIPS:
                got = run_and_check(product, A, ctx, entries, texels, (filt, mip), (M.F16, M.INTERLEAVED, 3), [(0, 3, cube, dirs, lod, 0.0)], what="inside")[0]
                out = torch.full((11, 19, 3), 7.0, dtype=torch.float16, device="cuda")
                err = product.sample_lod_tensors_device(ctx, entries, fmt, (filt, S.CLAMP, S.CLAMP, mip), [(0, 3, 6 * cube + f, dev(uv), dev(lod), out)])
                assert err == A.SUCCESS, product.error_string(err)
                torch.cuda.synchronize()
                assert np.array_equal(got[32:32 + 11 * 19 * 3], out.cpu().numpy().view(np.uint16).reshape(-1)), (f, cube, filt, mip)


def test_nan_behind_a_tap_or_a_level_of_weight_zero(product, A, contexts, pow2):
    """F16 levels under the HDR profile: the reserved-mode block of levels 0 and 1 is NaN.  Texel centres have fr = 0 on both axes:
    the NaN texels' neighbours must stay numbers; and at lambda' = 0 and 2 under MIP_LINEAR g = 0: level 1, NaNs and all, is not
    read.  The model leaves zero weights out, and every bit is compared with it."""
    ctx = contexts((4, 4), A.PRF_HDR)
    entries, texels = entries_of(pow2, "f16"), texels_of(pow2, A.PRF_HDR, "f16")
    nan0 = np.isnan(texels[0].astype(np.float32)).any(axis=-1)
    assert nan0.any() and not nan0.all() and np.isnan(texels[1].astype(np.float32)).any()
    d = centres(16)
    lod = np.zeros(d.shape[:2], dtype=np.float32)
    lod[::2] = 2.0
    got = run_and_check(product, A, ctx, entries, texels, (K.BILINEAR, K.MIP_LINEAR), (M.F32, M.INTERLEAVED, 4), [(0, 3, 0, d, lod, 0.0), (0, 3, 1, d, None, 0.0)], what="nan")
    level0 = np.isnan(got[1][16:16 + 96 * 16 * 4].view(np.float32).reshape(6, 16, 16, 4)).any(axis=-1)
    assert np.array_equal(level0, nan0[6:12])


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, chains):
    """Every error the cube call adds to the lod call's, and a few of those it shares, each with nothing written.  (Not among the
    cases: a `dirs` on another device than entry 0's blocks -- on one GPU there is no such pointer to give.)"""
    import torch
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((3, 40 * 40 * 4 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        d, lod = random_points(1, (40, 40), n)
        dirs, lods = dev(d), dev(lod)
        dptr, lptr = dirs.data_ptr(), lods.data_ptr()
        # first_entry, level_count, cube, out_x, out_y, dirs, dir_row_pitch, lod, lod_row_pitch, lod_bias, out, row_pitch, plane_pitch
        good = [A.CubeGrid(0, n, 0, 30, 20, dptr, 120, lptr, 40, 0.0, out[0].data_ptr(), 0, 0), A.CubeGrid(1, 1, 1, 40, 40, dptr, 0, lptr, 0, 0.5, out[1].data_ptr(), 0, 0),
                A.CubeGrid(2, 3, 1, 30, 40, dptr, 0, None, 0, 1.0, out[2].data_ptr(), 0, 0)]
        entries = entries_of(chain, "u8")

        def call(fmt, grids, sampler=A.CubeSampler(A.SAMPLE_BILINEAR, A.MIP_LINEAR), entry_list=None, context=None):
            en = entry_list or entries
            arr = (A.ImageSetEntry * len(en))(*en)
            garr = (A.CubeGrid * len(grids))(*grids)
            return product.lib.astcenc_amd_sample_cube_tensors_device(context or ctx, arr, len(en), C.byref(fmt) if fmt is not None else None,
                                                                      C.byref(sampler) if sampler is not None else None, garr, len(grids), None)

        def grid(index, **change):
            g = [A.CubeGrid.from_buffer_copy(x) for x in good]
            for k, v in change.items():
                setattr(g[index], k, v)
            return g

        def entry(index, **change):
            en = [A.ImageSetEntry.from_buffer_copy(x) for x in entries]
            for k, v in change.items():
                setattr(en[index], k, v)
            return en

        fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
        cases = [
            # the cube call's own
            ("a level that is not square", good, A.ERR_BAD_PARAM, "grid 0 of 3", dict(entry_list=entry(3, dim_y=4))),
            ("a level whose layers are no multiple of six", good[1:], A.ERR_BAD_PARAM, "grid 1 of 2", dict(entry_list=entry(4, dim_z=11))),
            ("a cube beyond the layers", grid(1, cube=2), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("a cube beyond the layers of one level", grid(2, cube=1), A.ERR_BAD_PARAM, "grid 2 of 3", dict(entry_list=entry(3, dim_z=6))),
            ("a cube that wraps 32 bits", grid(0, cube=0x2AAAAAAB), A.ERR_BAD_PARAM, "grid 0 of 3", {}),
            ("a face above 65536 texels", good, A.ERR_BAD_PARAM, "grid 0 of 3", dict(entry_list=entry(1, dim_x=65537, dim_y=65537, dim_z=6, blocks_len=1 << 40))),
            ("directions not aligned to 4 bytes", grid(1, dirs=dptr + 2), A.ERR_BAD_PARAM, grid_message(1, 3, "dirs 0x... is not aligned to a float (4 bytes)"), {}),
            ("a dir_row_pitch below 3 out_x", grid(0, dir_row_pitch=89), A.ERR_BAD_PARAM, grid_message(0, 3, "dir_row_pitch 89: at least 90 floats"), {}),
            ("null directions", grid(2, dirs=None), A.ERR_BAD_CONTEXT, grid_message(2, 3, "dirs is null"), {}),
            # shared with the lod call
            ("a null sampler", good, A.ERR_BAD_PARAM, "sampler", dict(sampler=None)),
            ("an unknown mip filter", good, A.ERR_BAD_PARAM, "mip_filter", dict(sampler=A.CubeSampler(1, 2))),
            ("an unknown filter", good, A.ERR_BAD_PARAM, "filter", dict(sampler=A.CubeSampler(2, 0))),
            ("no levels", grid(1, level_count=0), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("levels beyond the entries", grid(2, first_entry=n - 1), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("an infinite lod_bias", grid(2, lod_bias=float("inf")), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("a lod not aligned to 4 bytes", grid(1, lod=lptr + 2), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("a lod_row_pitch below out_x", grid(0, lod_row_pitch=29), A.ERR_BAD_PARAM, "grid 0 of 3", {}),
            ("a zero out_x", grid(1, out_x=0), A.ERR_BAD_PARAM, "grid 1 of 3", {}),
            ("a row pitch below the output's", grid(2, row_pitch=29), A.ERR_BAD_PARAM, "grid 2 of 3", {}),
            ("a null out", grid(2, out=None), A.ERR_BAD_CONTEXT, "grid 2 of 3", {}),
        ]
        for what, grids, code, named, kw in cases:
            del logged[:]
            assert call(fmt, grids, **kw) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(log_names(named, m) for m in logged), (what, logged)
        # a context whose footprint is 3D
        del logged[:]
        assert call(fmt, good, context=contexts((3, 3, 3), A.PRF_LDR)) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all()) and any("3D" in m for m in logged), logged
        # directions and levels of detail are data: none of them is an error -- and the good call is good (a null lod included)
        assert call(fmt, good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:, :64] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
