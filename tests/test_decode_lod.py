# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_lod_tensors_device on the GPU: device-resident compressed mip chains sampled at buffers of normalised
coordinates with a level of detail per point into tensors.

Every case is bit for bit against the numpy model of the header's comment (tests/sample_lod_model.py) applied to what the
REFERENCE decoder writes for every whole level (the `ref` fixture, through the C ABI) -- never to anything the new call produced.
Every output buffer starts guard-filled and is compared whole: the addressed elements must be the model's and every other byte
the guard; padded and tight pitches alternate, for the outputs, the coordinates and the levels of detail (whose padding holds
NaNs).  A chain is the full mip chain of the 17 x 17-block image (6x6: 102, 51, 25, 12, 6, 3, 1), every level a stream of its own
(tests/test_decode_scaled.py's make_stream with its own seed, with a constant-colour and a reserved-mode block where the level has
three blocks), so the levels look nothing alike."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sample_lod_model as L
import sample_model as S
import tensor_model as M
from test_decode_scaled import FOOTPRINTS, GUARD, SCALE, BIAS, dev, make_stream, type_of
from test_decode_sample import MODES, FILTERS, Source, contexts  # noqa: F401  (contexts: the fixture)

pytestmark = pytest.mark.gpu

MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)


def grid_message(i, count, tail):
    """A pattern for the whole of a log line after the entry point's name: "grid i of count: " and `tail`, in which "0x..." stands
    for a pointer (the bad-argument tests of the lod, lod-grad, cube and volume calls)."""
    return re.compile(re.escape(": grid %d of %d: %s" % (i, count, tail)).replace(re.escape("0x..."), "0x[0-9a-f]+") + r"\Z")


def log_names(named, message):
    """`named` is in the log line `message`: a fragment of it, or a pattern of grid_message's."""
    return bool(named.search(message)) if isinstance(named, re.Pattern) else named in message


def make_chain(product, ref, A, block, dims, depth=1, seed=5):
    """A Source per level of the sizes `dims`."""
    chain = []
    for l, (w, h) in enumerate(dims):
        blocks = -(-w // block[0]) * -(-h // block[1]) * depth
        size = (w, h) if depth == 1 else (w, h, depth)
        chain.append(Source(ref, A, block, size, make_stream(product, A, block, w, h, depth=depth, seed=seed + 7 * l, special=blocks >= 3)))
    return chain


@pytest.fixture(scope="module")
def chains(product, ref, A):
    """Per footprint: the full chain of the 17 x 17-block image."""
    made = {}

    def get(name):
        if name not in made:
            bx, by = FOOTPRINTS[name]
            made[name] = make_chain(product, ref, A, (bx, by), L.chain_dims(17 * bx, 17 * by))
        return made[name]
    return get


class Out:
    """A guard-filled device buffer for one grid's tensor and device buffers of its coordinates and levels of detail, tight or
    with padded pitches."""

    def __init__(self, coords, lod, ttype, layout, channels, padded=False, coords_padded=False, lod_padded=False, front=64):
        import torch
        coords = np.ascontiguousarray(coords, dtype=np.float32)
        oy, ox = coords.shape[:2]
        self.coords, self.lod, self.out, self.ttype, self.layout, self.channels, self.front, self.padded = coords, lod, (ox, oy), ttype, layout, channels, front, padded
        self.element = 4 if ttype == M.F32 else 2
        self.row = (ox if layout == M.PLANAR else ox * channels) + (3 if padded else 0)
        self.plane = self.row * oy + (5 if padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * channels if layout == M.PLANAR else self.row * oy
        self.buf = torch.full((front + elements * self.element + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + front
        # (the padding of a row of coordinates or of levels of detail holds NaNs: read into a point they would show)
        held = np.full((oy, ox + (3 if coords_padded else 0), 2), np.nan, dtype=np.float32)
        held[:, :ox] = coords
        self.cbuf = dev(held)
        self.crow = held.shape[1] * 2
        self.coords_padded, self.lod_padded = coords_padded, lod_padded
        self.lbuf, self.lrow = None, 0
        if lod is not None:
            held = np.full((oy, ox + (5 if lod_padded else 0)), np.nan, dtype=np.float32)
            held[:, :ox] = lod
            self.lbuf = dev(held)
            self.lrow = held.shape[1]

    def grid(self, A, first_entry, level_count, z, bias, zero_pitches=False):
        pitches = (0, 0) if zero_pitches and not self.padded else (self.row, self.plane)
        crow = 0 if zero_pitches and not self.coords_padded else self.crow
        lrow = 0 if zero_pitches and not self.lod_padded else self.lrow
        return A.LodGrid(first_entry, level_count, z, self.out[0], self.out[1], self.cbuf.data_ptr(), crow, self.lbuf.data_ptr() if self.lbuf is not None else None, lrow,
                         bias, self.ptr, *pitches)

    def want(self, chain, sampler, bias, scale, fbias):
        want = np.full(self.buf.numel(), GUARD, dtype=np.uint8).view(M.BITS_DTYPE[self.ttype])
        bits = L.convert(chain, sampler[0], sampler[1], sampler[2], sampler[3], self.coords, self.lod, bias, self.ttype, self.channels, scale, fbias)
        M.scatter(want, self.front // self.element, bits, self.layout, 0, self.row, self.row * self.out[1], self.plane)
        return want

    def got(self):
        return self.buf.cpu().numpy().view(M.BITS_DTYPE[self.ttype])


def run_and_check(product, A, ctx, entries, texels, sampler, fmt_args, cases, turn=0, what=""):
    """entries: ImageSetEntry per entry, texels: the reference's [D, H, W, 4] per entry; cases: [(first entry, levels, z, coords
    [H, W, 2], lod [H, W] or None, lod_bias)], all in one call: padded and tight pitches alternate for outputs, coordinates and
    levels of detail, tight ones as zeros or spelled out.  Returns the outputs' bits."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    outs, grids = [], []
    for i, (first, count, z, coords, lod, bias) in enumerate(cases):
        o = Out(coords, lod, ttype, layout, channels, padded=(i + turn) % 2 == 1, coords_padded=(i + turn) % 4 >= 2, lod_padded=(i + turn) % 3 == 1)
        outs.append(o)
        grids.append(o.grid(A, first, count, z, bias, zero_pitches=(i + turn) % 3 == 0))
    err = product.sample_lod_tensors_device(ctx, entries, fmt, A.LodSampler(*sampler), grids)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    got_all = []
    for o, (first, count, z, coords, lod, bias) in zip(outs, cases):
        chain = [texels[first + l][z] for l in range(count)]
        got, want = o.got(), o.want(chain, sampler, bias, scale32, bias32)
        if not np.array_equal(got, want):
            at = int(np.argwhere(got != want)[0][0])
            raise AssertionError("%s sampler %r grid %dx%d of entries %d..%d slice %d%s: first differing element at %d (row %d, plane %d): got 0x%x, want 0x%x; %d differ" %
                                 (what, sampler, o.out[0], o.out[1], first, first + count - 1, z, " padded" if o.padded else "", at - o.front // o.element, o.row, o.plane,
                                  got[at], want[at], int((got != want).sum())))
        got_all.append(got)
    return got_all


def random_points(seed, shape, levels, lo=-0.25, hi=1.25):
    """Seeded (u, v) uniform over [lo, hi] and lambda uniform over [-1, levels + 0.5]: [shape[1], shape[0], 2] and [shape[1], shape[0]]."""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(lo, hi, size=(shape[1], shape[0], 2)).astype(np.float32)
    lod = rng.uniform(-1.0, levels + 0.5, size=(shape[1], shape[0])).astype(np.float32)
    return uv, lod


def entries_of(chain, tname):
    return [s.entry(tname) for s in chain]


def texels_of(chain, profile, tname):
    return [s.texels(profile, tname) for s in chain]


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_random_points_and_levels_under_every_address_mode(product, A, contexts, chains, name):
    """Seeded 37 x 11 grids of (u, v) in [-0.25, 1.25] with lambda in [-1, L + 0.5]: every address mode x both filters x both mip
    filters (the same mode on both axes under MIP_NEAREST, the modes mixed under MIP_LINEAR), a U8 chain next to the same streams
    as an F16 chain under the HDR profile (the reserved-mode blocks are NaN there)."""
    chain = chains(name)
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_HDR)
    entries = entries_of(chain, "u8") + entries_of(chain, "f16")
    texels = texels_of(chain, A.PRF_HDR, "u8") + texels_of(chain, A.PRF_HDR, "f16")
    assert any(np.isnan(t).any() for t in texels[n:])
    for filt in FILTERS:
        for k, mode in enumerate(MODES):
            for mip in MIPS:
                ay = mode if mip == L.MIP_NEAREST else MODES[(k + 1) % 4]
                cases = [(e * n, n, 0) + random_points(100 * filt + 10 * k + 2 * mip + e, (37, 11), n) + (0.0,) for e in range(2)]
                run_and_check(product, A, ctx, entries, texels, (filt, mode, ay, mip), (M.F16, M.PLANAR, 3), cases, turn=k + filt + mip, what=name + " random")


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_256_distinct_blocks_in_the_level_0_pass(product, A, contexts, chains, name):
    """A 64 x 1 grid at the level-0 block corners (bx i, by j), i, j even in 2 .. 16, with lambda = 0.5: BILINEAR has its four
    level-0 taps in four blocks and no two points share one -- 256 distinct blocks, eight full batches in the level-0 pass
    (tests/harness/decode_lod_check.cpp counts them), and under MIP_LINEAR the level-1 pass follows.  And 64 equal points."""
    chain = chains(name)
    n = len(chain)
    bx, by = chain[0].block
    w, h = chain[0].dims
    ctx = contexts(chain[0].block, A.PRF_LDR)
    corners = np.array([[(i / 17.0, j / 17.0) for j in range(2, 17, 2) for i in range(2, 17, 2)]], dtype=np.float32)
    assert corners.shape == (1, 64, 2)
    # (i / 17 is not a binary32, but u W is within a hair of the corner: the taps are the corner's)
    blocks = {(int(np.floor(float(u) * w - 0.5) + dx) // bx, int(np.floor(float(v) * h - 0.5) + dy) // by) for u, v in corners[0] for dx in (0, 1) for dy in (0, 1)}
    assert len(blocks) == 256
    half = np.full((1, 64), 0.5, dtype=np.float32)
    equal = np.tile(np.array([[(0.3, 0.7)]], dtype=np.float32), (1, 64, 1))
    order = np.random.default_rng(1).permutation(64)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, n, 0, corners, half, 0.0), (0, n, 0, equal, np.full((1, 64), 1.25, dtype=np.float32), 0.0), (0, n, 0, corners[:, order], None, 0.5)]
            run_and_check(product, A, ctx, entries, texels, (filt, S.CLAMP, S.CLAMP, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + mip, what=name + " corners")


def test_integer_lambda_is_the_sample_call_on_a_power_of_two_chain(product, ref, A, contexts):
    """The chain of a 64 x 32 image at 4x4 (64 x 32, 32 x 16, 16 x 8, ...), every level F16 under the HDR profile: where lambda' is
    an integer the bytes are those of astcenc_amd_sample_tensors_device on that entry at (u W, v H), under either mip filter --
    and level 1, the neighbour that is not read at lambda' = 0 and 2, holds NaNs."""
    import torch
    block = (4, 4)
    dims = L.chain_dims(64, 32)
    assert dims[:3] == [(64, 32), (32, 16), (16, 8)] and len(dims) == 7
    chain = make_chain(product, ref, A, block, dims, seed=40)
    ctx = contexts(block, A.PRF_HDR)
    entries, texels = entries_of(chain, "f16"), texels_of(chain, A.PRF_HDR, "f16")
    assert np.isnan(texels[1]).any() and not np.isnan(texels[1]).all()
    uv, _ = random_points(9, (37, 11), len(dims))
    # (points over the NaN block of level 1 -- block 2 of its first row -- among them)
    uv[0, :8, 0] = np.linspace(8.5 / 32, 11.5 / 32, 8, dtype=np.float32)
    uv[0, :8, 1] = np.float32(1.5 / 16)
    fmt = A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4, SCALE, BIAS)
    for level in (0, 2, 1, 6):
        w, h = dims[level]
        texel = uv * np.array([w, h], dtype=np.float32)
        assert np.array_equal(texel.astype(np.float64), uv.astype(np.float64) * np.array([w, h], dtype=np.float64))
        for filt in FILTERS:
            sampled = torch.full((11, 37, 4), 7.0, dtype=torch.float32, device="cuda")
            tdev = dev(texel)
            err = product.sample_tensors_device(ctx, entries, fmt, (filt, S.REPEAT, S.MIRROR), [(level, 0, tdev, sampled)])
            assert err == A.SUCCESS, product.error_string(err)
            torch.cuda.synchronize()
            sampled = sampled.cpu().numpy()
            if level != 1:
                assert not np.isnan(sampled[0, :8]).any()
            for mip in MIPS:
                # lod + lod_bias is the integer; the last level also from far beyond the chain
                lod = np.full(uv.shape[:2], level + 2.0 if level < 6 else 40.0, dtype=np.float32)
                got = run_and_check(product, A, ctx, entries, texels, (filt, S.REPEAT, S.MIRROR, mip), (M.F32, M.INTERLEAVED, 4), [(0, len(dims), 0, uv, lod, -2.0)],
                                    what="integer lambda")[0]
                assert got[16:16 + 11 * 37 * 4].tobytes() == sampled.tobytes(), (level, filt, mip)


def test_tile_shapes(product, A, contexts, chains):
    """out_y = 1, 2, 3 and 5 (tiles of 64 x 1, 32 x 2, 16 x 4, 8 x 8) with out_x no multiple of the tile's width, and 20 x 17."""
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    shapes = [(70, 1), (35, 2), (19, 3), (11, 5), (20, 17), (1, 1), (64, 1), (65, 4)]
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, n, 0) + random_points(7 + i, s, n) + (0.0,) for i, s in enumerate(shapes)]
            run_and_check(product, A, ctx, entries, texels, (filt, S.MIRROR, S.BORDER, mip), (M.BF16, M.INTERLEAVED, 2), cases, turn=filt + mip, what="shapes")


def test_special_coordinates_and_levels_of_detail(product, A, contexts, chains):
    """The special u and v of the hand checks (edges, -0.0, tiny, negative, NaN, infinities, 2^14 and the next binary32), each
    against each, with the special lambda (negative, the ties, the chain's end and beyond, infinities, NaN) turning through them."""
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
                got = run_and_check(product, A, ctx, entries, texels, (filt, mode, MODES[(k + 2) % 4], mip), (M.F32, M.PLANAR, 4), [(0, n, 0, grid, lod, 0.0)], turn=k + mip,
                                    what="special")
                assert len(got) == 1


@pytest.mark.parametrize("ttype,layout", [(t, l) for t in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED)])
def test_formats_and_a_chain_of_mixed_data_types(product, A, contexts, chains, ttype, layout):
    """Every tensor type with both layouts; channels 1 to 4; a chain whose levels are U8, F16 and F32 in turn."""
    chain = chains("6x6")
    n = len(chain)
    ctx = contexts(chain[0].block, A.PRF_LDR)
    names = [("u8", "f16", "f32")[l % 3] for l in range(n)]
    entries = [s.entry(t) for s, t in zip(chain, names)]
    texels = [s.texels(A.PRF_LDR, t) for s, t in zip(chain, names)]
    shapes = [(45, 9), (67, 3), (29, 7), (8, 2)]
    for channels in range(1, 5):
        cases = [(0, n, 0) + random_points(31 * channels + i, s, n) + (0.25 * i,) for i, s in enumerate(shapes)]
        for filt in FILTERS:
            mip = (channels + filt) % 2
            run_and_check(product, A, ctx, entries, texels, (filt, MODES[channels % 4], MODES[(channels + filt) % 4], mip), (ttype, layout, channels), cases,
                          turn=channels + filt, what="formats")


def test_two_chains_and_a_one_level_chain_in_one_call(product, ref, A, contexts, chains):
    """Grids over the full chain, over its levels 2 .. 4 as a chain of their own, over another image's chain of two levels and
    over one level alone -- where any lambda gives that level -- in one call; lod NULL among them."""
    chain = chains("6x6")
    n = len(chain)
    other = make_chain(product, ref, A, (6, 6), [(40, 30), (13, 50)], seed=60)
    ctx = contexts((6, 6), A.PRF_LDR)
    entries = entries_of(chain, "u8") + entries_of(other, "f32")
    texels = texels_of(chain, A.PRF_LDR, "u8") + texels_of(other, A.PRF_LDR, "f32")
    for filt in FILTERS:
        for mip in MIPS:
            cases = [(0, n, 0) + random_points(1, (37, 11), n) + (0.0,),
                     (2, 3, 0) + random_points(2, (23, 5), 3) + (0.5,),
                     (n, 2, 0) + random_points(3, (19, 3), 2) + (0.0,),
                     (n + 1, 1, 0) + random_points(4, (35, 2), 5) + (0.0,),
                     (n, 2, 0, random_points(5, (33, 1), 2)[0], None, 0.625),
                     (4, 1, 0, random_points(6, (9, 9), 2)[0], None, 0.0)]
            run_and_check(product, A, ctx, entries, texels, (filt, S.REPEAT, S.CLAMP, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + 2 * mip, what="chains")


def test_a_slice_of_an_array_chain(product, ref, A, contexts):
    """Slices 2 and 1 of the chain of a 40 x 30 x 3 array: z selects the slice in every level, nothing is sampled along z."""
    block = (6, 6)
    ctx = contexts(block, A.PRF_LDR)
    dims = L.chain_dims(40, 30, 4)
    assert dims == [(40, 30), (20, 15), (10, 7), (5, 3)]
    chain = make_chain(product, ref, A, block, dims, depth=3, seed=20)
    entries, texels = entries_of(chain, "u8"), texels_of(chain, A.PRF_LDR, "u8")
    assert all(t.shape[0] == 3 for t in texels)
    assert not np.array_equal(texels[1][2], texels[1][1]) and not np.array_equal(texels[1][2], texels[1][0])
    cases = [(0, 4, 2) + random_points(3, (37, 11), 4) + (0.0,), (0, 4, 1) + random_points(4, (23, 5), 4) + (0.0,), (1, 3, 2) + random_points(5, (20, 17), 3) + (0.0,)]
    for filt in FILTERS:
        for mip in MIPS:
            run_and_check(product, A, ctx, entries, texels, (filt, S.REPEAT, S.MIRROR, mip), (M.F16, M.PLANAR, 3), cases, turn=filt + mip, what="slice")


def limit_cases(n):
    return [(0, n, 0) + random_points(1, (37, 11), n) + (0.0,), (0, n, 0) + random_points(2, (70, 1), n) + (0.0,), (1, n - 1, 0) + random_points(3, (19, 3), n - 1) + (0.5,),
            (0, n, 0, random_points(4, (40, 9), n)[0], None, 1.5)]


LIMIT_SCRIPT = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
torch.zeros(1, device="cuda:0")
import astcenc_amd as A
import oracle_libs as O
import sample_lod_model as L, sample_model as S, tensor_model as M
import test_decode_lod as T
gpu, ref = A.Library(A.LIB_PRODUCT), A.Library(O.LIB_REF_NONE)
block = (6, 6)
err, cfg = gpu.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
err, ctx = gpu.context_alloc(cfg, 1)
assert err == 0
chain = T.make_chain(gpu, ref, A, block, L.chain_dims(102, 102))
n = len(chain)
bad = checked = 0
for mip in T.MIPS:
    try:
        checked += len(T.run_and_check(gpu, A, ctx, T.entries_of(chain, "u8"), T.texels_of(chain, A.PRF_LDR, "u8"), (S.BILINEAR, S.CLAMP, S.REPEAT, mip), (M.F16, M.PLANAR, 3),
                                       T.limit_cases(n), what="limit"))
    except AssertionError as e:
        bad += 1
        print("MISMATCH", e)
gpu.context_free(ctx)
print("limit cases checked:", checked, "mismatching:", bad)
"""


def test_tiles_spanning_several_launches(product, ref, A):
    """The 1D grid of tiles cut into launches of two (the limit is read once per process: a fresh child process): the 37 x 11 grid
    alone is ten tiles, and the grids of a call sit anywhere among the launches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ASTCENC_AMD_DECODE_GRID_LIMIT="2")
    script = LIMIT_SCRIPT % (os.path.join(root, "astc-encoder_amd", "python"), os.path.join(root, "oracle"), os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mismatching: 0" in out.stdout and "limit cases checked: 8" in out.stdout, out.stdout[-2000:]


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, chains):
    """(Not among the cases: a `lod` or `coords` buffer on another device than entry 0's blocks -- on one GPU there is no such
    pointer to give, the gap the sample call's suite has too.  The backend's map from a grid's three buffers to the ownership
    check runs on every successful call; grids with and without a `lod` in one call -- here and in
    test_two_chains_and_a_one_level_chain_in_one_call -- pass through both of its branches.)"""
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
        uv, lod = random_points(1, (40, 40), n)
        coords, lods = dev(uv), dev(lod)
        cptr, lptr = coords.data_ptr(), lods.data_ptr()
        # first_entry, level_count, z, out_x, out_y, coords, coord_row_pitch, lod, lod_row_pitch, lod_bias, out, row_pitch, plane_pitch
        good = [A.LodGrid(0, n, 0, 30, 20, cptr, 80, lptr, 40, 0.0, out[0].data_ptr(), 0, 0), A.LodGrid(n, 1, 0, 40, 40, cptr, 0, lptr, 0, 0.5, out[1].data_ptr(), 0, 0),
                A.LodGrid(2, 3, 0, 30, 40, cptr, 0, None, 0, 1.0, out[2].data_ptr(), 0, 0)]
        # (entry n is the 17 x 17-block level again, as F32: a chain of one level)
        entries = entries_of(chain, "u8") + [chain[0].entry("f32")]

        def call(fmt, grids, sampler=A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, A.MIP_LINEAR), context=None, entry_list=None):
            en = entry_list or entries
            arr = (A.ImageSetEntry * len(en))(*en)
            garr = (A.LodGrid * len(grids))(*grids)
            return product.lib.astcenc_amd_sample_lod_tensors_device(context or ctx, arr, len(en), C.byref(fmt) if fmt is not None else None,
                                                                     C.byref(sampler) if sampler is not None else None, garr, len(grids), None)

        def grid(index, **change):
            g = [A.LodGrid.from_buffer_copy(x) for x in good]
            for k, v in change.items():
                setattr(g[index], k, v)
            return g

        def fmt(type=A.TENSOR_F16, layout=A.TENSOR_PLANAR, channels=3, scale=(1.0,) * 4, bias=(0.0,) * 4):
            return A.tensor_format(type, layout, channels, scale, bias)

        inf = float("inf")
        bad_entry = A.ImageSetEntry.from_buffer_copy(entries[1])
        bad_entry.data_type = 7
        huge_level = A.ImageSetEntry.from_buffer_copy(entries[n])
        # (its blocks_len says the stream is there: the entry passes its own checks, and nothing is read before the level's)
        huge_level.dim_x, huge_level.dim_y, huge_level.blocks_len = 65537, 1, 1 << 20
        cases = [
            # the additional ones
            ("a null sampler", fmt(), good, A.ERR_BAD_PARAM, "sampler", dict(sampler=None)),
            ("an unknown mip filter", fmt(), good, A.ERR_BAD_PARAM, "mip_filter", dict(sampler=A.LodSampler(1, 0, 0, 2))),
            ("a negative mip filter", fmt(), good, A.ERR_BAD_PARAM, "mip_filter", dict(sampler=A.LodSampler(1, 0, 0, -1))),
            ("no levels", fmt(), grid(1, level_count=0), A.ERR_BAD_PARAM, "grid 1", {}),
            ("33 levels", fmt(), grid(0, level_count=33), A.ERR_BAD_PARAM, "grid 0", {}),
            ("levels beyond the entries", fmt(), grid(2, first_entry=n - 1), A.ERR_BAD_PARAM, "grid 2", {}),
            ("a first entry beyond the entries", fmt(), grid(1, first_entry=n + 1), A.ERR_BAD_PARAM, "grid 1", {}),
            ("a first entry that wraps 32 bits", fmt(), grid(1, first_entry=0xFFFFFFFF), A.ERR_BAD_PARAM, "grid 1", {}),
            ("z outside every level", fmt(), grid(0, z=1), A.ERR_BAD_PARAM, "grid 0", {}),
            ("an infinite lod_bias", fmt(), grid(2, lod_bias=inf), A.ERR_BAD_PARAM, "grid 2", {}),
            ("a NaN lod_bias", fmt(), grid(0, lod_bias=float("nan")), A.ERR_BAD_PARAM, "grid 0", {}),
            ("a lod not aligned to 4 bytes", fmt(), grid(1, lod=lptr + 2), A.ERR_BAD_PARAM, "grid 1", {}),
            ("a lod_row_pitch below out_x", fmt(), grid(0, lod_row_pitch=29), A.ERR_BAD_PARAM, "grid 0", {}),
            ("a level above 65536 texels", fmt(), good, A.ERR_BAD_PARAM, "grid 1", dict(entry_list=entries[:n] + [huge_level])),
            # shared with the sample call
            ("an unknown filter", fmt(), good, A.ERR_BAD_PARAM, "filter", dict(sampler=A.LodSampler(2, 0, 0, 0))),
            ("an unknown address mode along x", fmt(), good, A.ERR_BAD_PARAM, "address", dict(sampler=A.LodSampler(1, 4, 0, 1))),
            ("an unknown address mode along y", fmt(), good, A.ERR_BAD_PARAM, "address", dict(sampler=A.LodSampler(0, 3, -1, 1))),
            ("a zero out_x", fmt(), grid(1, out_x=0), A.ERR_BAD_PARAM, "grid 1", {}),
            ("an out_y above 65535", fmt(), grid(0, out_y=65536), A.ERR_BAD_PARAM, "grid 0", {}),
            ("coordinates not aligned to 8 bytes", fmt(), grid(1, coords=cptr + 4), A.ERR_BAD_PARAM, grid_message(1, 3, "coords 0x... is not aligned to a pair of floats (8 bytes)"), {}),
            ("an odd coord_row_pitch", fmt(), grid(0, coord_row_pitch=81), A.ERR_BAD_PARAM, grid_message(0, 3, "coord_row_pitch 81: even and at least 60 floats"), {}),
            ("a coord_row_pitch below 2 out_x", fmt(), grid(0, coord_row_pitch=58), A.ERR_BAD_PARAM, grid_message(0, 3, "coord_row_pitch 58: even and at least 60 floats"), {}),
            ("null coordinates", fmt(), grid(2, coords=None), A.ERR_BAD_CONTEXT, grid_message(2, 3, "coords is null"), {}),
            ("a null format", None, good, A.ERR_BAD_PARAM, "format", {}),
            ("an unknown type", fmt(type=3), good, A.ERR_BAD_PARAM, "format", {}),
            ("five channels", fmt(channels=5), good, A.ERR_BAD_PARAM, "format", {}),
            ("an infinite scale", fmt(scale=(1.0, inf, 1.0, 1.0)), good, A.ERR_BAD_PARAM, "channel 1", {}),
            ("a row pitch below the output's", fmt(), grid(2, row_pitch=29), A.ERR_BAD_PARAM, "grid 2", {}),
            ("a plane pitch below the output's", fmt(), grid(1, plane_pitch=40 * 40 - 1), A.ERR_BAD_PARAM, "grid 1", {}),
            ("a plane pitch with the interleaved layout", fmt(layout=A.TENSOR_INTERLEAVED), grid(2, plane_pitch=1 << 20), A.ERR_BAD_PARAM, "grid 2", {}),
            ("an out that is not aligned to the element", fmt(), grid(1, out=out[1].data_ptr() + 1), A.ERR_BAD_PARAM, "grid 1", {}),
            ("a null out", fmt(), grid(2, out=None), A.ERR_BAD_CONTEXT, "grid 2", {}),
            ("an entry with an unknown data type", fmt(), good, A.ERR_BAD_PARAM, "entry 1", dict(entry_list=[entries[0], bad_entry] + entries[2:])),
        ]
        for what, f, grids, code, named, kw in cases:
            del logged[:]
            assert call(f, grids, **kw) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(log_names(named, m) for m in logged), (what, logged)
        # More work items than 32 bits hold: 64 grids of 65535 x 65535 points are 2^32 tiles, one too many, and the 64th is named.
        # (Every check runs before the launch: all grids point at the one small buffer, which must keep its guard.)
        huge = A.LodGrid(0, n, 0, 65535, 65535, cptr, 0, None, 0, 0.0, out[0].data_ptr(), 0, 0)
        assert S.tiles(65535, 65535) * 64 == 2 ** 32
        del logged[:]
        assert call(fmt(), [huge] * 64) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        assert any("grid 63 of 64" in m and "2^32" in m for m in logged), logged
        # a context whose footprint is 3D
        del logged[:]
        assert call(fmt(), good, context=contexts((3, 3, 3), A.PRF_LDR)) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all()) and any("3D" in m for m in logged), logged
        # coordinates and levels of detail are data: none of them is an error -- and the good call is good (a null lod included)
        assert call(fmt(), good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:, :64] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
