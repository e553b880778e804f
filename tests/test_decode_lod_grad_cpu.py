# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_lod_grad_device (the gradients of the level-of-detail sampler for coordinates and levels of detail): what can
be checked without a GPU.

  - the numpy model (tests/sample_lod_grad_model.py) on hand-made cases: a 2 x 2 texture with known differences, a texel centre,
    a NaN texel in a tap that is in no sum, CLAMP beyond the edge, BORDER across the edge, grad_lod at integer, clamped and
    MIP_NEAREST lambda and on a chain of one level, an invalid point, a sum in which a fused multiply-add changes the bits; the
    array form of the model against its pointwise form;
  - the model against central differences of the FORWARD model (sample_lod_model.sample_point), never against the library;
  - tests/harness/decode_lod_grad_check.cpp: the tile routine (decode_lod_grad.h) tile by tile from the host-built table against
    decode_row_batch of every whole level followed by the definition in plain C++, a stand-alone program under the address and
    undefined-behaviour sanitizers; nothing of it loads into Python;
  - the ctypes structure against the C one, the argument checks that need no context, lod_grad_grid on torch views;
  - the code object of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sample_lod_grad_model as G
import sample_lod_model as L
import sample_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_lod_grad_check.cpp")

# LDS of a workgroup of astc_lod_grad: what astc_lod_sample has -- DecodeBatch (7040 B) and the list of a batch's 32 block indices
LDS_BYTES = 7040 + 32 * 4
# two waves per SIMD: 512 registers / 2
VGPR_BOUND = 256

MODES = (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER)
MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)
ONE = np.array([1.0], dtype=np.float64)


def level(rows):
    """[H, W, 4] float32 whose component 0 is `rows` and whose other components are NaN: with one channel they are in no sum."""
    rows = np.asarray(rows, dtype=np.float32)
    t = np.full(rows.shape + (4,), np.nan, dtype=np.float32)
    t[..., 0] = rows
    return t


def at(chain, u, v, lod=0.0, filt=S.BILINEAR, ax=S.CLAMP, ay=S.CLAMP, mip=L.MIP_LINEAR, a=ONE, bias=0.0, want_lod=True):
    r = G.grad_point(chain, filt, ax, ay, mip, np.float32(u), np.float32(v), None if lod is None else np.float32(lod), bias, a, want_lod)
    return tuple(None if x is None else float(x) for x in r)


def positive_zero(x):
    return x == 0.0 and not np.signbit(np.float32(x))


def test_model_2x2_texture_with_known_differences():
    """Texels 1 2 / 4 8 (W = H = 2).  At (0.5, 0.5) -- x = y = 1, the corner of all four -- ix0 = iy0 = 0, f = 0.5 on both axes:
    ds/dx = 0.5 (2 - 1) + 0.5 (8 - 4) = 2.5 and ds/dy = 0.5 (4 - 1) + 0.5 (8 - 2) = 4.5 a texel, times W = H = 2 a unit of u, v."""
    chain = [level([[1, 2], [4, 8]])]
    assert at(chain, 0.5, 0.5) == (5.0, 9.0, 0.0)
    # a quarter of a texel to the left: ds/dy weighs the left column more, ds/dx is unchanged (bilinear: linear in x for fixed y)
    assert at(chain, 0.375, 0.5) == (5.0, 2 * (0.75 * 3 + 0.25 * 6), 0.0)
    # the upstream scales both; NEAREST has no coordinate gradient at all
    assert at(chain, 0.5, 0.5, a=np.array([-3.0])) == (-15.0, -27.0, 0.0)
    gu, gv, gl = at(chain, 0.5, 0.5, filt=S.NEAREST)
    assert positive_zero(gu) and positive_zero(gv) and positive_zero(gl)
    # two channels: the sum over c in order
    both = np.stack([np.array([[1, 2], [4, 8]], dtype=np.float32), np.array([[0, 10], [0, 10]], dtype=np.float32)] + [np.zeros((2, 2), dtype=np.float32)] * 2, axis=-1)
    assert at([both], 0.5, 0.5, a=np.array([1.0, 0.5])) == (5.0 + 0.5 * 20.0, 9.0, 0.0)


def test_model_texel_centre_takes_the_right_hand_difference_and_reads_the_neighbour():
    """(0.25, 0.25) is the centre of texel (0, 0) of a 2 x 2 level: f = 0 on both axes, the forward call reads that texel alone;
    the gradient is the difference to the right-hand (and lower) neighbour, which is read."""
    chain = [level([[1, 2], [4, 8]])]
    assert at(chain, 0.25, 0.25) == (2.0 * (2 - 1), 2.0 * (4 - 1), 0.0)
    # the centre of texel (1, 1): the neighbours are beyond the edge -- CLAMP repeats the texel, REPEAT wraps, BORDER is +0.0
    assert at(chain, 0.75, 0.75) == (0.0, 0.0, 0.0)
    assert at(chain, 0.75, 0.75, ax=S.REPEAT, ay=S.REPEAT) == (2.0 * (4 - 8), 2.0 * (2 - 8), 0.0)
    assert at(chain, 0.75, 0.75, ax=S.BORDER, ay=S.MIRROR) == (2.0 * (0 - 8), 0.0, 0.0)


def test_model_nan_texel_in_no_sum_does_not_reach_a_gradient():
    """f = 0 along y at (0.5, 0.25): dsdx uses row 0 alone and dsdy column taps (kx0, kx1) of both rows -- texel (1, 1) IS in
    dsdy; with f = 0 on both axes texel (1, 1) is in no sum."""
    nan = np.nan
    chain = [level([[1, 2], [4, nan]])]
    assert at(chain, 0.25, 0.25) == (2.0, 6.0, 0.0)
    gu, gv, _ = at(chain, 0.5, 0.25)
    assert gu == 2.0 and np.isnan(gv)
    # ... and a NaN in another channel than the format's is in no sum either (level() fills them with NaN)
    assert np.isnan(chain[0][0, 0, 1])
    # a NaN that does reach a gradient is stored as the canonical quiet NaN
    assert np.float32(gv).view(np.uint32) == 0x7FC00000
    gu, gv, _ = at(chain, 0.5, 0.25, a=np.array([-1.0]))
    assert np.float32(gv).view(np.uint32) == 0x7FC00000


def test_model_clamp_beyond_the_edge_and_border_across_it():
    chain = [level([[1, 2, 4, 8]])]                      # W = 4, H = 1
    # more than half a texel outside under CLAMP: both taps clamp to one texel -- +0.0, not -0.0
    for u in (-0.126, -0.5, 1.126, 3.0):
        gu, gv, _ = at(chain, u, 0.5)
        assert positive_zero(gu) and positive_zero(gv), u
    # less than half a texel outside the taps are texel 0 twice too (ix0 = -1 and 0 clamp to 0) ...
    assert at(chain, -0.05, 0.5)[0] == 0.0
    # ... and just inside the first cell boundary the difference is texel 1 - texel 0, times W
    assert at(chain, 0.2, 0.5)[0] == 4.0 * (2 - 1)
    # BORDER across the edge: the tap outside is +0.0 and is part of the difference
    assert at(chain, 0.05, 0.5, ax=S.BORDER)[0] == 4.0 * (1 - 0)
    assert at(chain, 1.05, 0.5, ax=S.BORDER)[0] == 4.0 * (0 - 8)
    assert at(chain, 1.3, 0.5, ax=S.BORDER)[0] == 0.0
    # along y there is one texel: CLAMP gives zero, BORDER sees the edge on either side of the centre
    gv = at(chain, 0.125, 0.75, ay=S.BORDER)[1]         # x at the centre of texel 0: wx = 1
    assert gv == -1.0 and at(chain, 0.125, 0.25, ay=S.BORDER)[1] == 1.0
    # REPEAT and MIRROR: the same formula on the addressed taps
    assert at(chain, 1.0, 0.5, ax=S.REPEAT)[0] == 4.0 * (1 - 8)
    assert at(chain, 1.0, 0.5, ax=S.MIRROR)[0] == 0.0


def one_texel_chain(values):
    return [level([[v]]) for v in values]


def test_model_grad_lod():
    chain = one_texel_chain([10.0, 20.0, 40.0, 30.0])
    for filt in (S.NEAREST, S.BILINEAR):
        # between levels: the difference of the two samples; at an integer lambda' the right derivative, from level l0 + 1
        assert at(chain, 0.5, 0.5, 0.25, filt)[2] == 10.0 and at(chain, 0.5, 0.5, 1.75, filt)[2] == 20.0
        assert at(chain, 0.5, 0.5, 0.0, filt)[2] == 10.0 and at(chain, 0.5, 0.5, 1.0, filt)[2] == 20.0 and at(chain, 0.5, 0.5, 2.0, filt)[2] == -10.0
        assert at(chain, 0.5, 0.5, -0.0, filt)[2] == 10.0
        assert at(chain, 0.5, 0.5, 1.0, filt, a=np.array([-0.5]))[2] == -10.0
        # lambda' = lod + lod_bias, one float32 addition; lod NULL: the bias alone
        assert at(chain, 0.5, 0.5, 0.75, filt, bias=0.5)[2] == 20.0 and at(chain, 0.5, 0.5, None, filt, bias=2.5)[2] == -10.0
        # clamped: below 0, at the top and beyond, the infinities
        for lam in (-1.0, -1e-30, 3.0, 3.5, 40.0, np.inf, -np.inf):
            assert positive_zero(at(chain, 0.5, 0.5, lam, filt)[2]), lam
        # MIP_NEAREST, a chain of one level, an invalid point
        for lam in (0.0, 0.25, 0.5, 1.0, 2.75):
            assert positive_zero(at(chain, 0.5, 0.5, lam, filt, mip=L.MIP_NEAREST)[2]), lam
            assert positive_zero(at(chain[:1], 0.5, 0.5, lam, filt)[2]), lam
        # grad_lod NULL: no third value
        assert at(chain, 0.5, 0.5, 1.0, filt, want_lod=False)[2] is None
    # a level of NaNs above an integer lambda': read for grad_lod (this case samples l0 + 1 for S alone), not for grad_coords,
    # and with grad_lod NULL not at all
    chain = [level([[1, 2]]), level([[np.nan]]), level([[5]])]
    gu, gv, gl = at(chain, 0.5, 0.5, 0.0)
    assert gu == 2.0 and gv == 0.0 and np.isnan(gl)
    assert at(chain, 0.5, 0.5, 0.0, want_lod=False) == (2.0, 0.0, None)
    assert at(chain, 0.5, 0.5, 2.0) == (0.0, 0.0, 0.0) and at(chain, 0.5, 0.5, 0.0, mip=L.MIP_NEAREST) == (2.0, 0.0, 0.0)


def test_model_blends_the_levels_coordinate_gradients():
    """Level 0 is 1 2 (W = 2), level 1 is one texel: at lambda' = 0.25 grad_u = 0.75 * 2 (2 - 1) + 0.25 * 0."""
    chain = [level([[1, 2]]), level([[7]])]
    assert at(chain, 0.5, 0.5, 0.25) == (1.5, 0.0, 7.0 - 1.5)
    assert at(chain, 0.5, 0.5, 0.25, mip=L.MIP_NEAREST) == (2.0, 0.0, 0.0)
    assert at(chain, 0.5, 0.5, 0.75, mip=L.MIP_NEAREST) == (0.0, 0.0, 0.0)


def test_model_invalid_point_gives_positive_zeros():
    chain = one_texel_chain([10.0, 20.0])
    big = np.nextafter(np.float32(2.0 ** 14), np.float32(np.inf))
    for u, v, lam in ((np.nan, 0.5, 0.5), (0.5, np.inf, 0.5), (big, 0.5, 0.5), (0.5, -big, 0.5), (0.5, 0.5, np.nan)):
        assert all(positive_zero(x) for x in at(chain, u, v, lam)), (u, v, lam)
    assert at(chain, 2.0 ** 14, -2.0 ** 14, 0.5)[2] == 10.0


def round_to_f32(q):
    """The binary32 nearest to the rational q (no tie among the candidates here)."""
    c = np.float32(float(q))
    best = min((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))), key=lambda f: abs(Fraction(float(f)) - q))
    return np.float32(best)


def test_model_sums_are_products_and_sums_never_fused():
    """S_0 = a0 s0 + a1 s1 + a2 s2 with e = 2^-23: a0 = (1 + e)(1 + 2e) (upstream times scale, exact), s0 = 1 + 6e: the product
    1 + 9e + 20e^2 + 12e^3 rounds to 1 + 9e + 20e^2; a1 s1 = -(1 + 4e)(1 + 5e) is exactly minus that, so the first sum is 0 --
    fused, the first product would keep its 12e^3 -- and a2 s2 = 2^-60 makes the result visible: grad_lod = S_1 - S_0 = -2^-60
    unfused, -(2^-60 + 12 2^-69) fused: another binary32."""
    e = 2.0 ** -23
    up = np.array([1 + e, -(1 + 4 * e), 2.0 ** -30], dtype=np.float32)
    scale = np.array([1 + 2 * e, 1.0, 1.0, 1.0], dtype=np.float32)
    a = G.upstream(up, scale)
    texel0 = np.array([1 + 6 * e, 1 + 5 * e, 2.0 ** -30, 0.0], dtype=np.float32)
    chain = [texel0.reshape(1, 1, 4), np.zeros((1, 1, 4), dtype=np.float32)]
    assert Fraction(float(a[0])) == Fraction(float(up[0])) * Fraction(float(scale[0]))                       # a[c] is exact
    exact0 = Fraction(float(a[0])) * Fraction(float(texel0[0]))
    assert Fraction(float(a[0]) * float(texel0[0])) != exact0                                               # the first product rounds
    assert Fraction(float(a[1]) * float(texel0[1])) == Fraction(float(a[1])) * Fraction(float(texel0[1]))    # the second does not
    assert float(a[0]) * float(texel0[0]) + float(a[1]) * float(texel0[1]) == 0.0
    got = np.float32(at(chain, 0.5, 0.5, 0.0, filt=S.NEAREST, a=a)[2])
    fused = round_to_f32(-(exact0 + Fraction(float(a[1])) * Fraction(float(texel0[1])) + Fraction(2.0 ** -60)))
    assert got == np.float32(-(2.0 ** -60)) and fused != got and fused == np.float32(-(2.0 ** -60 + 12 * 2.0 ** -69))
    gc, gl = G.grad(chain, S.NEAREST, S.CLAMP, S.CLAMP, L.MIP_LINEAR, [[[0.5, 0.5]]], np.zeros((1, 1), dtype=np.float32), 0.0, a[None, None])
    assert gl[0, 0] == got


def random_chain(seed, dims, kind):
    """Levels [H, W, 4] of the sizes `dims`: uint8, float16 (finite, with an infinity and a NaN) or float32; kind 3 mixes them."""
    rng = np.random.default_rng(seed)
    chain = []
    for l, (w, h) in enumerate(dims):
        k = l % 3 if kind == 3 else kind
        if k == 0:
            t = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        elif k == 1:
            t = rng.integers(0, 0x7C00, size=(h, w, 4), dtype=np.uint16).view(np.float16)
            t[h // 2, w // 3, 0] = np.inf
            t[h // 3, w // 2, 1] = np.nan
        else:
            t = rng.integers(0, 0x7F800000, size=(h, w, 4), dtype=np.uint32).view(np.float32)
        chain.append(t)
    return chain


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_model_array_form_is_the_pointwise_form():
    dims = L.chain_dims(17, 11)
    rng = np.random.default_rng(11)
    su, sl = L.special_coordinates(), L.special_lambdas(len(dims))
    grid = np.stack(np.meshgrid(su, su, indexing="xy"), axis=-1)
    grid_lod = sl[(np.arange(grid.shape[0])[:, None] * 7 + np.arange(grid.shape[1])[None, :]) % len(sl)]
    rand = rng.uniform(-0.25, 1.25, size=(9, 13, 2)).astype(np.float32)
    rand_lod = rng.uniform(-1.0, len(dims) + 0.5, size=(9, 13)).astype(np.float32)
    rand_lod[0, :5] = (0.0, 1.0, 2.0, 4.0, -0.0)
    for kind in (0, 1, 3):
        chain = random_chain(20 + kind, dims, kind)
        for filt in (S.NEAREST, S.BILINEAR):
            for mip in MIPS:
                for k, (ax, ay) in enumerate(((S.CLAMP, S.BORDER), (S.REPEAT, S.MIRROR), (S.MIRROR, S.REPEAT), (S.BORDER, S.CLAMP))):
                    for coords, lod, bias in ((grid, grid_lod, 0.0), (rand, rand_lod, 0.25), (rand, None, 1.5)):
                        channels = 1 + (k + filt + mip) % 4
                        up = rng.normal(size=coords.shape[:2] + (channels,)).astype(np.float32)
                        up[0, 0, 0], up[1, 1, channels - 1] = np.nan, np.inf
                        a = G.upstream(up, [0.5, -3.0, 1.0 / 255.0, 7.0])
                        for want_lod in (True, False):
                            gc, gl = G.grad(chain, filt, ax, ay, mip, coords, lod, bias, a, want_lod)
                            pc, pl = G.grad_pointwise(chain, filt, ax, ay, mip, coords, lod, bias, a, want_lod)
                            assert same_bits(gc, pc), (kind, filt, mip, ax, ay)
                            assert (gl is None and pl is None) if not want_lod else same_bits(gl, pl), (kind, filt, mip, ax, ay)


def loss(chain, sampler, u, v, lam, a):
    """sum over c of a[c] s[c] of the FORWARD model, in binary64."""
    s = L.sample_point(chain, sampler[0], sampler[1], sampler[2], sampler[3], np.float32(u), np.float32(v), np.float32(lam), 0.0)
    return float(np.sum(a * s[:len(a)].astype(np.float64)))


def test_model_agrees_with_central_differences_of_the_forward_model():
    """A random chain of 8-bit texels scaled to [0, 1], 24 x 20 texels; all four address modes, both filters' mip filters; 1600
    seeded points, (u, v) uniform in [-0.25, 1.25] on a grid of 2^-16 (so that u +- h is a binary32), lambda uniform in
    [-1, L + 0.5] on a grid of 2^-10.  Central differences of the forward model with h = 2^-12 in u and v and 2^-6 in lambda; a
    point is left out of a comparison where +-h crosses a texel-cell boundary (x - 0.5 an integer) on a level it uses, or a lambda
    at which its levels change -- there the forward is not linear between the two evaluations.  Bound: two binary32 roundings of
    texels in [0, 1] per evaluation (the level samples; 2^-24 each against sum |a[c]|), twofold margin: 4 * 2^-24 * sum |a[c]| / h,
    plus one binary32 ulp of the gradient.  Derived, not measured."""
    dims = L.chain_dims(24, 20)
    rng = np.random.default_rng(2024)
    chain = [(rng.integers(0, 256, size=(h, w, 4)).astype(np.float32) / np.float32(255.0)) for w, h in dims]
    n = len(chain)
    hu, hl = 2.0 ** -12, 2.0 ** -6
    points = 1600
    uv = (np.round(rng.uniform(-0.25, 1.25, size=(points, 2)) * 65536.0) / 65536.0).astype(np.float32)
    lam = (np.round(rng.uniform(-1.0, n + 0.5, size=points) * 1024.0) / 1024.0).astype(np.float32)
    up = rng.normal(size=(points, 3)).astype(np.float32)
    a_all = G.upstream(up, [1.0, 0.5, 2.0, 1.0])
    kept_uv = kept_lam = 0
    worst = worst_bound = 0.0

    def crosses_cell(x, h, size):
        return np.floor((x - h) * size - 0.5) != np.floor((x + h) * size - 0.5)

    for p in range(points):
        sampler = (S.BILINEAR, MODES[p % 4], MODES[(p // 4) % 4], MIPS[(p // 16) % 2])
        u, v, lm, a = float(uv[p, 0]), float(uv[p, 1]), float(lam[p]), a_all[p]
        assert float(np.float32(u + hu)) == u + hu and float(np.float32(u - hu)) == u - hu and float(np.float32(lm + hl)) == lm + hl
        gu, gv, gl = G.grad_point(chain, *sampler, np.float32(u), np.float32(v), np.float32(lm), 0.0, a)
        used = [l for l, _ in L.levels(sampler[3], n, np.float32(lm))]
        scale = 4.0 * 2.0 ** -24 * float(np.sum(np.abs(a)))
        if not any(crosses_cell(u, hu, dims[l][0]) or crosses_cell(v, hu, dims[l][1]) for l in used):
            kept_uv += 1
            for got, (du, dv) in ((gu, (hu, 0.0)), (gv, (0.0, hu))):
                fd = (loss(chain, sampler, u + du, v + dv, lm, a) - loss(chain, sampler, u - du, v - dv, lm, a)) / (2 * hu)
                bound = scale / hu + float(np.spacing(np.float32(abs(got))))
                worst, worst_bound = max(worst, abs(fd - float(got))), max(worst_bound, bound)
                assert abs(fd - float(got)) <= bound, (p, sampler, u, v, lm, fd, got, bound)
        # the levels change at the integers (MIP_LINEAR; the clamps at 0 and the top are among them) or halfway between (MIP_NEAREST)
        # -- asked of the model's own level rule, whose ties go to the finer level
        def piece(x):
            return L.levels(sampler[3], n, np.float32(x))[0][0], G.unclamped(sampler[3], n, np.float32(x))

        if piece(lm - hl) == piece(lm) == piece(lm + hl):
            kept_lam += 1
            fd = (loss(chain, sampler, u, v, lm + hl, a) - loss(chain, sampler, u, v, lm - hl, a)) / (2 * hl)
            bound = scale / hl + float(np.spacing(np.float32(abs(gl))))
            assert abs(fd - float(gl)) <= bound, (p, sampler, u, v, lm, fd, gl, bound)
    print("finite differences: kept %d of %d points for (u, v), %d for lambda; worst (u, v) error %.3g within a bound of at most %.3g" %
          (kept_uv, points, kept_lam, worst, worst_bound))
    # at most 5 % of the points are left out of either comparison
    assert kept_uv >= 0.95 * points and kept_lam >= 0.95 * points, (kept_uv, kept_lam)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_lod_grad") / "decode_lod_grad_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tile_routine_matches_the_definition_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # three footprints x two profiles x four chains (U8, F16, F32, mixed) x two mip filters x two filters x six formats
    assert int(re.search(r"^(\d+) configurations", out.stdout, re.M).group(1)) == 3 * 2 * 4 * 2 * 2 * 6
    assert "address mode pairs met: 16 of 16" in out.stdout
    # level l0 + 1 was read at weight zero, for grad_lod alone
    assert int(re.search(r"^points that read level l0 \+ 1 at weight zero: (\d+)$", out.stdout, re.M).group(1)) > 1000


def test_table_builder_on_a_hand_computed_case(harness):
    """6x6 blocks; entries 0 .. 2 a chain of 100 x 60 x 2, 50 x 30 x 2 and 25 x 15 x 2.  Grid 0: the three levels, 100 x 1 points (two
    64 x 1 tiles); grid 1: levels 1 and 2, 20 x 17 (three tiles across, three down), lod and grad_lod NULL.  The table: 16 bytes of
    head, first[2], padding to 32, two records, then 3 + 2 level records."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    head = re.match(r"table: bytes (\d+) levels_at (\d+) level_bytes (\d+) count (\d+) total (\d+) returned (\d+) first (\d+) (\d+) records (.*)$", out.stdout.strip())
    size, levels_at, level_bytes, count, total, returned, first0, first1 = (int(head.group(i)) for i in range(1, 9))
    assert (count, total, returned, first0, first1) == (2, 11, 11, 0, 2)
    assert (levels_at - 32) % 2 == 0 and size == levels_at + 5 * level_bytes
    fields = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(9))]
    assert fields[0] == dict(levels=levels_at, level_count=3, out_x=100, out_y=1, row=100, plane=100, has_up=1, has_gc=1, gc_row=202, has_gl=1, gl_row=101)
    assert fields[1] == dict(levels=levels_at + 3 * level_bytes, level_count=2, out_x=20, out_y=17, row=20, plane=340, has_up=1, has_gc=1, gc_row=40, has_gl=0, gl_row=20)


FIELDS = ["first_entry", "level_count", "z", "out_x", "out_y", "coords", "coord_row_pitch", "lod", "lod_row_pitch", "lod_bias", "grad_out", "row_pitch", "plane_pitch",
          "grad_coords", "grad_coord_row_pitch", "grad_lod", "grad_lod_row_pitch"]


def test_structure_is_the_c_one(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    assert [f for f, _ in A.LodGradGrid._fields_] == FIELDS
    body = '  printf("%zu", sizeof(astcenc_amd_lod_grad_grid));\n' + "".join('  printf(" %%zu", offsetof(astcenc_amd_lod_grad_grid, %s));\n' % f for f in FIELDS)
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(A.LodGradGrid)
    assert got[1:] == [getattr(A.LodGradGrid, f).offset for f in FIELDS]
    # the header compiles as C too
    if shutil.which("gcc"):
        c_probe = tmp_path / "probe.c"
        c_probe.write_text('#include "astcenc_amd.h"\nint main(void) { struct astcenc_amd_lod_grad_grid g; g.grad_lod = 0; return g.grad_lod != 0; }\n')
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c_probe), "-o", str(tmp_path / "probe_c")], check=True)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_lod_grad_device
    assert "astcenc_amd_sample_lod_grad_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_lod_grad_device) and callable(lib.sample_lod)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
    grid = (A.LodGradGrid * 1)(A.LodGradGrid(0, 1, 0, 2, 2, None, 0, None, 0, 0.0, None, 0, 0, None, 0, None, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_lod_grad_grid_from_views(A):
    torch = pytest.importorskip("torch")
    upstream = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((8, 40, 50, 2), dtype=torch.float32)
    lod = torch.zeros((8, 40, 50), dtype=torch.float32)
    gc, gl = torch.zeros_like(coords), torch.zeros_like(lod)
    g = A.lod_grad_grid(2, 7, 1, coords[3], lod[3], upstream[3], gc[3], gl[3], lod_bias=-0.5)
    assert (g.first_entry, g.level_count, g.z, g.out_x, g.out_y, g.lod_bias) == (2, 7, 1, 50, 40, -0.5)
    assert (g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.grad_out, g.row_pitch, g.plane_pitch) == \
        (coords[3].data_ptr(), 100, lod[3].data_ptr(), 50, upstream[3].data_ptr(), 50, 2000)
    assert (g.grad_coords, g.grad_coord_row_pitch, g.grad_lod, g.grad_lod_row_pitch) == (gc[3].data_ptr(), 100, gl[3].data_ptr(), 50)
    # a tile of all five; grad_lod not wanted
    cv, lv, uv, gcv, glv = coords[1, 4:14, 8:28], lod[1, 4:14, 8:28], upstream[1, :, 4:14, 8:28], gc[2, 4:14, 8:28], gl[2, 4:14, 8:28]
    g = A.lod_grad_grid(0, 1, 0, cv, lv, uv, gcv, glv)
    assert (g.out_x, g.out_y, g.grad_out, g.row_pitch, g.plane_pitch, g.grad_coords, g.grad_coord_row_pitch, g.grad_lod, g.grad_lod_row_pitch) == \
        (20, 10, uv.data_ptr(), 50, 2000, gcv.data_ptr(), 100, glv.data_ptr(), 50)
    g = A.lod_grad_grid(0, 3, 0, cv, None, uv, gcv, None, lod_bias=1.0)
    assert (g.lod, g.lod_row_pitch, g.grad_lod, g.grad_lod_row_pitch, g.lod_bias) == (None, 0, None, 0, 1.0)
    # [H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    g = A.lod_grad_grid(0, 2, 0, cv, lv, nhwc[2, 4:14, 8:28], gcv, glv, layout=A.TENSOR_INTERLEAVED, type=A.TENSOR_BF16)
    assert (g.out_x, g.out_y, g.row_pitch, g.plane_pitch) == (20, 10, 200, 0)
    # explicit pointers and pitches
    g = A.lod_grad_grid(1, 4, 3, (4096, 6, 7, 64), (12288, 8), (8192, 16, 9000), (16384, 14), (20480, 9), lod_bias=2.0)
    assert [getattr(g, f) for f in FIELDS] == [1, 4, 3, 6, 7, 4096, 64, 12288, 8, 2.0, 8192, 16, 9000, 16384, 14, 20480, 9]
    assert A.lod_grad_grid(1, 4, 3, (4096, 6, 7, 64), None, (8192, 16, 9000), (16384, 0)).grad_lod is None
    # what the call cannot express
    bad = [dict(gc=gc[3].double()), dict(gc=gc[3, :, :49]), dict(gc=gc[3, :39]), dict(gc=torch.zeros((40, 50, 3))[:, :, :2]),
           dict(gl=gl[3].half()), dict(gl=gl[3, :, :49]), dict(gl=torch.zeros((50, 40)).t()), dict(up=upstream[3, 0]), dict(up=upstream[3].float()),
           dict(level_count=0), dict(lod_bias=float("nan"))]
    for change in bad:
        kw = dict(level_count=3, gc=gc[3], gl=gl[3], up=upstream[3], lod_bias=0.0)
        kw.update(change)
        with pytest.raises(ValueError):
            A.lod_grad_grid(0, kw["level_count"], 0, coords[3], lod[3], kw["up"], kw["gc"], kw["gl"], lod_bias=kw["lod_bias"], type=A.TENSOR_F16)


def test_lod_grad_kernel_descriptors(built, A, tmp_path):
    """From the code object's metadata notes only: LDS is DecodeBatch + SampleTile, no scratch, registers for two waves per SIMD.
    profiles/decode_lod_grad/kernel_stats.txt holds the counts measured when the kernels were written."""
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    grad = {n: d for n, d in by_short.items() if n.startswith("astc_lod_grad")}
    # one build per tensor type and layout
    assert len(grad) == 6, sorted(by_short)
    for name, d in grad.items():
        assert d["group_segment_fixed_size"] == LDS_BYTES, (name, d)
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["vgpr_count"] <= VGPR_BOUND, (name, d)
    # ... and the lod call's kernels are still its six
    assert len([n for n in by_short if n.startswith("astc_lod_sample")]) == 6
