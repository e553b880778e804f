# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_volume_grad_device (the gradients of the volume sampler for coordinates and levels of detail): what can be
checked without a GPU.

  - the numpy model (tests/sample_volume_grad_model.py) on hand-made cases: a 2 x 2 x 2 volume with known differences along each
    axis, a texel centre on each axis alone, a NaN texel in a tap that is in no sum, CLAMP beyond the edge and BORDER across it on
    z as well as x, grad_lod at integer, clamped and MIP_NEAREST lambda, every kind of invalid point, a sum in which a fused
    multiply-add changes the bits; the array form of the model against its pointwise form;
  - the one-z-tap consequence: at slice centres du, dv and grad_lod are sample_lod_grad_model's for that slice, bit for bit;
  - the model against central differences of the FORWARD model (sample_volume_model.sample_point), never against the library;
  - tests/harness/decode_volume_grad_check.cpp: the tile routine (decode_volume_grad.h) tile by tile from the host-built table
    against decode_row_batch of every whole level followed by the definition in plain C++, a stand-alone program under the
    address and undefined-behaviour sanitizers; nothing of it loads into Python;
  - the ctypes structure against the C one, the argument checks that need no context, volume_grad_grid on torch views, the export;
  - the code object of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sample_lod_grad_model as G2
import sample_lod_model as L
import sample_model as S
import sample_volume_grad_model as G
import sample_volume_model as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_volume_grad_check.cpp")
HEADER = os.path.join(ROOT, "include", "astcenc_amd.h")

# LDS of a workgroup of astc_volume_grad: what astc_volume_sample has -- DecodeBatch (7040 B) and the list of a batch's 32 block indices
LDS_BYTES = 7040 + 32 * 4
# two waves per SIMD: 512 registers / 2
VGPR_BOUND = 256

MODES = (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER)
MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)
ONE = np.array([1.0], dtype=np.float64)
CLAMP3 = (S.CLAMP, S.CLAMP, S.CLAMP)


def level(values):
    """[D, H, W, 4] float32 whose component 0 is `values` and whose other components are NaN: with one channel they are in no sum."""
    values = np.asarray(values, dtype=np.float32)
    t = np.full(values.shape + (4,), np.nan, dtype=np.float32)
    t[..., 0] = values
    return t


def at(chain, u, v, w, lod=0.0, filt=S.BILINEAR, address=CLAMP3, mip=L.MIP_LINEAR, a=ONE, bias=0.0, want_lod=True):
    r = G.grad_point(chain, filt, address, mip, np.float32(u), np.float32(v), np.float32(w), None if lod is None else np.float32(lod), bias, a, want_lod)
    return tuple(None if x is None else float(x) for x in r)


def positive_zero(x):
    return x == 0.0 and not np.signbit(np.float32(x))


# z = 0: 1 2 / 4 8; z = 1: 16 32 / 64 128 (W = H = D = 2)
CUBE = [[[1, 2], [4, 8]], [[16, 32], [64, 128]]]


def test_model_2x2x2_volume_with_known_differences():
    """At (0.5, 0.5, 0.5) -- x = y = z = 1, the corner of all eight -- i0 = 0 and f = 0.5 on every axis:
    ds/dx = 0.5 (0.5 (2 - 1) + 0.5 (8 - 4)) + 0.5 (0.5 (32 - 16) + 0.5 (128 - 64)) = 21.25,
    ds/dy = 0.5 (0.5 (4 - 1) + 0.5 (8 - 2)) + 0.5 (0.5 (64 - 16) + 0.5 (128 - 32)) = 38.25,
    ds/dz = 0.5 (0.5 (16 - 1) + 0.5 (32 - 2)) + 0.5 (0.5 (64 - 4) + 0.5 (128 - 8)) = 56.25 a texel, times 2 a unit of u, v, w."""
    chain = [level(CUBE)]
    assert at(chain, 0.5, 0.5, 0.5) == (42.5, 76.5, 112.5, 0.0)
    # a quarter of a texel towards z = 0: ds/dx and ds/dy weigh slice 0 more, ds/dz is unchanged (linear in z for fixed x, y)
    assert at(chain, 0.5, 0.5, 0.375) == (2 * (0.75 * 2.5 + 0.25 * 40), 2 * (0.75 * 4.5 + 0.25 * 72), 112.5, 0.0)
    # the upstream scales all three; NEAREST has no coordinate gradient at all
    assert at(chain, 0.5, 0.5, 0.5, a=np.array([-2.0])) == (-85.0, -153.0, -225.0, 0.0)
    assert all(positive_zero(x) for x in at(chain, 0.5, 0.5, 0.5, filt=S.NEAREST))
    # two channels: the sum over c in order; the sizes differ per axis (W = 2, H = 1, D = 4: Dz is ds/dz times 4)
    t = np.zeros((4, 1, 2, 4), dtype=np.float32)
    t[..., 0] = np.array([1, 2], dtype=np.float32)[None, None, :]
    t[..., 1] = np.array([0, 10, 30, 70], dtype=np.float32)[:, None, None]
    assert at([t], 0.5, 0.5, 0.25, a=np.array([1.0, 0.5])) == (2.0 * 1.0, 0.0, 4.0 * 0.5 * 10.0, 0.0)


def test_model_texel_centre_on_each_axis_alone_takes_the_right_hand_difference():
    """u = 0.25 is the centre of texel 0 of an axis of 2: f = 0, the forward call has one tap there; the difference along that
    axis still runs to index 1, which is read, and the sums over that axis in the two other gradients have one term."""
    chain = [level(CUBE)]
    assert at(chain, 0.25, 0.5, 0.5)[:3] == (42.5, 2 * (0.5 * 3 + 0.5 * 48), 2 * (0.5 * 15 + 0.5 * 60))
    assert at(chain, 0.5, 0.25, 0.5)[:3] == (2 * (0.5 * 1 + 0.5 * 16), 76.5, 2 * (0.5 * 15 + 0.5 * 30))
    assert at(chain, 0.5, 0.5, 0.25)[:3] == (2 * (0.5 * 1 + 0.5 * 4), 2 * (0.5 * 3 + 0.5 * 6), 112.5)
    # all three at once: the three neighbours of texel (0, 0, 0)
    assert at(chain, 0.25, 0.25, 0.25)[:3] == (2.0 * (2 - 1), 2.0 * (4 - 1), 2.0 * (16 - 1))
    # the centre of texel (1, 1, 1): the neighbours are beyond the edge -- CLAMP repeats the texel, REPEAT wraps, BORDER is +0.0
    assert at(chain, 0.75, 0.75, 0.75)[:3] == (0.0, 0.0, 0.0)
    assert at(chain, 0.75, 0.75, 0.75, address=(S.REPEAT,) * 3)[:3] == (2.0 * (64 - 128), 2.0 * (32 - 128), 2.0 * (8 - 128))
    assert at(chain, 0.75, 0.75, 0.75, address=(S.BORDER, S.MIRROR, S.BORDER))[:3] == (2.0 * (0 - 128), 0.0, 2.0 * (0 - 128))


def test_model_nan_texel_in_no_sum_does_not_reach_a_gradient():
    """nx = ny = nz = 1 at (0.25, 0.25, 0.25): every difference starts at texel (0, 0, 0) and runs along one axis; texel
    (kx1, ky1, kz1) = (1, 1, 1) is in no sum.  With two taps on any axis it is."""
    cube = np.array(CUBE, dtype=np.float32)
    cube[1, 1, 1] = np.nan
    chain = [level(cube)]
    assert at(chain, 0.25, 0.25, 0.25) == (2.0, 6.0, 30.0, 0.0)
    gu, gv, gw, _ = at(chain, 0.25, 0.25, 0.5)          # two z taps: dsdx and dsdy take slice 1's rows (0, *, 1) and (*, 0, 1): still not (1, 1, 1)
    assert (gu, gv, gw) == (2 * (0.5 * 1 + 0.5 * 16), 2 * (0.5 * 3 + 0.5 * 48), 30.0)
    gu, gv, gw, _ = at(chain, 0.25, 0.5, 0.5)           # two y taps and two z taps: d(ky1, kz1) holds it
    assert np.isnan(gu) and gv == 2 * (0.5 * 3 + 0.5 * 48) and gw == 2 * (0.5 * 15 + 0.5 * 60)
    # a NaN in another channel than the format's is in no sum either (level() fills them with NaN) ...
    assert np.isnan(chain[0][0, 0, 0, 1])
    # ... and a NaN that does reach a gradient is stored as the canonical quiet NaN, whatever its sign
    for a in (ONE, -ONE):
        assert np.float32(at(chain, 0.25, 0.5, 0.5, a=a)[0]).view(np.uint32) == 0x7FC00000


def test_model_clamp_beyond_the_edge_and_border_across_it_on_x_and_z():
    """v(kx, 0, kz) = A[kx] + B[kz] with A = 1 2 4 8 and B = 0 16 48 112: W = D = 4, H = 1."""
    A, B = np.array([1, 2, 4, 8], dtype=np.float32), np.array([0, 16, 48, 112], dtype=np.float32)
    chain = [level(A[None, None, :] + B[:, None, None])]
    # more than half a texel outside under CLAMP: both taps clamp to one texel -- +0.0, not -0.0 -- along that axis alone
    for c in (-0.126, -0.5, 1.126, 3.0):
        gu, gv, gw, _ = at(chain, c, 0.5, 0.1875)
        assert positive_zero(gu) and positive_zero(gv) and gw == 4.0 * 16, c
        gu, gv, gw, _ = at(chain, 0.1875, 0.5, c)
        assert gu == 4.0 * 1 and positive_zero(gv) and positive_zero(gw), c
    # u = 0.1875: x = 0.75, taps 0 and 1 with weights 0.75 and 0.25; w = 0.125: the centre of slice 0
    assert at(chain, 0.1875, 0.5, 0.125)[:3] == (4.0 * 1, 0.0, 4.0 * 16)
    # BORDER across the lower edge of z (w = 0.0625: taps -1 and 0): the tap outside is +0.0 and is part of the difference
    border_z = (S.CLAMP, S.CLAMP, S.BORDER)
    assert at(chain, 0.1875, 0.5, 0.0625, address=border_z)[2] == 4.0 * (0.75 * 1 + 0.25 * 2)
    # ... across the upper edge (w = 1.0625: taps 3 and 4), and with both taps outside
    assert at(chain, 0.1875, 0.5, 1.0625, address=border_z)[2] == -4.0 * (0.75 * 113 + 0.25 * 114)
    assert positive_zero(at(chain, 0.1875, 0.5, 1.5, address=border_z)[2])
    # a BORDER tap outside on z makes the whole tap +0.0: the x difference of that plane is 0 - 0
    assert at(chain, 0.1875, 0.5, 0.0625, address=border_z)[0] == 4.0 * (0.25 * 0 + 0.75 * 1)
    # the same across x
    border_x = (S.BORDER, S.CLAMP, S.CLAMP)
    assert at(chain, 0.0625, 0.5, 0.125, address=border_x)[0] == 4.0 * (1 - 0)
    assert at(chain, 1.0625, 0.5, 0.125, address=border_x)[0] == 4.0 * (0 - 8)
    assert positive_zero(at(chain, 1.5, 0.5, 0.125, address=border_x)[0])
    # REPEAT and MIRROR along z: the same formula on the addressed taps (w = 1: taps 3 and 4 -> 0, or 3)
    assert at(chain, 0.1875, 0.5, 1.0, address=(S.CLAMP, S.CLAMP, S.REPEAT))[2] == 4.0 * (0 - 112)
    assert at(chain, 0.1875, 0.5, 1.0, address=(S.CLAMP, S.CLAMP, S.MIRROR))[2] == 0.0


def one_texel_chain(values):
    return [level([[[v]]]) for v in values]


def test_model_grad_lod():
    chain = one_texel_chain([10.0, 20.0, 40.0, 30.0])
    for filt in (S.NEAREST, S.BILINEAR):
        # between levels: the difference of the two samples; at an integer lambda' the right derivative, from level l0 + 1
        assert at(chain, 0.5, 0.5, 0.5, 0.25, filt)[3] == 10.0 and at(chain, 0.5, 0.5, 0.5, 1.75, filt)[3] == 20.0
        assert [at(chain, 0.5, 0.5, 0.5, lam, filt)[3] for lam in (0.0, -0.0, 1.0, 2.0)] == [10.0, 10.0, 20.0, -10.0]
        assert at(chain, 0.5, 0.5, 0.5, 1.0, filt, a=np.array([-0.5]))[3] == -10.0
        # lambda' = lod + lod_bias, one float32 addition; lod NULL: the bias alone
        assert at(chain, 0.5, 0.5, 0.5, 0.75, filt, bias=0.5)[3] == 20.0 and at(chain, 0.5, 0.5, 0.5, None, filt, bias=2.5)[3] == -10.0
        # clamped: below 0, at the top and beyond, the infinities
        for lam in (-1.0, -1e-30, 3.0, 3.5, 40.0, np.inf, -np.inf):
            assert positive_zero(at(chain, 0.5, 0.5, 0.5, lam, filt)[3]), lam
        # MIP_NEAREST, a chain of one level
        for lam in (0.0, 0.25, 0.5, 1.0, 2.75):
            assert positive_zero(at(chain, 0.5, 0.5, 0.5, lam, filt, mip=L.MIP_NEAREST)[3]), lam
            assert positive_zero(at(chain[:1], 0.5, 0.5, 0.5, lam, filt)[3]), lam
        # grad_lod NULL: no fourth value
        assert at(chain, 0.5, 0.5, 0.5, 1.0, filt, want_lod=False)[3] is None
    # a level of NaNs above an integer lambda': read for grad_lod (this case samples l0 + 1 for S alone), not for grad_coords,
    # and with grad_lod NULL not at all
    chain = [level([[[1, 2]]]), level([[[np.nan]]]), level([[[5]]])]
    r = at(chain, 0.5, 0.5, 0.5, 0.0)
    assert r[:3] == (2.0, 0.0, 0.0) and np.isnan(r[3])
    assert at(chain, 0.5, 0.5, 0.5, 0.0, want_lod=False) == (2.0, 0.0, 0.0, None)
    assert at(chain, 0.5, 0.5, 0.5, 2.0) == (0.0, 0.0, 0.0, 0.0) and at(chain, 0.5, 0.5, 0.5, 0.0, mip=L.MIP_NEAREST) == (2.0, 0.0, 0.0, 0.0)
    # two levels blend all three coordinate gradients: level 0 is the cube, level 1 one texel; lambda' = 0.25
    chain = [level(CUBE), level([[[7]]])]
    s0 = float(V.sample_point(chain[:1], S.BILINEAR, CLAMP3, L.MIP_NEAREST, 0.5, 0.5, 0.5, None, 0.0)[0])
    assert at(chain, 0.5, 0.5, 0.5, 0.25) == (0.75 * 42.5, 0.75 * 76.5, 0.75 * 112.5, 7.0 - s0)


def test_model_invalid_point_gives_positive_zeros():
    chain = one_texel_chain([10.0, 20.0])
    big = np.nextafter(np.float32(2.0 ** 14), np.float32(np.inf))
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf, big, -big):
            p = [0.5, 0.5, 0.5]
            p[axis] = bad
            assert all(positive_zero(x) for x in at(chain, p[0], p[1], p[2], 0.5)), (axis, bad)
    assert all(positive_zero(x) for x in at(chain, 0.5, 0.5, 0.5, np.nan))
    # 2^14 itself is valid on every axis
    assert at(chain, 2.0 ** 14, -2.0 ** 14, 2.0 ** 14, 0.5)[3] == 10.0


def round_to_f32(q):
    """The binary32 nearest to the rational q (no tie among the candidates here)."""
    c = np.float32(float(q))
    best = min((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))), key=lambda f: abs(Fraction(float(f)) - q))
    return np.float32(best)


def test_model_sums_are_products_and_sums_never_fused():
    """tests/test_decode_lod_grad_cpu.py's case on a volume of one texel: S_0 = a0 s0 + a1 s1 + a2 s2 with e = 2^-23,
    a0 = (1 + e)(1 + 2e), s0 = 1 + 6e: the product rounds to 1 + 9e + 20e^2; a1 s1 = -(1 + 4e)(1 + 5e) is exactly minus that, so the
    first sum is 0 -- fused, the first product would keep its 12e^3 -- and a2 s2 = 2^-60 makes the result visible."""
    e = 2.0 ** -23
    up = np.array([1 + e, -(1 + 4 * e), 2.0 ** -30], dtype=np.float32)
    scale = np.array([1 + 2 * e, 1.0, 1.0, 1.0], dtype=np.float32)
    a = G.upstream(up, scale)
    texel0 = np.array([1 + 6 * e, 1 + 5 * e, 2.0 ** -30, 0.0], dtype=np.float32)
    chain = [texel0.reshape(1, 1, 1, 4), np.zeros((1, 1, 1, 4), dtype=np.float32)]
    exact0 = Fraction(float(a[0])) * Fraction(float(texel0[0]))
    assert Fraction(float(a[0]) * float(texel0[0])) != exact0                                               # the first product rounds
    assert float(a[0]) * float(texel0[0]) + float(a[1]) * float(texel0[1]) == 0.0
    got = np.float32(at(chain, 0.5, 0.5, 0.5, 0.0, filt=S.NEAREST, a=a)[3])
    fused = round_to_f32(-(exact0 + Fraction(float(a[1])) * Fraction(float(texel0[1])) + Fraction(2.0 ** -60)))
    assert got == np.float32(-(2.0 ** -60)) and fused != got and fused == np.float32(-(2.0 ** -60 + 12 * 2.0 ** -69))
    gc, gl = G.grad(chain, S.NEAREST, CLAMP3, L.MIP_LINEAR, [[[0.5, 0.5, 0.5]]], np.zeros((1, 1), dtype=np.float32), 0.0, a[None, None])
    assert gl[0, 0] == got
    # ... and a difference sum: wy0 d0 + wy1 d1 with wy0 d0 inexact and wy1 d1 its exact negative would differ fused; here the
    # cheaper statement: the array form and the pointwise form agree on random data below, and numpy never fuses


def random_chain(seed, dims, kind):
    """Levels [D, H, W, 4] of the sizes `dims` (W, H, D): uint8, float16 (finite, with an infinity and a NaN) or float32; kind 3 mixes them."""
    rng = np.random.default_rng(seed)
    chain = []
    for l, (w, h, d) in enumerate(dims):
        k = l % 3 if kind == 3 else kind
        if k == 0:
            t = rng.integers(0, 256, size=(d, h, w, 4), dtype=np.uint8)
        elif k == 1:
            t = rng.integers(0, 0x7C00, size=(d, h, w, 4), dtype=np.uint16).view(np.float16)
            t[d // 2, h // 2, w // 3, 0] = np.inf
            t[d // 3, h // 3, w // 2, 1] = np.nan
        else:
            t = rng.integers(0, 0x7F800000, size=(d, h, w, 4), dtype=np.uint32).view(np.float32)
        chain.append(t)
    return chain


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_model_array_form_is_the_pointwise_form():
    dims = V.CHAIN
    rng = np.random.default_rng(11)
    su, sl = L.special_coordinates(), L.special_lambdas(len(dims))
    # every special value against every other on two axes, the third turning through the list
    n = len(su)
    grid = np.empty((n, n, 3), dtype=np.float32)
    grid[..., 0], grid[..., 1] = su[None, :], su[:, None]
    grid[..., 2] = su[(np.arange(n)[:, None] * 3 + np.arange(n)[None, :] * 5) % n]
    grid_lod = sl[(np.arange(n)[:, None] * 7 + np.arange(n)[None, :]) % len(sl)]
    rand = rng.uniform(-0.25, 1.25, size=(7, 11, 3)).astype(np.float32)
    rand[0, :3] = V.constructed_points((3, 3, 3))[:3]
    rand_lod = rng.uniform(-1.0, len(dims) + 0.5, size=(7, 11)).astype(np.float32)
    rand_lod[0, :5] = (0.0, 1.0, 2.0, 4.0, -0.0)
    turn = 0
    for kind in (0, 1, 3):
        chain = random_chain(20 + kind, dims, kind)
        for filt in (S.NEAREST, S.BILINEAR):
            for mip in MIPS:
                for coords, lod, bias in ((grid, grid_lod, 0.0), (rand, rand_lod, 0.25), (rand, None, 1.5)):
                    address = (MODES[turn % 4], MODES[(turn // 4 + turn) % 4], MODES[(turn // 2 + 1) % 4])
                    channels = 1 + turn % 4
                    turn += 1
                    up = rng.normal(size=coords.shape[:2] + (channels,)).astype(np.float32)
                    up[0, 0, 0], up[1, 1, channels - 1] = np.nan, np.inf
                    a = G.upstream(up, [0.5, -3.0, 1.0 / 255.0, 7.0])
                    for want_lod in (True, False):
                        gc, gl = G.grad(chain, filt, address, mip, coords, lod, bias, a, want_lod)
                        pc, pl = G.grad_pointwise(chain, filt, address, mip, coords, lod, bias, a, want_lod)
                        assert same_bits(gc, pc), (kind, filt, mip, address)
                        assert (gl is None and pl is None) if not want_lod else same_bits(gl, pl), (kind, filt, mip, address)


def test_model_one_z_tap_is_the_lod_gradient_for_that_slice():
    """A chain whose levels all have depth 4: w = (kz + 0.5) / 4 is the centre of slice kz in every level, the z axis has one tap of
    weight exactly 1.0 and 1.0 * q is q: du, dv and grad_lod are sample_lod_grad_model's for z = kz, bit for bit, under either
    filter; dw is the difference towards slice kz + 1 as addressed, D times sum a[c] (s_(kz+1)[c] - s_kz[c]) up to the level
    samples' own rounding."""
    dims = [(12, 10, 4), (6, 5, 4), (3, 2, 4)]
    rng = np.random.default_rng(5)
    chain = [rng.uniform(-4, 4, size=(d, h, w, 4)).astype(np.float32) for w, h, d in dims]
    uv = rng.uniform(-0.3, 1.3, size=(6, 9, 2)).astype(np.float32)
    lod = V.seeded_lods(rng, (6, 9), 3)
    up = rng.normal(size=(6, 9, 3)).astype(np.float32)
    a = G.upstream(up, [0.5, -3.0, 2.0, 1.0])
    turn = 0
    for kz in range(4):
        coords = np.concatenate([uv, np.full((6, 9, 1), (kz + 0.5) / 4, dtype=np.float32)], axis=-1)
        slices = [t[kz] for t in chain]
        for filt in (S.NEAREST, S.BILINEAR):
            for mip in MIPS:
                ax, ay, az = MODES[turn % 4], MODES[(turn // 4 + turn + 1) % 4], MODES[(turn + 2) % 4]
                turn += 1
                for want_lod in (True, False):
                    gc, gl = G.grad(chain, filt, (ax, ay, az), mip, coords, lod, 0.25, a, want_lod)
                    rc, rl = G2.grad(slices, filt, ax, ay, mip, uv, lod, 0.25, a, want_lod)
                    assert same_bits(gc[..., :2], rc), (kz, filt, mip, ax, ay, az)
                    assert (gl is None and rl is None) if not want_lod else same_bits(gl, rl)
                if filt == S.NEAREST:
                    assert not gc[..., 2].any()
                    continue
                # dw under MIP_NEAREST: one level, so the z difference of that level's two slice samples
                if mip != L.MIP_NEAREST:
                    continue
                ok, l0, _, _ = V.level_arrays(mip, 3, coords, lod, 0.25)
                for l, t in enumerate(chain):
                    k1 = S.address(az, kz + 1, 4)
                    s0 = L.level_sample(t[kz], filt, ax, ay, uv).astype(np.float64)[..., :3]
                    s1 = np.zeros_like(s0) if k1 is None else L.level_sample(t[k1], filt, ax, ay, uv).astype(np.float64)[..., :3]
                    want = 4.0 * np.sum(a * (s1 - s0), axis=-1)
                    pick = ok & (l0 == l)
                    assert pick.any()
                    assert np.allclose(gc[..., 2][pick], want[pick], rtol=0, atol=4.0 * 3 * 2.0 ** -21 * np.abs(a).sum(axis=-1).max()), (kz, l)


def loss(chain, sampler, p, lam, a):
    """sum over c of a[c] s[c] of the FORWARD model, in binary64."""
    s = V.sample_point(chain, sampler[0], sampler[1], sampler[2], np.float32(p[0]), np.float32(p[1]), np.float32(p[2]), np.float32(lam), 0.0)
    return float(np.sum(a * s[:len(a)].astype(np.float64)))


def test_model_agrees_with_central_differences_of_the_forward_model():
    """A random chain of 8-bit texels scaled to [0, 1], 20 x 14 x 9 texels (sample_volume_model.CHAIN); the address modes turning
    per axis, both mip filters; 1600 seeded points, (u, v, w) uniform in [-0.25, 1.25] on a grid of 2^-16 (so that u +- h is a
    binary32), lambda uniform in [-1, L + 0.5] on a grid of 2^-10.  Central differences of the forward model with h = 2^-13 in u,
    v and w and 2^-6 in lambda; a point is left out of a comparison only where +-h crosses a texel-cell boundary (x - 0.5 an
    integer) on a level it uses, or where its levels change -- there the forward is not linear between the two evaluations.
    Condition: at least 95 % of the points are kept in either comparison (expected loss about 2 h (20 + 14 + 9) 1.5 = 1.6 %).
    Bound: two binary32 roundings of texels in [0, 1] per evaluation (the level samples; 2^-24 each against sum |a[c]|), twofold
    margin: 4 * 2^-24 * sum |a[c]| / h, plus one binary32 ulp of the gradient.  Derived, not measured."""
    dims = V.CHAIN
    assert dims[0] == (20, 14, 9)
    rng = np.random.default_rng(2025)
    chain = [(rng.integers(0, 256, size=(d, h, w, 4)).astype(np.float32) / np.float32(255.0)) for w, h, d in dims]
    n = len(chain)
    hu, hl = 2.0 ** -13, 2.0 ** -6
    points = 1600
    uvw = (np.round(rng.uniform(-0.25, 1.25, size=(points, 3)) * 65536.0) / 65536.0).astype(np.float32)
    lam = (np.round(rng.uniform(-1.0, n + 0.5, size=points) * 1024.0) / 1024.0).astype(np.float32)
    up = rng.normal(size=(points, 3)).astype(np.float32)
    a_all = G.upstream(up, [1.0, 0.5, 2.0, 1.0])
    kept_uvw = kept_lam = 0
    worst = worst_bound = worst_lam = worst_lam_bound = 0.0

    def crosses_cell(x, h, size):
        return np.floor((x - h) * size - 0.5) != np.floor((x + h) * size - 0.5)

    for p in range(points):
        address = (MODES[p % 4], MODES[(p // 4) % 4], MODES[(p // 16) % 4])
        sampler = (S.BILINEAR, address, MIPS[(p // 64) % 2])
        c, lm, a = [float(x) for x in uvw[p]], float(lam[p]), a_all[p]
        assert all(float(np.float32(x + hu)) == x + hu and float(np.float32(x - hu)) == x - hu for x in c) and float(np.float32(lm + hl)) == lm + hl
        g = G.grad_point(chain, sampler[0], sampler[1], sampler[2], np.float32(c[0]), np.float32(c[1]), np.float32(c[2]), np.float32(lm), 0.0, a)
        used = [l for l, _ in L.levels(sampler[2], n, np.float32(lm))]
        scale = 4.0 * 2.0 ** -24 * float(np.sum(np.abs(a)))
        if not any(crosses_cell(c[axis], hu, dims[l][axis]) for l in used for axis in range(3)):
            kept_uvw += 1
            for axis in range(3):
                hi, lo = list(c), list(c)
                hi[axis] += hu
                lo[axis] -= hu
                fd = (loss(chain, sampler, hi, lm, a) - loss(chain, sampler, lo, lm, a)) / (2 * hu)
                bound = scale / hu + float(np.spacing(np.float32(abs(g[axis]))))
                if abs(fd - float(g[axis])) > worst:
                    worst, worst_bound = abs(fd - float(g[axis])), bound
                assert abs(fd - float(g[axis])) <= bound, (p, sampler, c, lm, axis, fd, g[axis], bound)

        # the levels change at the integers (MIP_LINEAR; the clamps at 0 and the top are among them) or halfway between (MIP_NEAREST)
        # -- asked of the model's own level rule, whose ties go to the finer level
        def piece(x):
            return L.levels(sampler[2], n, np.float32(x))[0][0], G.unclamped(sampler[2], n, np.float32(x))

        if piece(lm - hl) == piece(lm) == piece(lm + hl):
            kept_lam += 1
            fd = (loss(chain, sampler, c, lm + hl, a) - loss(chain, sampler, c, lm - hl, a)) / (2 * hl)
            bound = scale / hl + float(np.spacing(np.float32(abs(g[3]))))
            if abs(fd - float(g[3])) > worst_lam:
                worst_lam, worst_lam_bound = abs(fd - float(g[3])), bound
            assert abs(fd - float(g[3])) <= bound, (p, sampler, c, lm, fd, g[3], bound)
    print("finite differences: kept %d of %d points for (u, v, w), %d for lambda; worst (u, v, w) error %.3g within its bound %.3g; worst lambda error %.3g within %.3g" %
          (kept_uvw, points, kept_lam, worst, worst_bound, worst_lam, worst_lam_bound))
    # at most 5 % of the points are left out of either comparison: a condition on the test's inputs, not a measurement
    assert kept_uvw >= 0.95 * points and kept_lam >= 0.95 * points, (kept_uvw, kept_lam)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_volume_grad") / "decode_volume_grad_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tile_routine_matches_the_definition_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # three footprints (4x4, 3x3x3, 5x5x4) x four chains (U8, F16, F32, mixed) x two mip filters x two filters x six formats
    assert int(re.search(r"^(\d+) configurations", out.stdout, re.M).group(1)) == 3 * 4 * 2 * 2 * 6
    assert "address mode triples met: 64 of 64" in out.stdout
    # 64 x 1, 32 x 2, 16 x 4 and 8 x 8 points
    assert int(re.search(r"^tile shapes met: (\d+)$", out.stdout, re.M).group(1)) >= 3
    # level l0 + 1 was read at weight zero, for grad_lod alone (the harness itself compares every tile's passes with the levels
    # its points need, with and without grad_lod)
    assert int(re.search(r"^points that read level l0 \+ 1 at weight zero: (\d+)$", out.stdout, re.M).group(1)) > 1000


def test_table_builder_on_a_hand_computed_case(harness):
    """4x4x3 blocks; entries 0 .. 2 a chain of 100 x 60 x 20, 50 x 30 x 10 and 25 x 15 x 5.  Grid 0: the three levels, 100 x 1 points
    (two 64 x 1 tiles); grid 1: levels 1 and 2, 20 x 17 (three tiles across, three down), lod and grad_lod NULL.  The table: 16
    bytes of head, first[2], padding to 32, two records, then 3 + 2 level records.  The sampler is BILINEAR, BORDER / REPEAT /
    MIRROR, MIP_LINEAR."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    head = re.match(r"table: bytes (\d+) levels_at (\d+) level_bytes (\d+) count (\d+) total (\d+) returned (\d+) first (\d+) (\d+) records (.*)$", out.stdout.strip())
    size, levels_at, level_bytes, count, total, returned, first0, first1 = (int(head.group(i)) for i in range(1, 9))
    assert (count, total, returned, first0, first1) == (2, 11, 11, 0, 2)
    assert (levels_at - 32) % 2 == 0 and size == levels_at + 5 * level_bytes
    fields = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(9))]
    common = dict(has_up=1, has_uvw=1, address_x=3, address_y=1, address_z=2, filter=1, mip=1, has_gc=1)
    assert fields[0] == dict(common, levels=levels_at, level_count=3, out_x=100, out_y=1, row=100, plane=100, uvw_row=300, tw_log2=6, tiles_x=2, level0_z=20, gc_row=301,
                             has_gl=1, gl_row=101)
    assert fields[1] == dict(common, levels=levels_at + 3 * level_bytes, level_count=2, out_x=20, out_y=17, row=20, plane=340, uvw_row=60, tw_log2=3, tiles_x=3, level0_z=10,
                             gc_row=60, has_gl=0, gl_row=20)


FIELDS = ["first_entry", "level_count", "out_x", "out_y", "coords", "coord_row_pitch", "lod", "lod_row_pitch", "lod_bias", "grad_out", "row_pitch", "plane_pitch",
          "grad_coords", "grad_coord_row_pitch", "grad_lod", "grad_lod_row_pitch"]


def test_structure_is_the_c_one(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    assert [f for f, _ in A.VolumeGradGrid._fields_] == FIELDS
    body = '  printf("%zu", sizeof(astcenc_amd_volume_grad_grid));\n' + "".join('  printf(" %%zu", offsetof(astcenc_amd_volume_grad_grid, %s));\n' % f for f in FIELDS)
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body + '  printf("\\n");\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(A.VolumeGradGrid)
    assert got[1:] == [getattr(A.VolumeGradGrid, f).offset for f in FIELDS]
    # the header compiles as C too, and the C structure has the same size
    if shutil.which("gcc"):
        c_probe = tmp_path / "probe.c"
        c_probe.write_text('#include "astcenc_amd.h"\n#include <stdio.h>\nint main(void) { struct astcenc_amd_volume_grad_grid g; g.grad_lod = 0; '
                           'printf("%zu\\n", sizeof g); return g.grad_lod != 0; }\n')
        c_exe = str(tmp_path / "probe_c")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c_probe), "-o", c_exe], check=True)
        assert int(subprocess.run([c_exe], capture_output=True, text=True, check=True).stdout) == C.sizeof(A.VolumeGradGrid)


def test_export_is_in_the_binding_and_in_the_header(A):
    name = "astcenc_amd_sample_volume_grad_device"
    assert name in A.EXPORTS_AMD
    text = open(HEADER).read()
    assert re.search(r"ASTCENC_PUBLIC enum astcenc_error %s\(" % name, text)
    # the two comments that called this out of scope point here
    assert text.count(name) >= 3
    assert "the cube and volume samplers" not in text


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_volume_grad_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_volume_grad) and callable(lib.sample_volume)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.VolumeSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
    grid = (A.VolumeGradGrid * 1)(A.VolumeGradGrid(0, 1, 2, 2, None, 0, None, 0, 0.0, None, 0, 0, None, 0, None, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_volume_grad_grid_from_views(A):
    torch = pytest.importorskip("torch")
    upstream = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((8, 40, 50, 3), dtype=torch.float32)
    lod = torch.zeros((8, 40, 50), dtype=torch.float32)
    gc, gl = torch.zeros_like(coords), torch.zeros_like(lod)
    g = A.volume_grad_grid(2, 7, coords[3], lod[3], upstream[3], gc[3], gl[3], lod_bias=-0.5)
    assert (g.first_entry, g.level_count, g.out_x, g.out_y, g.lod_bias) == (2, 7, 50, 40, -0.5)
    assert (g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.grad_out, g.row_pitch, g.plane_pitch) == \
        (coords[3].data_ptr(), 150, lod[3].data_ptr(), 50, upstream[3].data_ptr(), 50, 2000)
    assert (g.grad_coords, g.grad_coord_row_pitch, g.grad_lod, g.grad_lod_row_pitch) == (gc[3].data_ptr(), 150, gl[3].data_ptr(), 50)
    # a tile of all five; grad_lod not wanted
    cv, lv, uv, gcv, glv = coords[1, 4:14, 8:28], lod[1, 4:14, 8:28], upstream[1, :, 4:14, 8:28], gc[2, 4:14, 8:28], gl[2, 4:14, 8:28]
    g = A.volume_grad_grid(0, 1, cv, lv, uv, gcv, glv)
    assert (g.out_x, g.out_y, g.grad_out, g.row_pitch, g.plane_pitch, g.grad_coords, g.grad_coord_row_pitch, g.grad_lod, g.grad_lod_row_pitch) == \
        (20, 10, uv.data_ptr(), 50, 2000, gcv.data_ptr(), 150, glv.data_ptr(), 50)
    g = A.volume_grad_grid(0, 3, cv, None, uv, gcv, None, lod_bias=1.0)
    assert (g.lod, g.lod_row_pitch, g.grad_lod, g.grad_lod_row_pitch, g.lod_bias) == (None, 0, None, 0, 1.0)
    # [H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    g = A.volume_grad_grid(0, 2, cv, lv, nhwc[2, 4:14, 8:28], gcv, glv, layout=A.TENSOR_INTERLEAVED, type=A.TENSOR_BF16)
    assert (g.out_x, g.out_y, g.row_pitch, g.plane_pitch) == (20, 10, 200, 0)
    # explicit pointers and pitches
    g = A.volume_grad_grid(1, 4, (4096, 6, 7, 64), (12288, 8), (8192, 16, 9000), (16384, 19), (20480, 9), lod_bias=2.0)
    assert [getattr(g, f) for f in FIELDS] == [1, 4, 6, 7, 4096, 64, 12288, 8, 2.0, 8192, 16, 9000, 16384, 19, 20480, 9]
    assert A.volume_grad_grid(1, 4, (4096, 6, 7, 64), None, (8192, 16, 9000), (16384, 0)).grad_lod is None
    # what the call cannot express
    bad = [dict(gc=gc[3].double()), dict(gc=gc[3, :, :49]), dict(gc=gc[3, :39]), dict(gc=torch.zeros((40, 50, 4))[:, :, :3]), dict(gc=torch.zeros((40, 50, 2))),
           dict(gl=gl[3].half()), dict(gl=gl[3, :, :49]), dict(gl=torch.zeros((50, 40)).t()), dict(up=upstream[3, 0]), dict(up=upstream[3].float()),
           dict(level_count=0), dict(lod_bias=float("nan"))]
    for change in bad:
        kw = dict(level_count=3, gc=gc[3], gl=gl[3], up=upstream[3], lod_bias=0.0)
        kw.update(change)
        with pytest.raises(ValueError):
            A.volume_grad_grid(0, kw["level_count"], coords[3], lod[3], kw["up"], kw["gc"], kw["gl"], lod_bias=kw["lod_bias"], type=A.TENSOR_F16)


def test_volume_grad_kernel_descriptors(built, A, tmp_path):
    """From the code object's metadata notes only: LDS is DecodeBatch + SampleTile, no scratch, no spilled registers, workgroups of
    64, registers for two waves per SIMD.  profiles/decode_volume_grad/kernel_stats.txt holds the counts measured when the kernels
    were written."""
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    grad = {n: d for n, d in by_short.items() if n.startswith("astc_volume_grad")}
    # one build per tensor type and layout
    assert len(grad) == 6, sorted(by_short)
    for name, d in grad.items():
        assert d["group_segment_fixed_size"] == LDS_BYTES, (name, d)
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["vgpr_count"] <= VGPR_BOUND, (name, d)
    # ... and the volume call's kernels are still its six
    assert len([n for n in by_short if n.startswith("astc_volume_sample")]) == 6
