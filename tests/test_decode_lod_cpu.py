# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_lod_tensors_device (compressed mip chains sampled at a level of detail per point): what can be checked
without a GPU.

  - the numpy model (tests/sample_lod_model.py) on hand-made cases: the levels and weights of special lambda under both mip
    filters, a blend in which a fused multiply-add changes the bits, g = 0 next to a level of NaNs, lod NULL and a lod_bias that
    moves a point across a level, the validity limit; the consequence on power-of-two levels; the array form of the model against
    its pointwise form;
  - tests/harness/decode_lod_check.cpp: the tile routine (decode_lod.h) tile by tile from the host-built table against
    decode_row_batch of every whole level followed by the definition in plain C++, as sequential code under the address and
    undefined-behaviour sanitizers.  It would catch: a level or a weight one off; a point sampled on another lane's level; a level
    of weight zero read; a slot overwritten by a later pass; a lod read from a row's padding; everything the sample harness catches
    within a level;
  - the table builder on a hand-computed case, the kernel's level selection against the model's;
  - the ctypes structures and enums against the C ones, the argument checks that need no context, lod_grid on torch views;
  - the code object of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sample_lod_model as L
import sample_model as S
import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_lod_check.cpp")

# LDS of a workgroup of astc_lod_sample: what astc_decode_sample has -- DecodeBatch (7040 B) and the list of a batch's 32 block indices
LDS_BOUND = 7040 + 32 * 4
# three waves per SIMD: 512 registers / 3, in allocation granules of 8
VGPR_BOUND = 168

MODES = (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER)
MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)


def pairs(mip, count, lam):
    return [(l, float(w)) for l, w in L.levels(mip, count, np.float32(lam))]


def test_model_levels_of_special_lambdas():
    n = 5
    for mip in MIPS:
        assert pairs(mip, n, -1.0) == [(0, 1.0)]
        assert pairs(mip, n, 0.0) == [(0, 1.0)] and pairs(mip, n, -0.0) == [(0, 1.0)]
        assert pairs(mip, n, 1.0) == [(1, 1.0)]
        assert pairs(mip, n, n - 1) == [(4, 1.0)]
        assert pairs(mip, n, n + 3) == [(4, 1.0)]
        assert pairs(mip, n, np.inf) == [(4, 1.0)] and pairs(mip, n, -np.inf) == [(0, 1.0)]
        # a NaN lambda' is no level at all: the point is invalid
        assert not L.valid(0.5, 0.5, np.float32(np.nan)) and L.valid(0.5, 0.5, np.float32(np.inf)) and L.valid(0.5, 0.5, np.float32(-np.inf))
    # 0.5 selects level 0 under MIP_NEAREST (the finer level on a tie), the next binary32 level 1; 1.5 selects level 1
    assert pairs(L.MIP_NEAREST, n, 0.5) == [(0, 1.0)]
    assert pairs(L.MIP_NEAREST, n, np.nextafter(np.float32(0.5), np.float32(1.0))) == [(1, 1.0)]
    assert pairs(L.MIP_NEAREST, n, np.nextafter(np.float32(0.5), np.float32(0.0))) == [(0, 1.0)]
    assert pairs(L.MIP_NEAREST, n, 1.5) == [(1, 1.0)] and pairs(L.MIP_NEAREST, n, 1.75) == [(2, 1.0)]
    assert pairs(L.MIP_NEAREST, n, 3.75) == [(4, 1.0)] and pairs(L.MIP_NEAREST, n, 1e-30) == [(0, 1.0)]
    # MIP_LINEAR: 0.5 and 1.5 are halfway; the weights are exact
    assert pairs(L.MIP_LINEAR, n, 0.5) == [(0, 0.5), (1, 0.5)]
    assert pairs(L.MIP_LINEAR, n, 1.5) == [(1, 0.5), (2, 0.5)]
    assert pairs(L.MIP_LINEAR, n, 3.75) == [(3, 0.25), (4, 0.75)]
    # (1 - 1e-30 rounds to 1 in binary64: level 0 has weight 1.0 and level 1 is still part of the sum, with its tiny weight)
    assert pairs(L.MIP_LINEAR, n, 1e-30) == [(0, 1.0), (1, float(np.float32(1e-30)))]
    # a chain of one level: that level, whatever lambda is
    for mip in MIPS:
        for lam in (-1.0, 0.0, 0.5, 7.0, np.inf):
            assert pairs(mip, 1, lam) == [(0, 1.0)]


def one_texel_chain(values, dtype=np.float32):
    return [np.full((1, 1, 4), v, dtype=dtype) for v in values]


def round_to_f32(q):
    """The binary32 nearest to the rational q (no tie among the candidates here)."""
    c = np.float32(float(q))
    best = min((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))), key=lambda f: abs(Fraction(float(f)) - q))
    return np.float32(best)


def test_model_blend_is_two_products_and_a_sum_never_fused():
    """g = 2^-29 (1 + 2^-23) has w0 = 1 - g of 52 significant bits, so w0 s0 rounds for s0 = 1 + 15 2^-23; g s1 is exact (two
    binary32 values).  With s1 = -(1 + 13 2^-23) 2^29 the two products cancel to a few units in the last place of the first: what
    the sum keeps of w0 s0 is its rounding.  Fusing the first product into the sum keeps its exact value: another binary32."""
    g = np.float32(2.0 ** -29 * (1.0 + 2.0 ** -23))
    s0, s1 = np.float32(1.0 + 15 * 2.0 ** -23), np.float32(-(1.0 + 13 * 2.0 ** -23) * 2.0 ** 29)
    assert pairs(L.MIP_LINEAR, 2, g) == [(0, 1.0 - float(g)), (1, float(g))]
    w0 = 1.0 - float(g)
    assert Fraction(w0) == 1 - Fraction(float(g))                                          # the weight is exact
    assert Fraction(w0 * float(s0)) != Fraction(w0) * Fraction(float(s0))                  # the first product rounds
    assert Fraction(float(g) * float(s1)) == Fraction(float(g)) * Fraction(float(s1))      # the second does not
    got = L.sample_point(one_texel_chain([s0, s1]), S.NEAREST, S.CLAMP, S.CLAMP, L.MIP_LINEAR, 0.5, 0.5, g, 0.0)[0]
    unfused = np.float32(w0 * float(s0) + float(g) * float(s1))
    fused = round_to_f32(Fraction(w0) * Fraction(float(s0)) + Fraction(float(g)) * Fraction(float(s1)))
    assert got == unfused == np.float32(float.fromhex("0x1.f7ffccp-24"))
    assert fused == np.float32(float.fromhex("0x1.f7ffcap-24")) and fused != got
    assert L.sample(one_texel_chain([s0, s1]), S.NEAREST, S.CLAMP, S.CLAMP, L.MIP_LINEAR, [[[0.5, 0.5]]], np.array([[g]], dtype=np.float32), 0.0)[0, 0, 0] == got


def test_model_level_of_weight_zero_is_not_read():
    chain = one_texel_chain([3.0, np.nan, 5.0])
    for mip in MIPS:
        for form in (L.sample, L.sample_pointwise):
            def at(lam, bias=0.0, lod=True):
                return form(chain, S.BILINEAR, S.CLAMP, S.CLAMP, mip, np.array([[[0.25, 0.75]]], dtype=np.float32),
                            np.array([[lam]], dtype=np.float32) if lod else None, bias)[0, 0, 0]
            # g = 0 next to the level of NaNs, on either side; l0 = level_count - 1 has no l0 + 1 at all
            assert at(0.0) == 3.0 and at(2.0) == 5.0 and at(9.0) == 5.0 and at(-4.0) == 3.0
            assert np.isnan(at(1.0))
            # lod NULL: lambda' is the bias
            assert at(0.0, bias=2.0, lod=False) == 5.0 and at(0.0, bias=0.0, lod=False) == 3.0 and np.isnan(at(0.0, bias=1.0, lod=False))
        # a quarter of a level further the NaN is in the sum (MIP_LINEAR), or still a level away (MIP_NEAREST)
        got = L.sample(chain, S.NEAREST, S.CLAMP, S.CLAMP, mip, [[[0.5, 0.5]]], np.array([[0.25]], dtype=np.float32), 0.0)[0, 0, 0]
        assert np.isnan(got) if mip == L.MIP_LINEAR else got == 3.0


def test_model_lod_bias_moves_a_point_across_a_level():
    chain = one_texel_chain([10.0, 20.0, 40.0])
    def at(mip, lod, bias):
        return float(L.sample_point(chain, S.NEAREST, S.REPEAT, S.REPEAT, mip, 0.5, 0.5, lod, bias)[0])
    assert at(L.MIP_LINEAR, 0.75, 0.0) == 17.5 and at(L.MIP_LINEAR, 0.75, 0.5) == 25.0 and at(L.MIP_LINEAR, 0.75, -1.0) == 10.0
    assert at(L.MIP_NEAREST, 0.25, 0.0) == 10.0 and at(L.MIP_NEAREST, 0.25, 0.5) == 20.0 and at(L.MIP_NEAREST, 0.25, 1.5) == 40.0
    # one float32 addition: 2^-30 vanishes against 1.5
    assert L.lambda_prime(np.float32(2.0 ** -30), 1.5) == np.float32(1.5) and at(L.MIP_LINEAR, 2.0 ** -30, 1.5) == 30.0
    # an infinite lod clamps whatever the bias; a NaN lod is an invalid point: +0.0, then scale and bias like any other
    assert at(L.MIP_LINEAR, np.inf, -5.0) == 40.0 and at(L.MIP_LINEAR, -np.inf, 5.0) == 10.0 and at(L.MIP_LINEAR, np.nan, 0.0) == 0.0
    bits = L.convert(chain, S.NEAREST, S.CLAMP, S.CLAMP, L.MIP_LINEAR, [[[0.5, 0.5], [0.5, 0.5]]], np.array([[np.nan, 1.0]], dtype=np.float32), 0.0,
                     M.F32, 2, [2.0, 2.0, 1.0, 1.0], [0.5, -1.0, 0.0, 0.0])
    assert bits[0, 0, 0].view(np.float32).tolist() == [0.5, -1.0] and bits[0, 0, 1].view(np.float32).tolist() == [40.5, 39.0]


def test_model_validity_limit():
    big = np.float32(2.0 ** 14)
    nxt = np.nextafter(big, np.float32(np.inf))
    assert L.valid(big, -big, 0.0) and not L.valid(nxt, 0.0, 0.0) and not L.valid(0.0, -nxt, 0.0)
    assert not L.valid(np.nan, 0.0, 0.0) and not L.valid(0.0, np.inf, 0.0) and not L.valid(0.0, 0.0, np.nan)
    # 2^14 on an axis of 65536 texels is the level coordinate 2^30, the sample call's own limit
    assert float(big) * 65536 == 2.0 ** 30
    img = np.arange(4 * 4 * 4, dtype=np.uint8).reshape(4, 4, 4)
    coords = np.array([[[big, 0.125], [nxt, 0.125], [0.125, -big], [0.125, -nxt], [np.nan, 0.125], [0.125, np.inf]]], dtype=np.float32)
    for form in (L.sample, L.sample_pointwise):
        got = form([img], S.NEAREST, S.REPEAT, S.REPEAT, L.MIP_LINEAR, coords, None, 0.0)[0, :, 0].tolist()
        # (2^14 is a whole number of periods: texel 0 of that axis)
        assert got == [0.0, 0.0, 0.0, 0.0, 0.0, 0.0] and float(img[0, 0, 1]) == 1.0
        got = form([img], S.NEAREST, S.REPEAT, S.REPEAT, L.MIP_LINEAR, coords, None, 0.0)[0, :, 1].tolist()
        assert got == [1.0, 0.0, 1.0, 0.0, 0.0, 0.0]


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
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def test_model_on_power_of_two_levels_is_the_sample_model():
    """W_l and H_l powers of two: u W_l and v H_l are binary32 values, so at an integer lambda (or with one level) the result is
    sample_model.sample of that level at (u W_l, v H_l), under either mip filter."""
    dims = [(32, 16), (16, 8), (8, 4), (4, 2)]
    rng = np.random.default_rng(3)
    coords = rng.uniform(-0.5, 1.5, size=(7, 9, 2)).astype(np.float32)
    for kind in range(4):
        chain = random_chain(kind, dims, kind)
        for filt in (S.NEAREST, S.BILINEAR):
            for k, mode in enumerate(MODES):
                for mip in MIPS:
                    for l, (w, h) in enumerate(dims):
                        texel = coords * np.array([w, h], dtype=np.float32)
                        assert np.array_equal(texel.astype(np.float64), coords.astype(np.float64) * np.array([w, h], dtype=np.float64))
                        want = S.sample(chain[l], filt, mode, MODES[(k + 1) % 4], texel)
                        got = L.sample(chain, filt, mode, MODES[(k + 1) % 4], mip, coords, np.full(coords.shape[:2], l, dtype=np.float32), 0.0)
                        assert same_bits(got, want)
                        one = L.sample(chain[l:l + 1], filt, mode, MODES[(k + 1) % 4], mip, coords, np.full(coords.shape[:2], 0.625, dtype=np.float32), 0.0)
                        assert same_bits(one, want)


def test_model_array_form_is_the_pointwise_form():
    dims = L.chain_dims(17, 11)
    assert dims == [(17, 11), (8, 5), (4, 2), (2, 1), (1, 1)]
    rng = np.random.default_rng(11)
    su, sl = L.special_coordinates(), L.special_lambdas(len(dims))
    grid = np.stack(np.meshgrid(su, su, indexing="xy"), axis=-1)
    grid_lod = sl[(np.arange(grid.shape[0])[:, None] * 7 + np.arange(grid.shape[1])[None, :]) % len(sl)]
    rand = rng.uniform(-0.25, 1.25, size=(9, 13, 2)).astype(np.float32)
    rand_lod = rng.uniform(-1.0, len(dims) + 0.5, size=(9, 13)).astype(np.float32)
    for kind in (0, 1, 3):
        chain = random_chain(20 + kind, dims, kind)
        for filt in (S.NEAREST, S.BILINEAR):
            for mip in MIPS:
                for ax, ay in ((S.CLAMP, S.BORDER), (S.REPEAT, S.MIRROR), (S.MIRROR, S.REPEAT), (S.BORDER, S.CLAMP)):
                    for coords, lod, bias in ((grid, grid_lod, 0.0), (rand, rand_lod, 0.25), (rand, None, 1.5)):
                        a = L.sample(chain, filt, ax, ay, mip, coords, lod, bias)
                        b = L.sample_pointwise(chain, filt, ax, ay, mip, coords, lod, bias)
                        assert same_bits(a, b), (kind, filt, mip, ax, ay)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_lod") / "decode_lod_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tile_routine_matches_levels_sample_blend_convert_place_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # four footprints x four profiles x four chains (U8, F16, F32, mixed) x two mip filters x two filters x six formats (every tensor
    # type with both layouts); the corner grid of every footprint under both mip filters; the NaN chain under 2 x 2 samplers
    assert int(re.search(r"^(\d+) configurations", out.stdout, re.M).group(1)) == 4 * 4 * 4 * 2 * 2 * 6 + 4 * 2 + 4 * 4
    assert "address mode pairs met: 16 of 16" in out.stdout
    # 256 distinct blocks in the level-0 pass: eight full batches; then the level-1 pass of MIP_LINEAR (9 x 9 blocks at most)
    for name in ("4x4", "6x6", "10x8", "12x12"):
        assert "%s corners mip 0: tiles 1 passes 1 batches 8 blocks 256" % name in out.stdout, out.stdout
        m = re.search(r"^%s corners mip 1: tiles 1 passes 2 batches (\d+) blocks (\d+)$" % name, out.stdout, re.M)
        assert m and 256 < int(m.group(2)) <= 256 + 81 and int(m.group(1)) >= 9, out.stdout
    # some tile really had its points on at least four levels; both g = 0 and g != 0 occurred
    assert int(re.search(r"^most distinct levels in a tile: (\d+)$", out.stdout, re.M).group(1)) >= 4
    assert "g = 0 met: 1, g != 0 met: 1" in out.stdout


def test_blocks_mode_counts_passes_batches_and_blocks(harness, tmp_path):
    """6x6, a 120 x 60 image and its first three levels (120 x 60, 60 x 30, 30 x 15), BILINEAR, CLAMP, MIP_LINEAR, a 16 x 5 grid (two
    8 x 8 tiles across, one down).  Tile 0: every point at the centre of level 0's texel (0, 0) with lambda 0: one pass, one batch,
    one block.  Tile 1: rows 0 .. 3 at (0.05, 0.1) -- level 0's corner (6, 6): blocks (0, 0), (1, 0), (0, 1), (1, 1) -- with
    lambda 0.5, so level 1 is sampled at (3, 3): one block; row 4 at lambda 2: level 2 at (1.5, 1.5), one block.  Three passes,
    three batches, six blocks."""
    coords = np.zeros((5, 16, 2), dtype=np.float32)
    lod = np.zeros((5, 16), dtype=np.float32)
    coords[:, :8] = (0.5 / 120, 0.5 / 60)
    coords[:, 8:] = (0.05, 0.1)
    lod[:4, 8:] = 0.5
    lod[4, 8:] = 2.0
    assert float(np.float64(np.float32(0.05)) * 120) > 6.0 - 1e-5 and float(np.float64(np.float32(0.05)) * 120) < 6.5
    cpath, lpath = tmp_path / "coords.f32", tmp_path / "lod.f32"
    coords.tofile(str(cpath))
    lod.tofile(str(lpath))
    args = [harness, "blocks", "1", "0", "0", "1", "6", "6", "120", "60", "3", "16", "5", str(cpath)]
    out = subprocess.run(args + [str(lpath)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "tiles 2 passes 4 batches 4 decoded 7 points 80"
    # lod NULL: level 0 everywhere -- one block, and the corner's four
    out = subprocess.run(args + ["-"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "tiles 2 passes 2 batches 2 decoded 5 points 80"


def test_table_builder_and_level_selection_on_hand_computed_cases(harness):
    """6x6 blocks.  Entries 0 .. 2 are a chain of 100 x 60 x 2 U8, 50 x 30 x 2 F16 and 25 x 15 x 2 F32, entry 3 is 64 x 64 U8; BILINEAR,
    BORDER along x, REPEAT along y, MIP_LINEAR, planar BF16 with two channels.  Grid 0: the three levels, 100 x 1 points (two 64 x 1
    tiles); grid 1: entry 3 alone, 9 x 5 (two 8 x 8 tiles); grid 2: levels 1 and 2 as a chain of their own, 20 x 17 (three across,
    three down), lod NULL.  The table: 16 bytes of head, first[3], padding to 32, three records, then 3 + 1 + 2 level records."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    head = re.match(r"table: bytes (\d+) levels_at (\d+) level_bytes (\d+) count (\d+) total (\d+) returned (\d+) first ([\d ]+) records (.*)$", lines[0])
    size, levels_at, level_bytes, count, total, returned = (int(head.group(i)) for i in range(1, 7))
    assert (count, total, returned) == (3, 13, 13)
    assert [int(v) for v in head.group(7).split()] == [0, 2, 4]
    assert (levels_at - 32) % 3 == 0 and size == levels_at + 6 * level_bytes
    recs = re.findall(r"\[([^\]]*)\]", head.group(8))
    fields = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (-?\d+)", r.split(" dims")[0])) for r in recs]
    dims = [r.split(" dims ")[1].split() for r in recs]
    fmt = dict(filter=1, address_x=3, address_y=1, mip_filter=1, type=2, layout=0, channels=2, x_step=1)
    assert fields[0] == dict(tw=64, th=1, tiles_x=2, levels=levels_at, level_count=3, z=1, out_x=100, out_y=1, coord_row=200, has_lod=1, lod_row=100, bias_x4=2,
                             row=100, plane=100, **fmt)
    assert fields[1] == dict(tw=8, th=8, tiles_x=2, levels=levels_at + 3 * level_bytes, level_count=1, z=0, out_x=9, out_y=5, coord_row=24, has_lod=1, lod_row=16,
                             bias_x4=0, row=12, plane=70, **fmt)
    assert fields[2] == dict(tw=8, th=8, tiles_x=3, levels=levels_at + 4 * level_bytes, level_count=2, z=0, out_x=20, out_y=17, coord_row=40, has_lod=0, lod_row=20,
                             bias_x4=-4, row=20, plane=340, **fmt)
    assert dims == [["100x60t0", "50x30t1", "25x15t2"], ["64x64t0"], ["50x30t1", "25x15t2"]]
    # the kernel's levels and weights are the model's, for the hand-checked lambda in a chain of five levels
    seen = 0
    for line in lines[1:]:
        m = re.match(r"lambda (\S+) mip (\d): (\d+) (-?\d+) (\S+)$", line)
        if not m:
            continue
        lam, mip, l0, l1, g = float.fromhex(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), float.fromhex(m.group(5))
        want = L.levels(mip, 5, np.float32(lam))
        assert l0 == want[0][0] and (l1 == -1) == (len(want) == 1), line
        if len(want) == 2:
            assert (l1, g) == (want[1][0], float(want[1][1])), line
        else:
            assert g == 0.0, line
        seen += 1
    assert seen == 15 * 2
    # ... and its validity rule
    valid = [(float.fromhex(a), float.fromhex(b), float.fromhex(c), int(d)) for a, b, c, d in re.findall(r"^valid (\S+) (\S+) (\S+): (\d)$", out.stdout, re.M)]
    assert len(valid) == 8
    for u, v, lam, got in valid:
        assert bool(got) == L.valid(np.float32(u), np.float32(v), np.float32(lam)), (u, v, lam)


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    body = ""
    for cname, cls in (("astcenc_amd_lod_grid", A.LodGrid), ("astcenc_amd_lod_sampler", A.LodSampler)):
        body += '  printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body +
                     '  printf("%d %d %zu\\n", ASTCENC_AMD_MIP_NEAREST, ASTCENC_AMD_MIP_LINEAR, sizeof(enum astcenc_amd_mip_level_filter));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, cls in zip(lines, (A.LodGrid, A.LodSampler)):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in A.LodGrid._fields_] == ["first_entry", "level_count", "z", "out_x", "out_y", "coords", "coord_row_pitch", "lod", "lod_row_pitch", "lod_bias",
                                                  "out", "row_pitch", "plane_pitch"]
    assert [f for f, _ in A.LodSampler._fields_] == ["filter", "address_x", "address_y", "mip_filter"]
    assert [int(v) for v in lines[2].split()] == [A.MIP_NEAREST, A.MIP_LINEAR, C.sizeof(C.c_int)]
    assert (L.MIP_NEAREST, L.MIP_LINEAR) == (A.MIP_NEAREST, A.MIP_LINEAR)
    assert L.MAX_LEVELS == A.MAX_MIP_LEVELS
    # the header compiles as C too (the enum's tag is not the mip generation filter's)
    if shutil.which("gcc"):
        c_probe = tmp_path / "probe.c"
        c_probe.write_text('#include "astcenc_amd.h"\nint main(void) { struct astcenc_amd_lod_sampler s; s.mip_filter = ASTCENC_AMD_MIP_LINEAR; return (int)s.mip_filter - 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c_probe), "-o", str(tmp_path / "probe_c")], check=True)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_lod_tensors_device
    assert "astcenc_amd_sample_lod_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_lod_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
    grid = (A.LodGrid * 1)(A.LodGrid(0, 1, 0, 2, 2, None, 0, None, 0, 0.0, None, 0, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_lod_grid_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((8, 40, 50, 2), dtype=torch.float32)
    lod = torch.zeros((8, 40, 50), dtype=torch.float32)
    g = A.lod_grid(2, 7, 1, coords[3], lod[3], batch[3], lod_bias=-0.5)
    assert (g.first_entry, g.level_count, g.z, g.out_x, g.out_y, g.lod_bias) == (2, 7, 1, 50, 40, -0.5)
    assert (g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (coords[3].data_ptr(), 100, lod[3].data_ptr(), 50, batch[3].data_ptr(), 50, 2000)
    # a tile of all three
    cv, lv, ov = coords[1, 4:14, 8:28], lod[1, 4:14, 8:28], batch[1, :, 4:14, 8:28]
    g = A.lod_grid(0, 1, 0, cv, lv, ov)
    assert (g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (20, 10, cv.data_ptr(), 100, lv.data_ptr(), 50, ov.data_ptr(), 50, 2000)
    # no lod: NULL, 0 everywhere
    g = A.lod_grid(0, 3, 0, cv, None, ov, lod_bias=1.0)
    assert (g.lod, g.lod_row_pitch, g.lod_bias) == (None, 0, 1.0)
    # [H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    g = A.lod_grid(0, 2, 0, cv, lv, nhwc[2, 4:14, 8:28], layout=A.TENSOR_INTERLEAVED, type=A.TENSOR_BF16)
    assert (g.out_x, g.out_y, g.row_pitch, g.plane_pitch) == (20, 10, 200, 0)
    # one row of points: a list; the pitches of an axis of length one are the tight ones
    pts = torch.zeros((1, 1000, 2), dtype=torch.float32)
    g = A.lod_grid(0, 32, 0, pts, torch.zeros((1, 1000), dtype=torch.float32), torch.zeros((3, 1, 1000), dtype=torch.float32), type=A.TENSOR_F32)
    assert (g.out_x, g.out_y, g.coord_row_pitch, g.lod_row_pitch, g.row_pitch) == (1000, 1, 0, 0, 0)
    # explicit pointers and pitches
    g = A.lod_grid(1, 4, 3, (4096, 6, 7, 64), (12288, 8), (8192, 16, 9000), lod_bias=2.0)
    assert (g.first_entry, g.level_count, g.z, g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.lod_bias, g.out, g.row_pitch, g.plane_pitch) == \
        (1, 4, 3, 6, 7, 4096, 64, 12288, 8, 2.0, 8192, 16, 9000)
    assert A.lod_grid(1, 4, 3, (4096, 6, 7, 64), None, (8192, 16, 9000)).lod is None


def test_lod_grid_rejects_what_the_call_cannot_express(A):
    torch = pytest.importorskip("torch")
    out = torch.zeros((3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((40, 50, 2), dtype=torch.float32)
    lod = torch.zeros((40, 50), dtype=torch.float32)
    wide = torch.zeros((40, 100), dtype=torch.float32)
    bad = [
        dict(lod=lod.double()),                                            # float64 levels of detail
        dict(lod=lod.half()),
        dict(lod=torch.zeros((40, 50, 1))),                                # three dimensions
        dict(lod=lod[:, :49]),                                             # another width than the points'
        dict(lod=lod[:39]),                                                # another height
        dict(lod=wide[:, ::2]),                                            # columns two floats apart
        dict(lod=torch.zeros((50, 40)).t()),                               # transposed: columns a row apart
        dict(lod=lod[:1].expand(40, 50)),                                  # one row seen as forty
        dict(level_count=0),
        dict(level_count=33),
        dict(lod_bias=float("inf")),
        dict(lod_bias=float("nan")),
        # what sample_grid rejects of the coordinates and of the output
        dict(coords=coords.double()),
        dict(coords=coords[:, :49]),
        dict(out=out[0]),
        dict(out=out[:1].expand(3, 40, 50)),
    ]
    for change in bad:
        kw = dict(level_count=3, coords=coords, lod=lod, out=out, lod_bias=0.0)
        kw.update(change)
        with pytest.raises(ValueError):
            A.lod_grid(0, kw["level_count"], 0, kw["coords"], kw["lod"], kw["out"], lod_bias=kw["lod_bias"])
    with pytest.raises(ValueError):
        A.lod_grid(0, 3, 0, coords, lod, torch.zeros((3, 40, 50), dtype=torch.float32), type=A.TENSOR_F16)
    assert A.lod_grid(0, 3, 0, coords, lod, out, type=A.TENSOR_F16).out_x == 50
    # (the rows of a padded lod may be any number of floats apart: there is no alignment beyond the float's)
    assert A.lod_grid(0, 3, 0, coords, torch.zeros((40, 53))[:, :50], out).lod_row_pitch == 53


def test_lod_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    lod = {n: d for n, d in by_short.items() if n.startswith("astc_lod_sample")}
    # one build per tensor type and layout
    assert len(lod) == 6, sorted(by_short)
    for name, d in lod.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["group_segment_fixed_size"] <= LDS_BOUND, (name, d)
        assert d["vgpr_count"] <= VGPR_BOUND, (name, d)
        # the names the other code-object tests pick kernels by do not match the new ones
        assert not name.startswith(("astc_decode_sample", "astc_decode_regions", "astc_decode_tensors", "astc_decode_scaled", "astc_decompress_blocks", "astc_decompress_set",
                                    "astc_compare_"))
    # ... and the sample call's kernels are still its six
    assert len([n for n in by_short if n.startswith("astc_decode_sample")]) == 6
