# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_decompress_scaled_tensors_device (windows of compressed images resampled into tensors): what can be checked
without a GPU.

  - the numpy model (tests/scaled_model.py) on hand-made cases: the header's two hand checks, ratio 1, a window one texel wide,
    a box over seven texels, float cases in which a fused multiply-add or another summation order changes the bits;
  - tests/harness/decode_scaled_check.cpp: the staging sink, the clipped window policy and the tile routine (decode_scaled.h),
    tile by tile from the host-built table, against decode_row_batch of the whole image followed by the filter in plain C++, as
    sequential code under the address and undefined-behaviour sanitizers.  It would catch: a tap index or weight one off; a
    clamp at the image's edge instead of the window's; a zero-weight tap read into a sum; a sum restarted or reordered at a run
    or block-row seam; a staging tile overrun; a mirrored row or column one off; a write into padding or between planes;
  - the table builder on hand-computed cases: tiles per region, first[], the clipped source rectangle of tiles; the tiling's
    promise -- a tile wider than 8 columns decodes a block row in one run -- swept over sizes, footprints and data types;
  - the ctypes structures against the C ones, the argument checks that need no context, scaled_region on torch views;
  - the code object of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import scaled_model as S
import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_scaled_check.cpp")

# LDS of a workgroup of astc_decode_scaled: DecodeBatch (7040 B) and ScaledTile -- 6144 B staging, 12 x 4 x 8 binary64 carried row
# sums, the taps of 64 columns and 8 rows (kernel_decode_scaled.hip): nine workgroups per CU
LDS_BOUND = 7040 + 6144 + 12 * 4 * 8 * 8 + (64 + 8) * 16


def test_model_hand_checks_of_the_header():
    # BILINEAR, S = 2, D = 3: texel 0, (t0 + t1) / 2, texel 1
    assert [S.taps(S.BILINEAR, 2, 3, p) for p in range(3)] == [([(0, 1), (0, 5)], 6), ([(0, 3), (1, 3)], 6), ([(1, 5), (1, 1)], 6)]
    # BOX, S = 3, D = 2: (2 t0 + t1) / 3, (t1 + 2 t2) / 3
    assert [S.taps(S.BOX, 3, 2, p) for p in range(2)] == [([(0, 2), (1, 1)], 3), ([(1, 1), (2, 2)], 3)]
    row = np.zeros((1, 3, 4), dtype=np.uint8)
    row[0, :, 0] = (10, 40, 250)
    assert S.resample(row[:, :2], S.BILINEAR, 3, 1)[0, :, 0].tolist() == [10.0, 25.0, 40.0]
    got = S.resample(row, S.BOX, 2, 1)[0, :, 0]
    assert got.tolist() == [np.float32(60.0 / 3.0), np.float32(np.float64(540.0) / np.float64(3.0))]


def test_model_ratio_one_reproduces_the_texel():
    for filt in (S.BILINEAR, S.BOX):
        for size in (1, 2, 37):
            for p in range(size):
                t, den = S.taps(filt, size, size, p)
                assert t == [(p, den)], (filt, size, p)
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    f16 = rng.integers(0, 0x7C00, size=(5, 7, 4), dtype=np.uint16).view(np.float16)          # every finite non-negative half, subnormals included
    f16[1, 2, 0] = np.inf
    f16[3, 3, 1] = np.nan
    f32 = rng.integers(0, 0x7F800000, size=(5, 7, 4), dtype=np.uint32).view(np.float32)
    for filt in (S.BILINEAR, S.BOX):
        for texels in (u8, f16, f32):
            want = texels.astype(np.float32)
            got = S.resample(texels, filt, 7, 5)
            assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
            assert np.array_equal(np.isnan(got), np.isnan(want))
            # ... and then the tensors call's model says the same as the scaled one
            one, zero = [0.5, 3.0, 1.0, 2.0], [1.0, 0.0, -4.0, 0.25]
            assert np.array_equal(S.tensor(texels, filt, 7, 5, M.F16, M.PLANAR, 3, one, zero, M.FLIP_X),
                                  M.tensor(texels[None], M.F16, M.PLANAR, 3, one, zero, M.FLIP_X)[:, 0])


def test_model_one_texel_wide_window_clamps_everything():
    for p in range(5):
        t, den = S.taps(S.BILINEAR, 1, 5, p)
        assert den == 10 and all(k == 0 for k, _ in t) and sum(w for _, w in t) == 10
        assert S.taps(S.BOX, 1, 5, p) == ([(0, 1)], 1)
    col = np.zeros((3, 1, 4), dtype=np.uint8)
    col[:, 0, 1] = (7, 100, 255)
    got = S.resample(col, S.BILINEAR, 5, 3)
    assert got.shape == (3, 5, 4) and all(got[j, :, 1].tolist() == [float(v)] * 5 for j, v in enumerate((7, 100, 255)))


def test_model_box_over_seven_texels():
    assert S.taps(S.BOX, 7, 1, 0) == ([(k, 1) for k in range(7)], 7)
    row = np.zeros((1, 7, 4), dtype=np.uint8)
    row[0, :, 2] = (1, 2, 3, 4, 5, 6, 255)
    want = np.float32(np.float64(276) / np.float64(7))
    assert S.resample(row, S.BOX, 1, 1)[0, 0, 2] == want
    # a zero-weight tap is not read: BILINEAR at ratio 1 next to a NaN and an infinity
    row = np.array([[1.0, np.nan, np.inf, 2.0]], dtype=np.float32)[..., None].repeat(4, axis=2)
    got = S.resample(row, S.BILINEAR, 4, 1)[0, :, 0]
    assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == np.inf and got[3] == 2.0


def test_model_does_not_fuse_and_sums_in_tap_order():
    # Summation order.  BOX 4 -> 1, weights 1, den 4: ((1 + 2^-53) + 2^-53) + -1 is 0 in binary64 (each 2^-53 is half an ulp of
    # 1 and the tie goes to the even 1); right to left it is 2^-52, pairwise it is 2^-53
    e = 2.0 ** -53
    row = np.zeros((1, 4, 4), dtype=np.float32)
    row[0, :, 0] = (1.0, e, e, -1.0)
    assert float(np.float32(e)) == e
    got = S.resample(row, S.BOX, 1, 1)[0, 0, 0]
    assert got == 0.0 and ((-1.0 + e) + e) + 1.0 == 2.0 ** -52 and (1.0 + e) + (e - 1.0) == e
    # Fusing.  x: BILINEAR 2 -> 1, weights 1 and 1; y: BILINEAR 2 -> 3, position 1 has weights 3 and 3.  The rows sum to r and
    # -r with r = 1 + 2^-52, whose triple is a tie in binary64: 3 r rounds to 3 + 2^-50, so 3 r + 3 (-r) is 0 as two products and
    # a sum, and 2^-52 when the second product is fused into the sum
    assert S.taps(S.BILINEAR, 2, 1, 0) == ([(0, 1), (1, 1)], 2) and S.taps(S.BILINEAR, 2, 3, 1) == ([(0, 3), (1, 3)], 6)
    win = np.zeros((2, 2, 4), dtype=np.float32)
    win[0, :, 0] = (1.0, 2.0 ** -52)
    win[1, :, 0] = (-1.0, -2.0 ** -52)
    r = 1.0 + 2.0 ** -52
    assert 3.0 * r == 3.0 + 2.0 ** -50
    fused = float(Fraction(3) * Fraction(-r) + Fraction(3.0 * r))
    assert fused == 2.0 ** -52
    got = S.resample(win, S.BILINEAR, 1, 3)[:, 0, 0]
    assert got[1] == 0.0 and np.float32(fused / 12.0) != 0.0
    assert got[0] == np.float32(r * 0.5) and got[2] == np.float32(-r * 0.5)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_scaled") / "decode_scaled_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tile_routine_matches_decode_filter_convert_place_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # four footprints x four profiles x three data types x two filters x six formats (every tensor type with both layouts)
    assert int(out.stdout.split()[0]) == 4 * 4 * 3 * 2 * 6


def test_wide_tiles_decode_a_block_row_in_one_run(harness):
    """The promise of decode_scaled_tiling that lets the kernel keep carried row sums for 8 columns only: over five footprints, the
    three data types, both filters, window widths 1 .. 700 and up to 65535, output widths 1 .. 300 and up to 65535 and every
    alignment of the window to the blocks, no tile wider than 8 columns reaches more blocks in a block row than a run has."""
    out = subprocess.run([harness, "sweep"], capture_output=True, text=True)
    m = re.search(r"^(\d+) tiles, (\d+) wider than 8 columns, 0 broken$", out.stdout, re.M)
    assert out.returncode == 0 and m, out.stdout + out.stderr
    assert int(m.group(1)) > 10 ** 7 and int(m.group(2)) > 10 ** 7


def test_blocks_mode_counts_what_the_tiles_decode(harness):
    """6x6 U8, one window 300 x 250 at (100, 200) to 224 x 224, BILINEAR: 4 strips x 28 bands; it covers blocks 16 .. 66 by 33 .. 74."""
    out = subprocess.run([harness, "blocks", "0", "6", "6", "0", "224", "224"], input="100 200 300 250\n", capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"decoded (\d+) covered (\d+) tiles (\d+)$", out.stdout.strip())
    assert m and (int(m.group(2)), int(m.group(3))) == (51 * 42, 4 * 28)
    # every covered block is decoded at least once, and a band of 8 rows reaches at most 3 block rows more than it needs
    assert 51 * 42 <= int(m.group(1)) <= 3 * 51 * 42


def test_table_builder_on_hand_computed_cases(harness):
    """6x6 blocks.  Entry 0 is 230 x 50 x 2 U8, entry 1 is 100 x 30 F32.  The staging tile holds 6144 / 4 / 36 = 42 blocks of U8
    texels -- a run is DECODE_BATCH = 32 -- and 6144 / 16 / 36 = 10 of F32.  A run of n blocks holds any (n - 1) * 6 + 1 consecutive
    texels, 187 and 55; a strip is the floor((that - 3) * D / S) columns whose taps fit for certain, at most 64, and 8 where
    fewer than 8 would: 184 * 224 / 192 = 214 -> 64; 52 * 23 / 37 = 32; 184 * 5 / 1 -> 64; 184 * 3 / 230 = 2 -> 8; 52 * 4 / 6 = 34."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(": ", 1) for line in out.stdout.strip().splitlines())

    def parse(line):
        head = re.match(r"count (\d+) total (\d+) returned (\d+) first ([\d ]+) records (.*)$", line)
        recs = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(5))]
        return int(head.group(1)), int(head.group(2)), int(head.group(3)), [int(v) for v in head.group(4).split()], recs

    def tile(name, n):
        m = re.match(r"region (\d+) \[(.*)\]$", lines["%s tile %d" % (name, n)])
        return int(m.group(1)), dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", m.group(2)))

    # BILINEAR, planar F16, 3 channels.  Region 0: 192 x 48 -> 224 x 20 is 4 strips (64, 64, 64, 32 columns) by 3 bands (8, 8, 4
    # rows); region 1: 37 x 23 -> 23 x 37 is 1 strip by 5 bands; region 2: one texel -> 5 x 3 is one tile of 3 rows
    count, total, returned, first, recs = parse(lines["bilinear"])
    assert (count, total, returned, first) == (3, 18, 18, [0, 12, 17])
    fmt = dict(filter=0, type=1, layout=0, channels=3, x_step=1)
    assert recs[0] == dict(cols=64, strips=4, band=8, run_blocks=32, dim_x=230, x=6, y=0, z=0, size_x=192, size_y=48, out_x=224, out_y=20, row=224, plane=4480, flags=1, **fmt)
    assert recs[1] == dict(cols=32, strips=1, band=8, run_blocks=10, dim_x=100, x=10, y=5, z=0, size_x=37, size_y=23, out_x=23, out_y=37, row=30, plane=1200, flags=2, **fmt)
    assert recs[2] == dict(cols=64, strips=1, band=3, run_blocks=32, dim_x=230, x=229, y=49, z=1, size_x=1, size_y=1, out_x=5, out_y=3, row=5, plane=15, flags=0, **fmt)
    # Tile 3, the last strip of the first band.  Column 192: n = 385 * 192 - 224 = 73696 = 164 * 448 + 224, taps 164 and 165;
    # column 223: n = 447 * 192 - 224 = 85600 = 191 * 448 + 32, taps 191 and 192 -> 191 (the window's last).  Row 0: n = 28, taps
    # 0 and 1; row 7: n = 15 * 48 - 20 = 700 = 17 * 40 + 20, taps 17 and 18
    assert tile("bilinear", 3) == (0, dict(c0=192, nc=32, r0=0, nr=8, sx0=164, sx1=191, sy0=0, sy1=18))
    # Tile 11, the last of the region: rows 16 .. 19.  Row 16: n = 33 * 48 - 20 = 1564 = 39 * 40 + 4; row 19: n = 1852 = 46 * 40 + 12
    assert tile("bilinear", 11) == (0, dict(c0=192, nc=32, r0=16, nr=4, sx0=164, sx1=191, sy0=39, sy1=47))
    # Region 1's last band: rows 32 .. 36 of 37 from 23.  Row 32: n = 65 * 23 - 37 = 1458 = 19 * 74 + 52; row 36: n = 1642 = 22 * 74 + 14,
    # taps 22 and 23 -> 22
    assert tile("bilinear", 16) == (1, dict(c0=0, nc=23, r0=32, nr=5, sx0=0, sx1=36, sy0=19, sy1=22))
    assert tile("bilinear", 17) == (2, dict(c0=0, nc=5, r0=0, nr=3, sx0=0, sx1=0, sy0=0, sy1=0))
    # BOX, interleaved BF16, 4 channels.  The whole of entry 0 -> 3 x 2: one tile that reaches every texel; 6 x 6 -> 4 x 9 at the
    # image's corner: two bands, the second is output row 8 alone, which is source row (8 * 6) / 9 = 5
    count, total, returned, first, recs = parse(lines["box"])
    assert (count, total, returned, first) == (2, 3, 3, [0, 1])
    fmt = dict(filter=1, type=2, layout=1, channels=4, x_step=4, plane=0)
    assert recs[0] == dict(cols=8, strips=1, band=2, run_blocks=32, dim_x=230, x=0, y=0, z=0, size_x=230, size_y=50, out_x=3, out_y=2, row=12, flags=3, **fmt)
    assert recs[1] == dict(cols=34, strips=1, band=8, run_blocks=10, dim_x=100, x=94, y=24, z=0, size_x=6, size_y=6, out_x=4, out_y=9, row=16, flags=0, **fmt)
    assert tile("box", 0) == (0, dict(c0=0, nc=3, r0=0, nr=2, sx0=0, sx1=229, sy0=0, sy1=49))
    assert tile("box", 2) == (1, dict(c0=0, nc=4, r0=8, nr=1, sx0=0, sx1=5, sy0=5, sy1=5))


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    cname, cls = "astcenc_amd_scaled_region", A.ScaledRegion
    body = '  printf("%%zu", sizeof(%s));\n' % cname
    body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body +
                     '  printf("%d %d %zu\\n", ASTCENC_AMD_WINDOW_BILINEAR, ASTCENC_AMD_WINDOW_BOX, sizeof(enum astcenc_amd_window_filter));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    got = [int(v) for v in lines[0].split()]
    assert got[0] == C.sizeof(cls)
    assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in cls._fields_] == ["entry", "x", "y", "z", "size_x", "size_y", "out_x", "out_y", "flags", "out", "row_pitch", "plane_pitch"]
    assert [int(v) for v in lines[1].split()] == [A.WINDOW_BILINEAR, A.WINDOW_BOX, C.sizeof(C.c_int)]
    assert (S.BILINEAR, S.BOX) == (A.WINDOW_BILINEAR, A.WINDOW_BOX)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_decompress_scaled_tensors_device
    assert "astcenc_amd_decompress_scaled_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.decompress_scaled_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    region = (A.ScaledRegion * 1)(A.ScaledRegion(0, 0, 0, 0, 1, 1, 2, 2, 0, None, 0, 0))
    # no regions: nothing to do, whatever else is passed (an unknown filter included)
    assert fn(None, None, 0, None, 7, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), A.WINDOW_BOX, region, 0, None) == A.SUCCESS
    # a null context; a count without regions; a count without entries
    assert fn(None, one, 1, C.byref(fmt), A.WINDOW_BOX, region, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), A.WINDOW_BILINEAR, None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), A.WINDOW_BILINEAR, region, 1, None) == A.ERR_BAD_PARAM


def test_scaled_region_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    # [C, H, W]: one sample of a batch, then a tile of it
    r = A.scaled_region(2, (5, 6, 1), (70, 33), batch[3], flip_x=True)
    assert (r.entry, r.x, r.y, r.z, r.size_x, r.size_y, r.out_x, r.out_y, r.flags) == (2, 5, 6, 1, 70, 33, 50, 40, A.TENSOR_FLIP_X)
    assert (r.out, r.row_pitch, r.plane_pitch) == (batch[3].data_ptr(), 50, 2000)
    view = batch[1, :, 4:14, 8:28]
    r = A.scaled_region(0, (0, 0, 0), (3, 3), view, flip_y=True)
    assert (r.out, r.out_x, r.out_y, r.row_pitch, r.plane_pitch, r.flags) == (view.data_ptr(), 20, 10, 50, 2000, A.TENSOR_FLIP_Y)
    # the first two channels of a wider tensor
    assert A.scaled_region(0, (0, 0, 0), (50, 40), batch[0, :2]).plane_pitch == 2000
    # [H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    view = nhwc[2, 4:14, 8:28]
    r = A.scaled_region(0, (0, 0, 0), (200, 100), view, layout=A.TENSOR_INTERLEAVED, flip_x=True, flip_y=True)
    assert (r.out, r.out_x, r.out_y, r.row_pitch, r.plane_pitch, r.flags) == (view.data_ptr(), 20, 10, 200, 0, 3)
    # explicit pointer, output size and pitches
    r = A.scaled_region(1, (1, 2, 3), (4, 5), (4096, 6, 7, 64, 9000))
    assert (r.entry, r.z, r.size_x, r.size_y, r.out, r.out_x, r.out_y, r.row_pitch, r.plane_pitch) == (1, 3, 4, 5, 4096, 6, 7, 64, 9000)


def test_scaled_region_rejects_views_the_layouts_cannot_express(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.float16)
    bad = [
        (batch[0, :, :, 0:40:2], (20, 40), A.TENSOR_PLANAR),               # every second column
        (batch[0].permute(0, 2, 1), (40, 50), A.TENSOR_PLANAR),            # transposed: columns a row apart
        (nhwc[0, :, :, :3], (50, 40), A.TENSOR_INTERLEAVED),               # three channels of four: columns are not C apart
        (nhwc[0, :, :, ::2], (50, 40), A.TENSOR_INTERLEAVED),              # channels that are not adjacent
        (nhwc[0].permute(2, 0, 1), (50, 40), A.TENSOR_PLANAR),             # a channels-last tensor seen as planar
        (batch, (50, 40), A.TENSOR_PLANAR),                                # four dimensions: a region is one sample
        (batch[0, 0], (50, 40), A.TENSOR_PLANAR),                          # two dimensions
        (batch[0], (70000, 40), A.TENSOR_PLANAR),                          # a window wider than 65535
        (batch[0], (50, 0), A.TENSOR_PLANAR),                              # an empty window
        (batch[0, :, :0], (50, 40), A.TENSOR_PLANAR),                      # an empty output
        # expanded views: a zero stride would reach the call as "tightly packed" and write where the view does not alias
        (batch[0, :1].expand(3, 40, 50), (50, 40), A.TENSOR_PLANAR),       # one plane seen as three
        (batch[0, :, :1].expand(3, 40, 50), (50, 40), A.TENSOR_PLANAR),    # one row seen as forty
        (batch[0, :, :, :1].expand(3, 40, 50), (50, 40), A.TENSOR_PLANAR),
        (nhwc[0, :1].expand(40, 50, 4), (50, 40), A.TENSOR_INTERLEAVED),
    ]
    for view, size, layout in bad:
        with pytest.raises(ValueError):
            A.scaled_region(0, (0, 0, 0), size, view, layout=layout)
    # the view's dtype against the format's type, where the caller names it (Library.decompress_scaled_tensors_device does)
    for type, dtype in ((A.TENSOR_F32, torch.float16), (A.TENSOR_F16, torch.bfloat16), (A.TENSOR_BF16, torch.float16), (A.TENSOR_F16, torch.float32)):
        with pytest.raises(ValueError):
            A.scaled_region(0, (0, 0, 0), (50, 40), torch.zeros((3, 40, 50), dtype=dtype), type=type)
    for type, dtype in ((A.TENSOR_F32, torch.float32), (A.TENSOR_F16, torch.float16), (A.TENSOR_BF16, torch.bfloat16)):
        assert A.scaled_region(0, (0, 0, 0), (50, 40), torch.zeros((3, 40, 50), dtype=dtype), type=type).out_x == 50
    # an axis of length one has no pitch to speak of: the tight one
    r = A.scaled_region(0, (0, 0, 0), (50, 40), batch[0, :1, :1].expand(1, 1, 50))
    assert (r.out_x, r.out_y, r.row_pitch, r.plane_pitch) == (50, 1, 0, 0)


def test_scaled_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    scaled = {n: d for n, d in by_short.items() if n.startswith("astc_decode_scaled")}
    # one build per tensor type and layout
    assert len(scaled) == 6, sorted(by_short)
    for name, d in scaled.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["group_segment_fixed_size"] <= LDS_BOUND, (name, d)
        # the names the other code-object tests pick kernels by do not match the new ones
        assert not name.startswith(("astc_decode_regions", "astc_decode_tensors", "astc_decompress_blocks", "astc_decompress_set", "astc_compare_"))
