# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_tensors_device (compressed images sampled at coordinates into tensors): what can be checked without a GPU.

  - the numpy model (tests/sample_model.py) on hand-made cases: the taps at the edges and at special coordinates under each
    address mode, the texel-centre consequence, a zero-weight tap next to a NaN and an infinity, float cases in which a fused
    multiply-add or summing y before x changes the bits, invalid points; the array form of the model against its pointwise form;
  - tests/harness/decode_sample_check.cpp: the tile routine (decode_sample.h) tile by tile from the host-built table against
    decode_row_batch of the whole image followed by the definition in plain C++, as sequential code under the address and
    undefined-behaviour sanitizers.  It would catch: a tap index or weight one off; the wrong edge rule; a block decoded into
    the wrong slot of a batch; a tap evaluated against a batch that does not hold its block; a list overrun at 256 blocks; a
    write into padding or between planes; a coordinate read from a row's padding;
  - the table builder on hand-computed cases: tile shapes, tiles per grid, first[];
  - the ctypes structures and enums against the C ones, the argument checks that need no context, sample_grid on torch views;
  - the code object of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import sample_model as S
import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_sample_check.cpp")

# LDS of a workgroup of astc_decode_sample: DecodeBatch (7040 B) and the list of a batch's 32 block indices, nothing else
LDS_BOUND = 7040 + 32 * 4

MODES = (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER)


def addressed(filter, mode, u, size):
    """[(texel index or None, weight)] of coordinate u along an axis of `size` texels."""
    return [(S.address(mode, i, size), float(w)) for i, w in S.axis_taps(filter, u)]


def test_model_taps_at_the_edges_and_special_coordinates():
    size = 10
    # x = 0.5: the centre of texel 0 -- one tap with either filter, under every mode
    for mode in MODES:
        assert addressed(S.NEAREST, mode, 0.5, size) == [(0, 1.0)]
        assert addressed(S.BILINEAR, mode, 0.5, size) == [(0, 1.0)]
    # x = 0.0 and -0.0: NEAREST is texel 0; BILINEAR has t = -0.5, taps -1 and 0 with weights 1/2 and 1/2
    for x in (0.0, -0.0):
        for mode in MODES:
            assert addressed(S.NEAREST, mode, x, size) == [(0, 1.0)]
        assert addressed(S.BILINEAR, S.CLAMP, x, size) == [(0, 0.5), (0, 0.5)]
        assert addressed(S.BILINEAR, S.REPEAT, x, size) == [(9, 0.5), (0, 0.5)]
        assert addressed(S.BILINEAR, S.MIRROR, x, size) == [(0, 0.5), (0, 0.5)]
        assert addressed(S.BILINEAR, S.BORDER, x, size) == [(None, 0.5), (0, 0.5)]
    # x = S - 0.5: the centre of the last texel
    for mode in MODES:
        assert addressed(S.NEAREST, mode, 9.5, size) == [(9, 1.0)]
        assert addressed(S.BILINEAR, mode, 9.5, size) == [(9, 1.0)]
    # x = S: NEAREST is index S, outside; BILINEAR has taps S - 1 and S with weights 1/2
    assert [addressed(S.NEAREST, m, 10.0, size) for m in MODES] == [[(9, 1.0)], [(0, 1.0)], [(9, 1.0)], [(None, 1.0)]]
    assert addressed(S.BILINEAR, S.CLAMP, 10.0, size) == [(9, 0.5), (9, 0.5)]
    assert addressed(S.BILINEAR, S.REPEAT, 10.0, size) == [(9, 0.5), (0, 0.5)]
    assert addressed(S.BILINEAR, S.MIRROR, 10.0, size) == [(9, 0.5), (9, 0.5)]
    assert addressed(S.BILINEAR, S.BORDER, 10.0, size) == [(9, 0.5), (None, 0.5)]
    # x = 1e-30: NEAREST is texel 0; BILINEAR: t = 1e-30 - 0.5 rounds to -0.5 in binary64, so it is the case x = 0
    assert float(np.float64(np.float32(1e-30)) - 0.5) == -0.5
    assert addressed(S.NEAREST, S.BORDER, 1e-30, size) == [(0, 1.0)]
    assert addressed(S.BILINEAR, S.REPEAT, 1e-30, size) == [(9, 0.5), (0, 0.5)]
    # x = -3.25: NEAREST index -4; BILINEAR: t = -3.75, i0 = -4, f = 0.25: taps -4 (3/4) and -3 (1/4)
    assert [addressed(S.NEAREST, m, -3.25, size) for m in MODES] == [[(0, 1.0)], [(6, 1.0)], [(3, 1.0)], [(None, 1.0)]]
    assert addressed(S.BILINEAR, S.CLAMP, -3.25, size) == [(0, 0.75), (0, 0.25)]
    assert addressed(S.BILINEAR, S.REPEAT, -3.25, size) == [(6, 0.75), (7, 0.25)]
    assert addressed(S.BILINEAR, S.MIRROR, -3.25, size) == [(3, 0.75), (2, 0.25)]
    assert addressed(S.BILINEAR, S.BORDER, -3.25, size) == [(None, 0.75), (None, 0.25)]
    # MIRROR over several periods: ... 1 0 | 0 1 2 | 2 1 0 | 0 1 2 ...
    assert [S.address(S.MIRROR, i, 3) for i in range(-7, 8)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert [S.address(S.REPEAT, i, 3) for i in range(-4, 5)] == [2, 0, 1, 2, 0, 1, 2, 0, 1]


def random_texels(seed):
    rng = np.random.default_rng(seed)
    u8 = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    f16 = rng.integers(0, 0x7C00, size=(5, 7, 4), dtype=np.uint16).view(np.float16)          # every finite non-negative half, subnormals included
    f16[1, 2, 0] = np.inf
    f16[3, 3, 1] = np.nan
    f32 = rng.integers(0, 0x7F800000, size=(5, 7, 4), dtype=np.uint32).view(np.float32)
    return u8, f16, f32


def test_model_texel_centres_reproduce_the_texels():
    """NEAREST anywhere inside a texel and BILINEAR at its centre: the texel itself, so the tensors call's model says the same."""
    ys, xs = np.meshgrid(np.arange(5), np.arange(7), indexing="ij")
    centres = np.stack([xs + 0.5, ys + 0.5], axis=-1).astype(np.float32)
    inside = np.stack([xs + 0.99, ys + 0.01], axis=-1).astype(np.float32)
    for texels in random_texels(5):
        want = texels.astype(np.float32)
        for filt, coords in ((S.NEAREST, centres), (S.BILINEAR, centres), (S.NEAREST, inside)):
            for mode in MODES:
                got = S.sample(texels, filt, mode, mode, coords)
                assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
                assert np.array_equal(np.isnan(got), np.isnan(want))
                one, zero = [0.5, 3.0, 1.0, 2.0], [1.0, 0.0, -4.0, 0.25]
                assert np.array_equal(S.tensor(texels, filt, mode, mode, coords, M.F16, M.PLANAR, 3, one, zero),
                                      M.tensor(texels[None], M.F16, M.PLANAR, 3, one, zero)[:, 0])


def test_model_zero_weight_tap_is_not_read():
    row = np.array([[1.0, np.nan, np.inf, 2.0]], dtype=np.float32)[..., None].repeat(4, axis=2)
    coords = np.array([[[0.5, 0.5], [1.5, 0.5], [2.5, 0.5], [3.5, 0.5]]], dtype=np.float32)
    for mode in MODES:
        got = S.sample(row, S.BILINEAR, mode, mode, coords)[0, :, 0]
        assert got[0] == 1.0 and np.isnan(got[1]) and got[2] == np.inf and got[3] == 2.0
    # ... and a quarter of a texel further the NaN is in the sum
    assert np.isnan(S.sample(row, S.BILINEAR, S.CLAMP, S.CLAMP, np.array([[[0.75, 0.5]]], dtype=np.float32))[0, 0, 0])
    # BORDER: a tap outside is +0.0 and part of the sum: at the corner (0, 0) a quarter of texel (0, 0)
    img = np.full((2, 2, 4), 8, dtype=np.uint8)
    assert S.sample(img, S.BILINEAR, S.BORDER, S.BORDER, np.array([[[0.0, 0.0]]], dtype=np.float32))[0, 0].tolist() == [2.0] * 4
    assert S.sample(img, S.BILINEAR, S.BORDER, S.CLAMP, np.array([[[0.0, 0.0]]], dtype=np.float32))[0, 0].tolist() == [4.0] * 4


def test_model_does_not_fuse_and_sums_x_before_y():
    """A coordinate of 2^-53 has t = 2^-53 - 1/2 (exact), i0 = -1 and f = 1/2 + 2^-53: tap 0 is index -1 with weight a = 1/2 - 2^-53,
    tap 1 is index 0 with weight b = 1/2 + 2^-53 -- weights of 53 significant bits, whose products with a binary32 round."""
    tiny = np.float32(2.0 ** -53)
    a, b = 0.5 - 2.0 ** -53, 0.5 + 2.0 ** -53
    assert [(i, float(w)) for i, w in S.axis_taps(S.BILINEAR, tiny)] == [(-1, a), (0, b)]
    # Fusing.  One column (x = 0.5: one x tap), two rows under REPEAT: index -1 is row 1 = v, index 0 is row 0 = -v, v = 1 + 2^-22.
    # a v = 1/2 + 2^-23 - 2^-53 - 2^-75 and b v = 1/2 + 2^-23 + 2^-53 + 2^-75 each lose their last term to rounding, so the sum of
    # the two products is -2^-52; with the second product fused into the sum its 2^-75 survives: -2^-52 (1 + 2^-23), the next binary32
    v = float(np.float32(1.0 + 2.0 ** -22))
    img = np.zeros((2, 1, 4), dtype=np.float32)
    img[1, 0, 0], img[0, 0, 0] = v, -v
    got = S.sample(img, S.BILINEAR, S.CLAMP, S.REPEAT, np.array([[[0.5, tiny]]], dtype=np.float32))[0, 0, 0]
    assert a * v == 0.5 + 2.0 ** -23 - 2.0 ** -53 and b * v == 0.5 + 2.0 ** -23 + 2.0 ** -53
    assert got == np.float32(-2.0 ** -52)
    fused = float(Fraction(b) * Fraction(-v) + Fraction(a * v))
    assert np.float32(fused) == np.float32(-2.0 ** -52 * (1.0 + 2.0 ** -23)) and np.float32(fused) != got
    # Order.  Both coordinates 2^-53 on a 2 x 2 image under REPEAT, row 0 all zero, row 1 = (3, -3): x first, the row sums are
    # r(1) = a (-3) + b 3 and r(0) = 0, and acc = a r(1) + b 0; y first, the column sums are a 3 and a (-3) and acc = a (a (-3)) + b (a 3)
    img = np.zeros((2, 2, 4), dtype=np.float32)
    img[1, :, 0] = (3.0, -3.0)
    got = S.sample(img, S.BILINEAR, S.REPEAT, S.REPEAT, np.array([[[tiny, tiny]]], dtype=np.float32))[0, 0, 0]
    x_first = a * (a * -3.0 + b * 3.0) + b * (a * 0.0 + b * 0.0)
    y_first = a * (a * -3.0 + b * 0.0) + b * (a * 3.0 + b * 0.0)
    assert got == np.float32(x_first) == np.float32(2.0 ** -51)
    assert np.float32(y_first) == np.float32(2.0 ** -52) and np.float32(y_first) != got


def test_model_invalid_points():
    img = np.full((3, 3, 4), 200, dtype=np.uint8)
    big = np.float32(2.0 ** 30)
    nxt = np.nextafter(big, np.float32(np.inf))
    assert S.valid(big, -big) and not S.valid(nxt, 0.0) and not S.valid(0.0, -nxt)
    assert not S.valid(np.nan, 0.0) and not S.valid(0.0, np.inf) and not S.valid(-np.inf, 0.0)
    coords = np.array([[[np.nan, 1.0], [1.0, np.inf], [-np.inf, 1.0], [big, 1.0], [nxt, 1.0], [1.0, -big], [1.0, -nxt]]], dtype=np.float32)
    for filt in (S.NEAREST, S.BILINEAR):
        got = S.sample(img, filt, S.REPEAT, S.MIRROR, coords)[0, :, 0].tolist()
        assert got == [0.0, 0.0, 0.0, 200.0, 0.0, 200.0, 0.0]
        assert not np.signbit(S.sample(img, filt, S.REPEAT, S.MIRROR, coords)).any()
    # an invalid point goes through scale and bias like any other: bias alone
    bits = S.convert(img, S.NEAREST, S.CLAMP, S.CLAMP, coords, M.F32, 2, [2.0, 2.0, 1.0, 1.0], [0.5, -1.0, 0.0, 0.0])
    assert bits[0, 0, 0].view(np.float32).tolist() == [0.5, -1.0] and bits[0, 0, 3].view(np.float32).tolist() == [400.5, 399.0]
    # 2^30 under BORDER lies outside: +0.0 from the taps, not from the validity rule
    assert S.sample(img, S.NEAREST, S.BORDER, S.BORDER, coords)[0, 3, 0] == 0.0


def test_model_array_form_is_the_pointwise_form():
    rng = np.random.default_rng(11)
    special = np.array([0.5, 0.0, -0.0, 6.5, 7.0, 1e-30, -3.25, np.nan, np.inf, 2.0 ** 30, -2.0 ** 30, 4.5, 5.0, -0.5], dtype=np.float32)
    grid = np.stack(np.meshgrid(special, special, indexing="xy"), axis=-1)
    rand = rng.uniform(-9.0, 16.0, size=(9, 13, 2)).astype(np.float32)
    for texels in random_texels(6):
        for filt in (S.NEAREST, S.BILINEAR):
            for ax, ay in ((S.CLAMP, S.BORDER), (S.REPEAT, S.MIRROR), (S.MIRROR, S.REPEAT), (S.BORDER, S.CLAMP)):
                for coords in (grid, rand):
                    a = S.sample(texels, filt, ax, ay, coords)
                    b = S.sample_pointwise(texels, filt, ax, ay, coords)
                    assert np.array_equal(np.isnan(a), np.isnan(b))
                    assert np.array_equal(a.view(np.uint32)[~np.isnan(a)], b.view(np.uint32)[~np.isnan(b)])


def test_model_tile_shapes():
    assert [S.tile_shape(n) for n in (1, 2, 3, 4, 5, 8, 9, 65535)] == [(64, 1), (32, 2), (16, 4), (16, 4), (8, 8), (8, 8), (8, 8), (8, 8)]
    assert S.tiles(65535, 65535) == 8192 * 8192 and 64 * S.tiles(65535, 65535) == 2 ** 32
    assert (S.tiles(64, 1), S.tiles(65, 1), S.tiles(33, 2), S.tiles(17, 3), S.tiles(9, 5), S.tiles(20, 17)) == (1, 2, 2, 2, 2, 9)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_sample") / "decode_sample_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tile_routine_matches_decode_sample_convert_place_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # four footprints x four profiles x three data types x two filters x six formats (every tensor type with both layouts), and
    # the corner grid of every footprint
    assert int(re.search(r"^(\d+) configurations", out.stdout, re.M).group(1)) == 4 * 4 * 3 * 2 * 6 + 4
    assert "address mode pairs met: 16 of 16" in out.stdout
    # 256 distinct blocks in one tile: eight full batches
    for name in ("4x4", "6x6", "10x8", "12x12"):
        assert "%s corners: tiles 1 batches 8 blocks 256" % name in out.stdout, out.stdout


def test_blocks_mode_counts_what_the_tiles_decode(harness, tmp_path):
    """6x6, 120 x 60 image, 16 x 5 grid (two 8 x 8 tiles across, one down).  Tile 0: every point at the centre of texel (0, 0):
    one block, one batch.  Tile 1: rows 0 .. 3 at the corner (6, 6) -- taps in blocks (0, 0), (1, 0), (0, 1), (1, 1) -- and row 4
    at (60.5, 30.5): block (10, 5).  Five blocks, one batch."""
    coords = np.zeros((5, 16, 2), dtype=np.float32)
    coords[:, :8] = (0.5, 0.5)
    coords[:4, 8:] = (6.0, 6.0)
    coords[4, 8:] = (60.5, 30.5)
    path = tmp_path / "coords.f32"
    coords.tofile(str(path))
    out = subprocess.run([harness, "blocks", "1", "0", "0", "6", "6", "120", "60", "16", "5", str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "tiles 2 batches 2 decoded 6 points 80"


def test_table_builder_on_hand_computed_cases(harness):
    """6x6 blocks.  Entry 0 is 230 x 50 x 2 U8, entry 1 is 100 x 30 F32; BILINEAR, MIRROR along x, BORDER along y, interleaved F16
    with three channels.  100 x 1 points: two 64 x 1 tiles; 33 x 2: two 32 x 2; 17 x 3: two 16 x 4; 9 x 5: two 8 x 8; 20 x 17:
    three across, three down."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    head = re.match(r"table: count (\d+) total (\d+) returned (\d+) first ([\d ]+) records (.*)$", lines[0])
    recs = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(5))]
    assert (int(head.group(1)), int(head.group(2)), int(head.group(3))) == (5, 17, 17)
    assert [int(v) for v in head.group(4).split()] == [0, 2, 4, 6, 8]
    fmt = dict(filter=1, address_x=2, address_y=3, type=1, layout=1, channels=3, x_step=3, plane=0)
    assert recs[0] == dict(tw=64, th=1, tiles_x=2, dim_x=230, data_type=0, z=1, out_x=100, out_y=1, coord_row=200, row=300, **fmt)
    assert recs[1] == dict(tw=32, th=2, tiles_x=2, dim_x=100, data_type=2, z=0, out_x=33, out_y=2, coord_row=70, row=99, **fmt)
    assert recs[2] == dict(tw=16, th=4, tiles_x=2, dim_x=230, data_type=0, z=0, out_x=17, out_y=3, coord_row=34, row=51, **fmt)
    assert recs[3] == dict(tw=8, th=8, tiles_x=2, dim_x=100, data_type=2, z=0, out_x=9, out_y=5, coord_row=18, row=27, **fmt)
    assert recs[4] == dict(tw=8, th=8, tiles_x=3, dim_x=230, data_type=0, z=1, out_x=20, out_y=17, coord_row=40, row=64, **fmt)
    # the kernel's taps along an axis of 10 texels are the model's, for the hand-checked coordinates under each address mode
    seen = 0
    for line in lines[1:]:
        m = re.match(r"taps (\S+) filter (\d) mode (\d):(.*)$", line)
        x, filt, mode = float.fromhex(m.group(1)), int(m.group(2)), int(m.group(3))
        got = [(int(k), float.fromhex(w)) for k, w in re.findall(r"\[(-?\d+) (\S+)\]", m.group(4))]
        want = [(-1 if k is None else k, w) for k, w in addressed(filt, mode, x, 10)]
        assert got == want, line
        seen += 1
    assert seen == 7 * 2 * 4


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    body = ""
    for cname, cls in (("astcenc_amd_sample_grid", A.SampleGrid), ("astcenc_amd_sampler", A.Sampler)):
        body += '  printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body +
                     '  printf("%d %d %zu\\n", ASTCENC_AMD_SAMPLE_NEAREST, ASTCENC_AMD_SAMPLE_BILINEAR, sizeof(enum astcenc_amd_sample_filter));\n'
                     '  printf("%d %d %d %d %zu\\n", ASTCENC_AMD_ADDRESS_CLAMP, ASTCENC_AMD_ADDRESS_REPEAT, ASTCENC_AMD_ADDRESS_MIRROR, ASTCENC_AMD_ADDRESS_BORDER,\n'
                     '         sizeof(enum astcenc_amd_sample_address));\n  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, cls in zip(lines, (A.SampleGrid, A.Sampler)):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in A.SampleGrid._fields_] == ["entry", "z", "out_x", "out_y", "coords", "coord_row_pitch", "out", "row_pitch", "plane_pitch"]
    assert [f for f, _ in A.Sampler._fields_] == ["filter", "address_x", "address_y"]
    assert [int(v) for v in lines[2].split()] == [A.SAMPLE_NEAREST, A.SAMPLE_BILINEAR, C.sizeof(C.c_int)]
    assert [int(v) for v in lines[3].split()] == [A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, A.ADDRESS_MIRROR, A.ADDRESS_BORDER, C.sizeof(C.c_int)]
    assert (S.NEAREST, S.BILINEAR) == (A.SAMPLE_NEAREST, A.SAMPLE_BILINEAR)
    assert (S.CLAMP, S.REPEAT, S.MIRROR, S.BORDER) == (A.ADDRESS_CLAMP, A.ADDRESS_REPEAT, A.ADDRESS_MIRROR, A.ADDRESS_BORDER)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_tensors_device
    assert "astcenc_amd_sample_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.Sampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP)
    grid = (A.SampleGrid * 1)(A.SampleGrid(0, 0, 2, 2, None, 0, None, 0, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_sample_grid_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((8, 40, 50, 2), dtype=torch.float32)
    g = A.sample_grid(2, 1, coords[3], batch[3])
    assert (g.entry, g.z, g.out_x, g.out_y) == (2, 1, 50, 40)
    assert (g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (coords[3].data_ptr(), 100, batch[3].data_ptr(), 50, 2000)
    # a tile of both
    cv, ov = coords[1, 4:14, 8:28], batch[1, :, 4:14, 8:28]
    g = A.sample_grid(0, 0, cv, ov)
    assert (g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (20, 10, cv.data_ptr(), 100, ov.data_ptr(), 50, 2000)
    # [H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    g = A.sample_grid(0, 0, cv, nhwc[2, 4:14, 8:28], layout=A.TENSOR_INTERLEAVED, type=A.TENSOR_BF16)
    assert (g.out_x, g.out_y, g.row_pitch, g.plane_pitch) == (20, 10, 200, 0)
    # one row of points: a list; the pitches of an axis of length one are the tight ones
    pts = torch.zeros((1, 1000, 2), dtype=torch.float32)
    g = A.sample_grid(0, 0, pts, torch.zeros((3, 1, 1000), dtype=torch.float32), type=A.TENSOR_F32)
    assert (g.out_x, g.out_y, g.coord_row_pitch, g.row_pitch) == (1000, 1, 0, 0)
    # explicit pointers and pitches
    g = A.sample_grid(1, 3, (4096, 6, 7, 64), (8192, 16, 9000))
    assert (g.entry, g.z, g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (1, 3, 6, 7, 4096, 64, 8192, 16, 9000)


def test_sample_grid_rejects_what_the_call_cannot_express(A):
    torch = pytest.importorskip("torch")
    out = torch.zeros((3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((40, 50, 2), dtype=torch.float32)
    wide = torch.zeros((40, 50, 4), dtype=torch.float32)
    nhwc = torch.zeros((40, 50, 4), dtype=torch.float16)
    bad = [
        (coords.double(), out, A.TENSOR_PLANAR),                           # float64 coordinates
        (coords.half(), out, A.TENSOR_PLANAR),
        (torch.zeros((40, 50, 3)), out, A.TENSOR_PLANAR),                  # triples
        (torch.zeros((40, 100)), out, A.TENSOR_PLANAR),                    # two dimensions
        (wide[:, :, :2], out, A.TENSOR_PLANAR),                            # pairs four floats apart
        (wide[:, :, ::2], out, A.TENSOR_PLANAR),                           # x and y not adjacent
        (torch.zeros((50, 40, 2)).permute(1, 0, 2), out, A.TENSOR_PLANAR), # transposed: columns a row apart
        (coords[:, :49], out, A.TENSOR_PLANAR),                            # another width than the output's
        (coords[:39], out, A.TENSOR_PLANAR),                               # another height
        (coords[:1].expand(40, 50, 2), out, A.TENSOR_PLANAR),              # one row seen as forty
        (torch.zeros((40 * 50 * 2 + 1,))[1:].view(40, 50, 2), out, A.TENSOR_PLANAR),                         # not on 8 bytes
        (torch.zeros((40 * 101,)).as_strided((40, 50, 2), (101, 2, 1)), out, A.TENSOR_PLANAR),               # rows an odd number of floats apart
        # the output: what scaled_region rejects
        (coords, out.transpose(1, 2).contiguous().transpose(1, 2), A.TENSOR_PLANAR),                         # columns a row apart
        (coords[:, :25].contiguous(), out[:, :, 0:50:2], A.TENSOR_PLANAR),
        (coords, nhwc[:, :, :3], A.TENSOR_INTERLEAVED),
        (coords, out[0], A.TENSOR_PLANAR),
        (coords, out[:1].expand(3, 40, 50), A.TENSOR_PLANAR),
    ]
    for c, o, layout in bad:
        with pytest.raises(ValueError):
            A.sample_grid(0, 0, c, o, layout=layout)
    for type, dtype in ((A.TENSOR_F32, torch.float16), (A.TENSOR_F16, torch.bfloat16), (A.TENSOR_BF16, torch.float32)):
        with pytest.raises(ValueError):
            A.sample_grid(0, 0, coords, torch.zeros((3, 40, 50), dtype=dtype), type=type)
    assert A.sample_grid(0, 0, coords, out, type=A.TENSOR_F16).out_x == 50


def test_sample_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    sample = {n: d for n, d in by_short.items() if n.startswith("astc_decode_sample")}
    # one build per tensor type and layout
    assert len(sample) == 6, sorted(by_short)
    for name, d in sample.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["group_segment_fixed_size"] <= LDS_BOUND, (name, d)
        # the names the other code-object tests pick kernels by do not match the new ones
        assert not name.startswith(("astc_decode_regions", "astc_decode_tensors", "astc_decode_scaled", "astc_decompress_blocks", "astc_decompress_set", "astc_compare_"))
