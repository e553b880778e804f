# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_cube_tensors_device (compressed cube maps sampled by direction at a level of detail per point): what can be
checked without a GPU.

  - the numpy model (tests/sample_cube_model.py) on hand-made cases: the face table, the ties, the consequence on power-of-two
    faces, scaling by a power of two, a corner and an edge worked out by hand;
  - the conditions the constructed directions must reach, asserted on the model: all 24 (face, side) pairs, all 24 (face, corner
    quadrant) pairs, a second tap of weight zero on each axis, both branches of every tie;
  - tests/harness/decode_cube_check.cpp, a g++ build of decode_cube.h under the address and undefined-behaviour sanitizers, run as
    a program of its own: the coordinate stage function by function against the model (`points`), and whole tiles through
    decode_cube_tile from the host-built table, bit for bit against the model applied to decode_row_batch of every whole level
    (`tiles`): the three tile shapes, cube 1 of two, chains of five levels, both filters and mip filters, the six store builds;
  - the ctypes structures against the C ones, the argument checks that need no context, cube_grid on torch views;
  - the code object of the new kernels: six builds, no scratch, 7168 B of LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mip_cube_model as Q
import sample_cube_model as K
import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_cube_check.cpp")
SIZES = (1, 2, 3, 5, 8, 64)
FILTERS = (K.NEAREST, K.BILINEAR)
MIPS = (K.MIP_NEAREST, K.MIP_LINEAR)
# the harness's format
SCALE = [float(np.float32(v)) for v in (0.017124754, -0.5, 3.0, 0.00390625)]
BIAS = [float(np.float32(v)) for v in (-2.1179039, 0.25, 100.0, 0.0)]
GUARD = 0xA5


def test_model_face_table_and_ties():
    # the six axes select their faces; (sc, tc) are the header's table
    table = {0: lambda x, y, z: (-z, -y), 1: lambda x, y, z: (z, -y), 2: lambda x, y, z: (x, z), 3: lambda x, y, z: (x, -z), 4: lambda x, y, z: (x, -y),
             5: lambda x, y, z: (-x, -y)}
    rng = np.random.default_rng(1)
    seen = set()
    for d in rng.uniform(-1, 1, size=(200, 3)).astype(np.float32):
        f, sc, tc, ma = K.face_of(d)
        axis = int(np.argmax(np.abs(d)))
        assert f == 2 * axis + (d[axis] < 0) and ma == abs(d[axis])
        assert (sc, tc) == table[f](*d)
        seen.add(f)
    assert seen == set(range(6))
    for f in range(6):
        assert K.face_of(Q.MAJOR[f])[0] == f
    # ties: x before y before z
    assert K.face_of((1, 1, 0))[0] == 0 and K.face_of((-1, 1, 1))[0] == 1 and K.face_of((1, -1, -1))[0] == 0
    assert K.face_of((0, 1, 1))[0] == 2 and K.face_of((0, -1, 1))[0] == 3 and K.face_of((1, 0, 1))[0] == 0 and K.face_of((-1, 0, 1))[0] == 1
    assert K.face_of((0.5, 1, 1))[0] == 2 and K.face_of((1, 1, 2))[0] == 4 and K.face_of((1, 1, -2))[0] == 5
    # zeros of either sign are zeros; the zero vector and non-finite components are invalid, a NaN lambda' too
    assert K.valid((0.0, -0.0, 1e-45), 0.0) and not K.valid((0.0, -0.0, -0.0), 0.0) and not K.valid((np.nan, 1, 1), 0.0)
    assert not K.valid((1, np.inf, 1), 0.0) and not K.valid((1, 1, -np.inf), 0.0) and not K.valid((1, 1, 1), np.nan) and K.valid((3e38, -3e38, 3e38), np.inf)
    f, sc, tc, ma = K.face_of((-0.0, 0.0, -2.0))
    assert (f, float(ma)) == (5, 2.0) and np.signbit(sc) == False and np.signbit(tc) == True  # noqa: E712  (-dx = +0.0, -dy = -0.0)


def cube_level(seed, s, cubes=2, dtype=np.float32):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(6 * cubes, s, s, 4), dtype=np.uint8)
    return rng.uniform(-4, 4, size=(6 * cubes, s, s, 4)).astype(dtype)


def test_model_texel_centres_reproduce_the_texels_on_power_of_two_faces():
    for s in (1, 2, 8, 16):
        level = cube_level(s, s)
        for f in range(6):
            for y in range(s):
                for x in range(s):
                    d = Q.centre(f, x, y, s)
                    assert np.array_equal(np.array(d, dtype=np.float32), K.direction(f, x + 0.5, y + 0.5, s))
                    ff, sc, tc, ma = K.face_of(d)
                    p, q = K.quotients(sc, tc, ma)
                    assert ff == f and (K.face_coordinate(p, s), K.face_coordinate(q, s)) == (x + 0.5, y + 0.5)
                    for filt in FILTERS:
                        for mip in MIPS:
                            got = K.sample_point([level], 1, filt, mip, d, None, 0.0)
                            assert np.array_equal(got, level[6 + f, y, x]), (s, f, x, y, filt)
    # scaling by a power of two gives the same bits, down into the subnormals and up to the largest exponents
    level = [cube_level(3, 5), cube_level(4, 2)]
    rng = np.random.default_rng(5)
    for d in rng.uniform(-1, 1, size=(40, 3)).astype(np.float32):
        want = K.sample_point(level, 0, K.BILINEAR, K.MIP_LINEAR, d, 0.25, 0.0)
        for e in (-100, 100):
            scaled = np.ldexp(d, e).astype(np.float32)
            assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), d.astype(np.float64))
            assert np.array_equal(K.sample_point(level, 0, K.BILINEAR, K.MIP_LINEAR, scaled, 0.25, 0.0), want)


def test_model_edge_and_corner_by_hand():
    """s = 4, face +X.  The direction through (0.25, 2.5): t = -0.25 along x, so the taps are indices -1 and 0 with weights 0.25
    and 0.75; -1 is the neighbour +Z (the header's list: x < 0 of +X is +Z) at depth 0, its column 3, the same row.  The direction
    through (0.25, 0.25) has a tap with both indices outside: the face's own corner texel, not an average."""
    s = 4
    level = cube_level(9, s, cubes=1)
    d = K.direction(0, 0.25, 2.5, s)
    want = (np.float64(0.25) * level[4, 2, 3].astype(np.float64) + np.float64(0.75) * level[0, 2, 0].astype(np.float64))
    want = (np.float64(1.0) * want).astype(np.float32)
    assert Q.source(0, -1, 2, s) == (4, 3, 2)
    assert np.array_equal(K.sample_point([level], 0, K.BILINEAR, K.MIP_NEAREST, d, None, 0.0), want)
    d = K.direction(0, 0.25, 0.25, s)
    f, sc, tc, ma = K.face_of(d)
    p, q = K.quotients(sc, tc, ma)
    rows = K.point_taps(K.BILINEAR, f, K.face_coordinate(p, s), K.face_coordinate(q, s), s)
    assert [[t[1] for t in row] for _, row in rows] == [[(0, 0, 0), Q.source(0, 0, -1, s)], [Q.source(0, -1, 0, s), (0, 0, 0)]]
    assert Q.source(0, 0, -1, s)[0] == 2 and Q.source(0, -1, 0, s)[0] == 4
    # NEAREST at x = s is the last texel, not the neighbour
    assert K.axis_taps(K.NEAREST, np.float64(s), s) == [(s - 1, 1.0)] and K.axis_taps(K.NEAREST, np.float64(0.0), s) == [(0, 1.0)]


@pytest.fixture(scope="module")
def constructed():
    return K.constructed_directions(SIZES)


def test_constructed_directions_reach_every_case(constructed):
    sides, quadrants, zero_axes, ties = K.coverage(constructed, SIZES)
    assert sides == {(f, k) for f in range(6) for k in range(4)}
    assert quadrants == {(f, k) for f in range(6) for k in range(4)}
    assert zero_axes == {"x", "y"}
    # both branches of every tie: the tie decides (the earlier axis wins), or a larger third component does
    assert ties == {("ab", True), ("ab>c", True), ("bc", True), ("bc<=a", True), ("ac", True), ("ac<b", True)}
    # every face is reached; invalid points of every kind are among the inputs
    assert {K.face_of(d)[0] for d in constructed if K.valid(d, 0.0)} == set(range(6))
    bad = [d for d in constructed if not K.valid(d, 0.0)]
    assert any(np.isnan(d).any() for d in bad) and any(np.isposinf(d).any() for d in bad) and any(np.isneginf(d).any() for d in bad)
    assert sum(1 for d in bad if not d.any()) == 8
    tiny = np.float32(1e-45)
    assert any(np.abs(d).max() == tiny for d in constructed) and any(np.abs(d).max() == np.float32(3e38) for d in constructed)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The harness as a program of its own under the sanitizers: no Python and no preload are involved in what it runs."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_cube") / "decode_cube_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_coordinate_stage_matches_the_model(harness, constructed, tmp_path):
    path = tmp_path / "dirs.f32"
    constructed.tofile(str(path))
    out = subprocess.run([harness, "points", str(path), str(len(constructed))], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    heads, taps = {}, {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "D":
            heads[int(w[1])] = w[2:]
        else:
            taps[(int(w[1]), int(w[2]), int(w[3]))] = w[4:]
    assert len(heads) == len(constructed)
    checked = 0
    for i, d in enumerate(constructed):
        h = heads[i]
        ok = K.valid(d, 0.0)
        assert (int(h[0]), int(h[1])) == (int(ok), 0), (i, d)
        if not ok:
            assert int(h[2]) == -1 and not any(k[0] == i for k in taps)
            continue
        f, sc, tc, ma = K.face_of(d)
        p, q = K.quotients(sc, tc, ma)
        assert int(h[2]) == f, (i, d)
        got = [float.fromhex(v) for v in h[3:8]]
        want = [float(sc), float(tc), float(ma), float(p), float(q)]
        assert got == want and [np.signbit(v) for v in got] == [np.signbit(v) for v in want], (i, d, got, want)
        assert abs(p) <= 1.0 and abs(q) <= 1.0
        for s in SIZES:
            x, y = K.face_coordinate(p, s), K.face_coordinate(q, s)
            assert 0.0 <= x <= s and 0.0 <= y <= s
            for filt in FILTERS:
                w = taps[(i, s, filt)]
                assert (float.fromhex(w[0]), float.fromhex(w[1])) == (float(x), float(y)), (i, d, s)
                rows = K.point_taps(filt, f, x, y, s)
                assert (int(w[2]), int(w[3])) == (len(rows[0][1]), len(rows)), (i, d, s, filt)
                wx = [float(t[0]) for t in rows[0][1]]
                wy = [float(r[0]) for r in rows]
                assert [float.fromhex(v) for v in w[4:4 + len(wx)]] == wx and [float.fromhex(v) for v in w[6:6 + len(wy)]] == wy
                slots = [tuple(int(v) for v in w[8 + 3 * t:11 + 3 * t]) for t in range(4)]
                want_slots = [(-1, -1, -1)] * 4
                for b, (_, row) in enumerate(rows):
                    for a, (_, texel, _) in enumerate(row):
                        want_slots[2 * b + a] = texel
                assert slots == want_slots, (i, d, s, filt, slots, want_slots)
                checked += 1
    assert checked == sum(1 for d in constructed if K.valid(d, 0.0)) * len(SIZES) * 2


def spanning_directions(rng, n):
    """Directions near a cube corner and along its edges, so that the taps of one tile lie on three faces; then anywhere."""
    near = np.array([1.0, 1.0, 1.0], dtype=np.float32) + rng.uniform(-0.3, 0.3, size=(n // 2, 3)).astype(np.float32)
    anywhere = rng.normal(size=(n - n // 2, 3)).astype(np.float32)
    return np.concatenate([near, anywhere])


def run_tiles(harness, tmp_path, tag, block, profile, kind, seed, s0, levels, cube, filt, mip, fmt, dirs, lod, bias, pads):
    """One chain and one grid through the harness; returns (chain of [12, s, s, 4] arrays, output bits, per-tile counts, layout of
    the output buffer)."""
    ttype, layout, channels = fmt
    oy, ox = dirs.shape[:2]
    dpath, lpath, prefix = tmp_path / (tag + ".dirs"), tmp_path / (tag + ".lod"), str(tmp_path / tag)
    np.ascontiguousarray(dirs, dtype=np.float32).tofile(str(dpath))
    if lod is not None:
        np.ascontiguousarray(lod, dtype=np.float32).tofile(str(lpath))
    args = [harness, "tiles", block[0], block[1], profile, kind, seed, s0, levels, cube, filt, mip, ttype, layout, channels, ox, oy, dpath, lpath if lod is not None else "-",
            repr(float(bias)), pads, prefix]
    out = subprocess.run([str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    chain, tiles, shape = [], [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "level":
            l, s, t = int(w[1]), int(w[2]), int(w[3])
            chain.append(np.fromfile(prefix + ".level%d" % l, dtype=(np.uint8, np.float16, np.float32)[t]).reshape(12, s, s, 4))
        elif w[0] == "out":
            shape = tuple(int(v) for v in w[1:])
        elif w[0] == "tile":
            tiles.append(tuple(int(v) for v in w[2:]))
    got = np.fromfile(prefix + ".out", dtype=np.uint8).view(M.BITS_DTYPE[ttype])
    return chain, got, tiles, shape


def check_tiles(harness, tmp_path, tag, block, profile, kind, seed, s0, levels, cube, filt, mip, fmt, dirs, lod, bias, pads):
    chain, got, tiles, (guard, row, plane, elements) = run_tiles(harness, tmp_path, tag, block, profile, kind, seed, s0, levels, cube, filt, mip, fmt, dirs, lod, bias, pads)
    ttype, layout, channels = fmt
    oy, ox = dirs.shape[:2]
    assert [c.shape[1] for c in chain] == [max(1, s0 >> l) for l in range(levels)]
    element = 4 if ttype == M.F32 else 2
    want = np.full(got.size * element, GUARD, dtype=np.uint8).view(M.BITS_DTYPE[ttype])
    bits = K.convert(chain, cube, filt, mip, dirs, lod, bias, ttype, channels, SCALE, BIAS)
    M.scatter(want, guard // element, bits, layout, 0, row, row * oy, plane)
    assert np.array_equal(got, want), (tag, int((got != want).sum()), int(np.argwhere(got != want)[0][0]) - guard // element)
    # as many tiles as the grid's size needs; no pass lists more than 256 blocks; a tile has at most as many passes as the chain
    # has levels
    th = 8 if oy >= 5 else 4 if oy >= 3 else oy
    tw = 64 // th
    assert len(tiles) == -(-ox // tw) * -(-oy // th)
    for passes, batches, blocks, mask, most in tiles:
        assert passes == bin(mask).count("1") <= levels and most <= 256 and most <= blocks <= most * passes and batches * 32 >= blocks
    return chain, tiles


def lods(rng, shape, levels):
    lod = rng.uniform(-1.0, levels + 0.5, size=shape).astype(np.float32)
    flat = lod.reshape(-1)
    special = np.array([0.0, 1.0, levels - 1.0, np.inf, -np.inf, 0.5, 1.5, np.nan, -0.0, 2.0], dtype=np.float32)
    flat[:len(special)] = special[:flat.size]
    return lod


FORMATS = [(M.F16, M.PLANAR, 3), (M.BF16, M.INTERLEAVED, 4), (M.F32, M.INTERLEAVED, 1), (M.F32, M.PLANAR, 4), (M.F16, M.INTERLEAVED, 3), (M.BF16, M.PLANAR, 1)]
SHAPES = [(70, 1), (19, 3), (19, 11)]          # 64 x 1, 16 x 4, 8 x 8 tiles, each with a partial tile


@pytest.mark.parametrize("block", [(4, 4), (6, 6), (8, 5), (12, 12)])
def test_whole_tiles_match_the_model(harness, constructed, tmp_path, block):
    """Chains of five levels (faces 20, 10, 5, 2, 1), two cubes in every level, cube 1 sampled (cube 0 once): the three tile shapes,
    both filters, both mip filters, the six store builds, the four kinds of chain and the profiles turning; seeded directions
    whose taps span three faces in one tile, and the constructed directions as one grid."""
    rng = np.random.default_rng(block[0] * 16 + block[1])
    turn = block[0] + block[1]
    three_faces = False
    for k, (ox, oy) in enumerate(SHAPES):
        for filt in FILTERS:
            for mip in MIPS:
                n = turn + 4 * k + 2 * filt + mip
                dirs = spanning_directions(rng, ox * oy).reshape(oy, ox, 3)
                lod = lods(rng, (oy, ox), 5) if n % 4 else None
                fmt = FORMATS[n % 6]
                cube = 0 if n % 7 == 3 else 1
                chain, tiles = check_tiles(harness, tmp_path, "t%d" % n, block, n % 4, n % 4 if n % 3 else 3, n, 20, 5, cube, filt, mip, fmt, dirs, lod, 0.25 * (n % 3), n % 8)
                if filt == K.BILINEAR:
                    # (the first tile's points near the corner (1, 1, 1): +X, +Y and +Z)
                    faces = set()
                    tw = 64 // (8 if oy >= 5 else 4 if oy >= 3 else oy)
                    for d in dirs[:min(oy, 8), :tw].reshape(-1, 3):
                        f, sc, tc, ma = K.face_of(d)
                        p, q = K.quotients(sc, tc, ma)
                        faces |= {t[1][0] for _, row in K.point_taps(filt, f, K.face_coordinate(p, 20), K.face_coordinate(q, 20), 20) for t in row}
                    three_faces = three_faces or len(faces) >= 3
    assert three_faces
    # the constructed directions, invalid ones included, under both filters; lambda' from the bias alone and from a lod
    n = len(constructed)
    grid = np.concatenate([constructed, np.tile(constructed[:1], (-n % 19, 1))]).reshape(-1, 19, 3)
    check_tiles(harness, tmp_path, "c0", block, 0, 3, 1, 20, 5, 1, K.BILINEAR, K.MIP_LINEAR, (M.F32, M.PLANAR, 4), grid, None, 1.5, 2)
    check_tiles(harness, tmp_path, "c1", block, 3, 1, 2, 16, 5, 1, K.NEAREST, K.MIP_NEAREST, (M.F16, M.PLANAR, 3), grid, lods(rng, grid.shape[:2], 5), 0.0, 5)


def test_a_chain_of_one_level_and_a_nan_behind_a_weight_of_zero(harness, tmp_path):
    """A cube without mips (one level, lod NULL); and, under the HDR profile with F16 levels, reserved-mode blocks decode to NaN: the
    directions through texel centres (fr = 0 on both axes) read one texel each, so a NaN reaches a point only from its own texel --
    the model, which leaves zero weights out, has compared every bit -- and integer lambda' leaves the other level unread."""
    rng = np.random.default_rng(3)
    dirs = spanning_directions(rng, 33 * 3).reshape(3, 33, 3)
    check_tiles(harness, tmp_path, "one", (6, 6), 0, 0, 7, 20, 1, 1, K.BILINEAR, K.MIP_LINEAR, (M.F16, M.PLANAR, 3), dirs, None, 0.0, 0)
    s = 16
    centres = np.array([[K.direction(f, x + 0.5, y + 0.5, s) for x in range(s)] for f in range(6) for y in range(s)], dtype=np.float32)
    lod = np.where(rng.integers(0, 2, size=centres.shape[:2]) == 1, np.float32(2.0), np.float32(0.0)).astype(np.float32)
    chain, _ = check_tiles(harness, tmp_path, "nan", (4, 4), 3, 1, 11, s, 3, 1, K.BILINEAR, K.MIP_LINEAR, (M.F32, M.INTERLEAVED, 4), centres, lod, 0.0, 3)
    assert np.isnan(chain[0].astype(np.float32)).any() and not np.isnan(chain[0].astype(np.float32)).all()


def test_blocks_mode_counts_passes_batches_and_blocks(harness, tmp_path):
    """6x6, faces of 24 texels and two levels, BILINEAR, MIP_LINEAR, a 16 x 5 grid (two 8 x 8 tiles).  Tile 0: the axis +X at
    lambda 0: one pass; the centre (12, 12) is a block corner: four blocks of face +X.  Tile 1: the cube corner (1, 1, 1) at
    lambda 0.5: on +X (the tie) at (0, 0): taps (-1, -1), (0, -1), (-1, 0), (0, 0): the face's own corner texel, +Y's and +Z's:
    three blocks a level on two levels."""
    dirs = np.zeros((5, 16, 3), dtype=np.float32)
    dirs[:, :8] = (1.0, 0.0, 0.0)
    dirs[:, 8:] = (1.0, 1.0, 1.0)
    lod = np.zeros((5, 16), dtype=np.float32)
    lod[:, 8:] = 0.5
    dpath, lpath = tmp_path / "b.dirs", tmp_path / "b.lod"
    dirs.tofile(str(dpath))
    lod.tofile(str(lpath))
    out = subprocess.run([harness, "blocks", "1", "1", "6", "6", "24", "2", "16", "5", str(dpath), str(lpath)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "tiles 2 passes 3 batches 3 decoded 10 points 80"


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    body = ""
    for cname, cls in (("astcenc_amd_cube_grid", A.CubeGrid), ("astcenc_amd_cube_sampler", A.CubeSampler)):
        body += '  printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body + '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, cls in zip(lines, (A.CubeGrid, A.CubeSampler)):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in A.CubeGrid._fields_] == ["first_entry", "level_count", "cube", "out_x", "out_y", "dirs", "dir_row_pitch", "lod", "lod_row_pitch", "lod_bias",
                                                   "out", "row_pitch", "plane_pitch"]
    assert [f for f, _ in A.CubeSampler._fields_] == ["filter", "mip_filter"]
    if shutil.which("gcc"):
        c_probe = tmp_path / "probe.c"
        c_probe.write_text('#include "astcenc_amd.h"\nint main(void) { struct astcenc_amd_cube_sampler s; s.mip_filter = ASTCENC_AMD_MIP_LINEAR; return (int)s.mip_filter - 1; }\n')
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c_probe), "-o", str(tmp_path / "probe_c")], check=True)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_cube_tensors_device
    assert "astcenc_amd_sample_cube_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_cube_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 6, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.CubeSampler(A.SAMPLE_BILINEAR, A.MIP_LINEAR)
    grid = (A.CubeGrid * 1)(A.CubeGrid(0, 1, 0, 2, 2, None, 0, None, 0, 0.0, None, 0, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_cube_grid_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    dirs = torch.zeros((8, 40, 50, 3), dtype=torch.float32)
    lod = torch.zeros((8, 40, 50), dtype=torch.float32)
    g = A.cube_grid(2, 7, 1, dirs[3], lod[3], batch[3], lod_bias=-0.5)
    assert (g.first_entry, g.level_count, g.cube, g.out_x, g.out_y, g.lod_bias) == (2, 7, 1, 50, 40, -0.5)
    assert (g.dirs, g.dir_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (dirs[3].data_ptr(), 150, lod[3].data_ptr(), 50, batch[3].data_ptr(), 50, 2000)
    # a tile of all three: the directions need no alignment beyond the float's
    dv, lv, ov = dirs[1, 4:14, 7:27], lod[1, 4:14, 7:27], batch[1, :, 4:14, 7:27]
    g = A.cube_grid(0, 1, 0, dv, lv, ov)
    assert (g.out_x, g.out_y, g.dirs, g.dir_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (20, 10, dv.data_ptr(), 150, lv.data_ptr(), 50, ov.data_ptr(), 50, 2000)
    g = A.cube_grid(0, 3, 0, dv, None, ov, lod_bias=1.0)
    assert (g.lod, g.lod_row_pitch, g.lod_bias) == (None, 0, 1.0)
    # one row of points: a list
    g = A.cube_grid(0, 32, 0, torch.zeros((1, 1000, 3)), torch.zeros((1, 1000)), torch.zeros((3, 1, 1000)), type=A.TENSOR_F32)
    assert (g.out_x, g.out_y, g.dir_row_pitch, g.lod_row_pitch, g.row_pitch) == (1000, 1, 0, 0, 0)
    # explicit pointers and pitches
    g = A.cube_grid(1, 4, 1, (4100, 6, 7, 64), (12288, 8), (8192, 16, 9000), lod_bias=2.0)
    assert (g.first_entry, g.level_count, g.cube, g.out_x, g.out_y, g.dirs, g.dir_row_pitch, g.lod, g.lod_row_pitch, g.lod_bias, g.out, g.row_pitch, g.plane_pitch) == \
        (1, 4, 1, 6, 7, 4100, 64, 12288, 8, 2.0, 8192, 16, 9000)
    # what the call cannot express
    out = torch.zeros((3, 40, 50), dtype=torch.float16)
    d = torch.zeros((40, 50, 3), dtype=torch.float32)
    for bad in (dict(dirs=d.double()), dict(dirs=torch.zeros((40, 50, 2))), dict(dirs=torch.zeros((40, 50, 4))[:, :, :3]), dict(dirs=d[:, :49]),
                dict(dirs=d[:1].expand(40, 50, 3)), dict(lod=torch.zeros((40, 49))), dict(level_count=0), dict(level_count=33), dict(lod_bias=float("nan")),
                dict(out=out[0])):
        kw = dict(level_count=3, dirs=d, lod=None, out=out, lod_bias=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            A.cube_grid(0, kw["level_count"], 0, kw["dirs"], kw["lod"], kw["out"], lod_bias=kw["lod_bias"])


def test_cube_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    cube = {n: d for n, d in by_short.items() if n.startswith("astc_cube_sample")}
    # one build per tensor type and layout
    assert len(cube) == 6, sorted(by_short)
    for name, d in cube.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["group_segment_fixed_size"] == 7168, (name, d)
        # three waves per SIMD: 512 registers / 3, in allocation granules of 8
        assert d["vgpr_count"] <= 168, (name, d)
    # ... and the lod call's kernels are still its six
    assert len([n for n in by_short if n.startswith("astc_lod_sample")]) == 6
