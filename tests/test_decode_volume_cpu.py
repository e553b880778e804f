# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_sample_volume_tensors_device (compressed volumes sampled at (u, v, w), trilinear, at a level of detail per point):
what can be checked without a GPU.

  - the numpy model (tests/sample_volume_model.py) on hand-made cases: a trilinear point with eight distinct weights, a BORDER
    point with taps outside on z only, the one-z-tap consequence against sample_lod_model, texel centres on power-of-two volumes,
    and the array form against the pointwise form;
  - the conditions the generated grids (sample_volume_model.grid_inputs: what tests/test_decode_volume.py runs) must reach,
    asserted on the model: every address mode on every axis with taps outside on both sides, a second tap of weight zero on each
    axis separately, for the 3D footprints a point whose eight taps lie in one block and one whose taps lie in eight, a tile pass
    with more than DECODE_BATCH distinct blocks, MIP_LINEAR points blended and with g = 0, invalid points of every kind;
  - tests/harness/decode_volume_check.cpp, a g++ build of decode_volume.h under the address and undefined-behaviour sanitizers,
    run as a program of its own: the tap stage function by function against the model (`points`), and whole tiles through
    decode_volume_tile from the host-built table, bit for bit against the model applied to decode_row_batch of every whole level
    (`tiles`): the three tile shapes, chains of five levels, both filters and mip filters, the six store builds, one 2D and two
    3D footprints;
  - the ctypes structures against the C ones, the argument checks that need no context, volume_grid on torch views;
  - the code object of the new kernels: six builds, no scratch, 7168 B of LDS."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_lod_model as L
import sample_model as S
import sample_volume_model as K
import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_volume_check.cpp")
FILTERS = (S.NEAREST, S.BILINEAR)
MIPS = (L.MIP_NEAREST, L.MIP_LINEAR)
DECODE_BATCH = 32
# the harness's format
SCALE = [float(np.float32(v)) for v in (0.017124754, -0.5, 3.0, 0.00390625)]
BIAS = [float(np.float32(v)) for v in (-2.1179039, 0.25, 100.0, 0.0)]
GUARD = 0xA5


@pytest.fixture(autouse=True, scope="module")
def the_call_is_bound(A):
    """Everything here is about one entry point: without it in the binding no test of this file has a subject."""
    assert "astcenc_amd_sample_volume_tensors_device" in A.EXPORTS_AMD and hasattr(A, "volume_grid")


def volume(seed, dims, dtype=np.float32):
    W, H, D = dims
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(D, H, W, 4), dtype=np.uint8)
    return rng.uniform(-4, 4, size=(D, H, W, 4)).astype(dtype)


def test_model_trilinear_point_by_hand():
    """An 8 x 4 x 2 level, the point (0.34375, 0.4375, 0.40625): x = 2.75, y = 1.75, z = 0.8125, so t = 2.25, 1.25, 0.3125: taps
    (2, 3) with weights (0.75, 0.25), (1, 2) with (0.75, 0.25), (0, 1) with (0.6875, 0.3125) -- the eight products of weights are
    distinct once the axes differ; here the sums are spelled out in the defined order."""
    t = volume(1, (8, 4, 2))
    v = t.astype(np.float64)
    wx, wy, wz = (0.75, 0.25), (0.75, 0.25), (0.6875, 0.3125)
    planes = []
    for kz in (0, 1):
        rows = [wx[0] * v[kz, ky, 2] + wx[1] * v[kz, ky, 3] for ky in (1, 2)]
        planes.append(wy[0] * rows[0] + wy[1] * rows[1])
    want = (wz[0] * planes[0] + wz[1] * planes[1]).astype(np.float32)
    for address in ((S.CLAMP, S.REPEAT, S.BORDER), (S.MIRROR, S.MIRROR, S.CLAMP)):
        got = K.sample_point([t], S.BILINEAR, address, L.MIP_NEAREST, 0.34375, 0.4375, 0.40625, None, 0.0)
        assert np.array_equal(got, want)
    # eight distinct weights: a 16 x 8 x 4 level at x = 5.625, y = 3.75, z = 1.8125
    t = volume(2, (16, 8, 4))
    u, vv, w = 5.625 / 16, 3.75 / 8, 1.8125 / 4
    ax, ay, az = L.axis_taps(S.BILINEAR, 5.625), L.axis_taps(S.BILINEAR, 3.75), L.axis_taps(S.BILINEAR, 1.8125)
    assert len({float(a[1] * b[1] * c[1]) for a in ax for b in ay for c in az}) == 8
    assert [k for _, k in K.point_taps(t, S.BILINEAR, (0, 0, 0), u, vv, w)] == [(kx, ky, kz) for kz in (1, 2) for ky in (3, 4) for kx in (5, 6)]
    v = t.astype(np.float64)
    acc = None
    for iz, fz in az:
        p = None
        for iy, fy in ay:
            r = ax[0][1] * v[iz, iy, ax[0][0]] + ax[1][1] * v[iz, iy, ax[1][0]]
            p = fy * r if p is None else p + fy * r
        acc = fz * p if acc is None else acc + fz * p
    assert np.array_equal(K.sample_point([t], S.BILINEAR, (0, 0, 0), L.MIP_LINEAR, u, vv, w, 0.0, 0.0), acc.astype(np.float32))


def test_model_border_outside_on_z_only():
    """z = 0.25 of a level of depth 2: taps -1 and 0 with weights 0.25 and 0.75; under BORDER along z the plane of tap -1 is +0.0
    in every channel and is part of the sum, so the result is 0.25 * 0 + 0.75 * plane(0); under CLAMP it is plane(0) twice."""
    t = volume(3, (8, 4, 2))
    u, v, w = 2.75 / 8, 1.75 / 4, 0.125
    inner = K.sample_point([t[:1]], S.BILINEAR, (S.CLAMP, S.CLAMP, S.CLAMP), L.MIP_NEAREST, u, v, 0.5, None, 0.0).astype(np.float64)
    # (the slice alone at its centre has one z tap: `inner` is plane(0) rounded to binary32, so compare in binary64 from the taps)
    vals = t.astype(np.float64)
    rows = [0.75 * vals[0, ky, 2] + 0.25 * vals[0, ky, 3] for ky in (1, 2)]
    plane0 = 0.75 * rows[0] + 0.25 * rows[1]
    assert np.array_equal(plane0.astype(np.float32).astype(np.float64), inner)
    outside = np.zeros(4)
    want = (0.25 * outside + 0.75 * plane0).astype(np.float32)
    got = K.sample_point([t], S.BILINEAR, (S.BORDER, S.BORDER, S.BORDER), L.MIP_NEAREST, u, v, w, None, 0.0)
    assert np.array_equal(got, want)
    taps = K.point_taps(t, S.BILINEAR, (S.BORDER, S.BORDER, S.BORDER), u, v, w)
    assert [k for _, k in taps[:4]] == [None] * 4 and all(k is not None and k[2] == 0 for _, k in taps[4:])
    clamp = K.sample_point([t], S.BILINEAR, (S.BORDER, S.BORDER, S.CLAMP), L.MIP_NEAREST, u, v, w, None, 0.0)
    assert np.array_equal(clamp, (0.25 * plane0 + 0.75 * plane0).astype(np.float32))


def test_model_one_z_tap_is_the_lod_call_for_that_slice():
    """NEAREST anywhere, and BILINEAR where w D - 0.5 is an integer: one z tap of weight 1.0, and 1.0 * p is p."""
    dims = [(12, 10, 8), (6, 5, 4), (3, 2, 2)]
    chain = [volume(10 + l, d) for l, d in enumerate(dims)]
    rng = np.random.default_rng(4)
    coords = rng.uniform(-0.5, 1.5, size=(5, 9, 2)).astype(np.float32)
    lod = K.seeded_lods(rng, (5, 9), 3)
    # BILINEAR (and NEAREST) at the slice centres of a level on its own: the depths 8, 4 and 2 make (kz + 0.5) / D exact
    for l, d in enumerate(dims):
        for slice_z in range(d[2]):
            w = np.float32((slice_z + 0.5) / d[2])
            assert np.float64(w) * d[2] - 0.5 == slice_z
            c3 = np.concatenate([coords, np.full(coords.shape[:2] + (1,), w, dtype=np.float32)], axis=-1)
            for filt in FILTERS:
                for address in ((S.REPEAT, S.MIRROR), (S.BORDER, S.CLAMP)):
                    got = K.sample([chain[l]], filt, address + (S.BORDER,), L.MIP_LINEAR, c3, lod, 0.0)
                    want = L.sample([chain[l][slice_z]], filt, address[0], address[1], L.MIP_LINEAR, coords, lod, 0.0)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (l, slice_z, filt)
    # NEAREST: any w inside the slice, every level of the chain at once when the depths agree
    flat = [volume(20 + l, (d[0], d[1], 4)) for l, d in enumerate(dims)]
    for slice_z, w in ((0, 0.01), (1, 0.3), (3, 0.99)):
        c3 = np.concatenate([coords, np.full(coords.shape[:2] + (1,), w, dtype=np.float32)], axis=-1)
        got = K.sample(flat, S.NEAREST, (S.REPEAT, S.CLAMP, S.CLAMP), L.MIP_LINEAR, c3, lod, 0.25)
        want = L.sample([t[slice_z] for t in flat], S.NEAREST, S.REPEAT, S.CLAMP, L.MIP_LINEAR, coords, lod, 0.25)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_model_texel_centres_reproduce_power_of_two_volumes():
    for dims in ((1, 1, 1), (2, 1, 4), (8, 4, 2), (16, 8, 8)):
        for dtype in (np.float32, np.float16, np.uint8):
            t = volume(sum(dims), dims, dtype)
            centres = K.texel_centres(t)
            for filt in FILTERS:
                for mip in MIPS:
                    got = K.sample([t], filt, (S.BORDER, S.MIRROR, S.REPEAT), mip, centres, None, 0.0)
                    assert np.array_equal(got.reshape(t.shape), t.astype(np.float32)), (dims, dtype, filt)


def test_model_array_form_is_the_pointwise_form():
    dims = K.CHAIN
    chain = [volume(30 + l, d, (np.float32, np.float16, np.uint8)[l % 3]) for l, d in enumerate(dims)]
    chain[0][1, 2, 3, 1] = np.nan
    coords, lod = K.grid_inputs(7, 19, 11, (3, 3, 3))
    for filt in FILTERS:
        for mip in MIPS:
            for address in ((0, 1, 2), (3, 3, 3), (1, 2, 3), (2, 0, 1)):
                a = K.sample(chain, filt, address, mip, coords, lod, 0.25)
                b = K.sample_pointwise(chain, filt, address, mip, coords, lod, 0.25)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (filt, mip, address)


def test_validity():
    big = np.float32(2.0 ** 14)
    nxt = np.nextafter(big, np.float32(np.inf))
    assert K.valid(big, -big, big, np.inf) and K.valid(0.0, -0.0, 1e-45, -np.inf)
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf, nxt, -nxt):
            p = [0.5, 0.5, 0.5]
            p[axis] = bad
            assert not K.valid(*p, 0.0)
    assert not K.valid(0.5, 0.5, 0.5, np.nan)
    # an invalid point is +0.0 in every channel
    t = volume(5, (4, 4, 4))
    assert np.array_equal(K.sample_point([t], 1, (0, 0, 0), 1, 0.5, 0.5, np.nan, 0.0, 0.0).view(np.uint32), np.zeros(4, dtype=np.uint32))


@pytest.mark.parametrize("footprint", K.FOOTPRINTS_2D + K.FOOTPRINTS_3D)
def test_generated_grids_reach_every_case(footprint):
    """The grids of tests/test_decode_volume.py (seed = the grid's index; the modes turn with it there, every mode is asserted on
    every axis here)."""
    most_all = 0
    for k, (ox, oy) in enumerate(K.GRIDS):
        coords, lod = K.grid_inputs(k, ox, oy, footprint)
        for mode in range(4):
            outside, zero_axes, counts, most, blended, single, invalid = K.coverage(K.CHAIN, footprint, S.BILINEAR, (mode,) * 3, L.MIP_LINEAR, coords, lod, 0.0)
            assert outside == {(a, s) for a in range(3) for s in range(2)}, (ox, oy, mode)
            assert zero_axes == {0, 1, 2}
            assert blended and single
            # the 15 invalid triples among the constructed points, and the NaN among the lambdas
            assert invalid >= 16
            if footprint[2] > 1 and ox * oy >= 6:
                assert {1, 8} <= counts, (footprint, ox, oy, counts)
        most_all = max(most_all, K.coverage(K.CHAIN, footprint, S.BILINEAR, (S.REPEAT, S.MIRROR, S.REPEAT), L.MIP_NEAREST, coords, None, 0.0)[3])
    # (level 0 has 24 blocks of 6x6x6 and 48 of 5x5x4 in all: the small footprints are the ones that fill more than a batch)
    if footprint in ((4, 4, 1), (6, 6, 1), (8, 5, 1), (3, 3, 3), (4, 4, 3)):
        assert most_all > DECODE_BATCH, (footprint, most_all)
    # invalid points of every kind are among the constructed ones
    c = K.constructed_points(footprint)
    for axis in range(3):
        col = c[:, axis]
        assert np.isnan(col).any() and np.isposinf(col).any() and np.isneginf(col).any() and (np.abs(col[np.isfinite(col)]) > K.LIMIT).any()
        assert (col == np.float32(K.LIMIT)).any() and (col == -np.float32(K.LIMIT)).any()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """The harness as a program of its own under the sanitizers: no Python and no preload are involved in what it runs."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_volume") / "decode_volume_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("footprint", [(4, 4, 1), (3, 3, 3), (5, 5, 4)])
def test_tap_stage_matches_the_model(harness, tmp_path, footprint):
    W, H, D = K.CHAIN[0]
    rng = np.random.default_rng(9)
    pts = np.concatenate([K.constructed_points(footprint), K.seeded_points(rng, 150)])
    path = tmp_path / "pts.f32"
    pts.tofile(str(path))
    out = subprocess.run([harness, "points"] + [str(v) for v in footprint + (W, H, D)] + [str(path), str(len(pts))], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    heads, taps = {}, {}
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "V":
            heads[int(w[1])] = (int(w[2]), int(w[3]))
        else:
            taps[(int(w[1]), int(w[2]), int(w[3]))] = w[4:]
    assert len(heads) == len(pts)
    texels = np.zeros((D, H, W, 4), dtype=np.uint8)
    checked = 0
    for i, p in enumerate(pts):
        ok = K.valid(p[0], p[1], p[2], 0.0)
        assert heads[i] == (int(ok), 0), (i, p)
        if not ok:
            assert not any(k[0] == i for k in taps)
            continue
        xyz = K.level_coordinates(texels, *p)
        for filt in FILTERS:
            for m in range(4):
                address = (m, (m + 1) % 4, (m + 2) % 4)
                w = taps[(i, filt, m)]
                assert tuple(float.fromhex(v) for v in w[0:3]) == tuple(float(c) for c in xyz), (i, p)
                axes = [L.axis_taps(filt, c) for c in xyz]
                assert [int(v) for v in w[3:6]] == [len(a) for a in axes], (i, p, filt)
                for k, a in enumerate(axes):
                    assert [float.fromhex(v) for v in w[6 + 2 * k:6 + 2 * k + len(a)]] == [float(t[1]) for t in a]
                slots = [tuple(int(v) for v in w[12 + 3 * t:15 + 3 * t]) for t in range(8)]
                want = [(-1, -1, -1)] * 8
                for slot, k in K.point_taps(texels, filt, address, *p):
                    if k is not None:
                        want[slot] = k
                assert slots == want, (i, p, filt, address, slots, want)
                checked += 1
    assert checked == sum(1 for p in pts if K.valid(p[0], p[1], p[2], 0.0)) * 8


def run_tiles(harness, tmp_path, tag, footprint, profile, kind, seed, dims, levels, filt, address, mip, fmt, coords, lod, bias, pads):
    ttype, layout, channels = fmt
    oy, ox = coords.shape[:2]
    cpath, lpath, prefix = tmp_path / (tag + ".coords"), tmp_path / (tag + ".lod"), str(tmp_path / tag)
    np.ascontiguousarray(coords, dtype=np.float32).tofile(str(cpath))
    if lod is not None:
        np.ascontiguousarray(lod, dtype=np.float32).tofile(str(lpath))
    args = [harness, "tiles", *footprint, profile, kind, seed, *dims, levels, filt, *address, mip, ttype, layout, channels, ox, oy, cpath, lpath if lod is not None else "-",
            repr(float(bias)), pads, prefix]
    out = subprocess.run([str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    chain, tiles, shape = [], [], None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "level":
            l, W, H, D, t = (int(v) for v in w[1:6])
            chain.append(np.fromfile(prefix + ".level%d" % l, dtype=(np.uint8, np.float16, np.float32)[t]).reshape(D, H, W, 4))
        elif w[0] == "out":
            shape = tuple(int(v) for v in w[1:])
        elif w[0] == "tile":
            tiles.append(tuple(int(v) for v in w[2:]))
    got = np.fromfile(prefix + ".out", dtype=np.uint8).view(M.BITS_DTYPE[ttype])
    return chain, got, tiles, shape


def check_tiles(harness, tmp_path, tag, footprint, profile, kind, seed, dims, levels, filt, address, mip, fmt, coords, lod, bias, pads):
    chain, got, tiles, (guard, row, plane, elements) = run_tiles(harness, tmp_path, tag, footprint, profile, kind, seed, dims, levels, filt, address, mip, fmt, coords, lod, bias,
                                                                 pads)
    ttype, layout, channels = fmt
    oy, ox = coords.shape[:2]
    assert [c.shape[:3][::-1] for c in chain] == [tuple(max(1, d >> l) for d in dims) for l in range(levels)]
    element = 4 if ttype == M.F32 else 2
    want = np.full(got.size * element, GUARD, dtype=np.uint8).view(M.BITS_DTYPE[ttype])
    bits = M.convert(K.sample(chain, filt, address, mip, coords, lod, bias)[None], ttype, channels, SCALE, BIAS)
    M.scatter(want, guard // element, bits, layout, 0, row, row * oy, plane)
    assert np.array_equal(got, want), (tag, int((got != want).sum()), int(np.argwhere(got != want)[0][0]) - guard // element)
    assert len(tiles) == S.tiles(ox, oy)
    for passes, batches, blocks, mask, most, blended, single in tiles:
        assert passes == bin(mask).count("1") <= levels and most <= 512 and most <= blocks <= most * max(passes, 1) and batches * DECODE_BATCH >= blocks
    return chain, tiles


FORMATS = [(M.F16, M.PLANAR, 3), (M.BF16, M.INTERLEAVED, 4), (M.F32, M.INTERLEAVED, 1), (M.F32, M.PLANAR, 4), (M.F16, M.INTERLEAVED, 3), (M.BF16, M.PLANAR, 1)]


@pytest.mark.parametrize("footprint", [(4, 4, 1), (3, 3, 3), (5, 5, 4)])
def test_whole_tiles_match_the_model(harness, tmp_path, footprint):
    """Chains of five levels (K.CHAIN): the three tile shapes, both filters, both mip filters, the six store builds, the four kinds
    of chain and the profiles and the address modes turning; the grids of tests/test_decode_volume.py; then level 0 alone (lod
    NULL), where a tile's pass lists more than a batch of blocks."""
    turn = sum(footprint)
    most, blended, single = 0, False, False
    for k, (ox, oy) in enumerate(K.GRIDS):
        coords, lod = K.grid_inputs(k, ox, oy, footprint)
        for filt in FILTERS:
            for mip in MIPS:
                n = turn + 4 * k + 2 * filt + mip
                address = (n % 4, (n // 2 + 1) % 4, (n + 3) % 4)
                use = lod if n % 4 else None
                _, tiles = check_tiles(harness, tmp_path, "t%d" % n, footprint, n % 4, n % 4 if n % 3 else 3, n, K.CHAIN[0], 5, filt, address, mip, FORMATS[n % 6], coords, use,
                                       0.25 * (n % 3), n % 8)
                most = max([most] + [t[4] for t in tiles])
                if mip == L.MIP_LINEAR:
                    blended = blended or any(t[5] for t in tiles)
                    single = single or any(t[6] for t in tiles)
    assert blended and single
    # level 0 alone: every point of a tile is in the one pass
    for k, (ox, oy) in enumerate(K.GRIDS):
        coords, _ = K.grid_inputs(k, ox, oy, footprint)
        _, tiles = check_tiles(harness, tmp_path, "m%d" % k, footprint, 0, 3, 40 + k, K.CHAIN[0], 5, S.BILINEAR, (S.REPEAT, S.MIRROR, S.REPEAT), L.MIP_NEAREST, FORMATS[k], coords,
                               None, 0.0, k)
        most = max([most] + [t[4] for t in tiles])
    if footprint != (5, 5, 4):
        assert most > DECODE_BATCH, most


def test_a_nan_behind_a_weight_of_zero(harness, tmp_path):
    """Under the HDR profile with F16 levels, reserved-mode blocks decode to NaN: the texel centres of a power-of-two volume
    (f = 0 on all three axes) read one texel each, so a NaN reaches a point only from its own texel -- the model, which leaves
    zero weights out, has compared every bit -- and integer lambda' leaves the other level unread."""
    rng = np.random.default_rng(3)
    t = np.zeros((8, 8, 16, 4), dtype=np.float16)
    centres = K.texel_centres(t)
    lod = np.where(rng.integers(0, 2, size=centres.shape[:2]) == 1, np.float32(2.0), np.float32(0.0)).astype(np.float32)
    chain, _ = check_tiles(harness, tmp_path, "nan", (4, 4, 3), 3, 1, 11, (16, 8, 8), 3, S.BILINEAR, (S.BORDER, S.REPEAT, S.MIRROR), L.MIP_LINEAR, (M.F32, M.INTERLEAVED, 4), centres, lod,
                           0.0, 3)
    assert np.isnan(chain[0].astype(np.float32)).any() and not np.isnan(chain[0].astype(np.float32)).all()


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    body = ""
    for cname, cls in (("astcenc_amd_volume_grid", A.VolumeGrid), ("astcenc_amd_volume_sampler", A.VolumeSampler)):
        body += '  printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body + '  return 0;\n}\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, cls in zip(lines, (A.VolumeGrid, A.VolumeSampler)):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(cls)
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [f for f, _ in A.VolumeGrid._fields_] == ["first_entry", "level_count", "out_x", "out_y", "coords", "coord_row_pitch", "lod", "lod_row_pitch", "lod_bias", "out",
                                                     "row_pitch", "plane_pitch"]
    assert [f for f, _ in A.VolumeSampler._fields_] == ["filter", "address_x", "address_y", "address_z", "mip_filter"]
    if shutil.which("gcc"):
        c_probe = tmp_path / "probe.c"
        c_probe.write_text('#include "astcenc_amd.h"\nint main(void) { struct astcenc_amd_volume_sampler s; s.address_z = ASTCENC_AMD_ADDRESS_BORDER; return (int)s.address_z - 3; }\n')
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c_probe), "-o", str(tmp_path / "probe_c")], check=True)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_sample_volume_tensors_device
    assert "astcenc_amd_sample_volume_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 8
    assert callable(lib.sample_volume_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    smp = A.VolumeSampler(A.SAMPLE_BILINEAR, 0, 1, 2, A.MIP_LINEAR)
    grid = (A.VolumeGrid * 1)(A.VolumeGrid(0, 1, 2, 2, None, 0, None, 0, 0.0, None, 0, 0))
    # no grids: nothing to do, whatever else is passed (a null sampler included)
    assert fn(None, None, 0, None, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 0, None) == A.SUCCESS
    # a null context; a count without grids; a count without entries
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), C.byref(smp), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), C.byref(smp), grid, 1, None) == A.ERR_BAD_PARAM


def test_volume_grid_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    coords = torch.zeros((8, 40, 50, 3), dtype=torch.float32)
    lod = torch.zeros((8, 40, 50), dtype=torch.float32)
    g = A.volume_grid(2, 7, coords[3], lod[3], batch[3], lod_bias=-0.5)
    assert (g.first_entry, g.level_count, g.out_x, g.out_y, g.lod_bias) == (2, 7, 50, 40, -0.5)
    assert (g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (coords[3].data_ptr(), 150, lod[3].data_ptr(), 50, batch[3].data_ptr(), 50,
                                                                                                        2000)
    # a tile of all three: the triples need no alignment beyond the float's
    cv, lv, ov = coords[1, 4:14, 7:27], lod[1, 4:14, 7:27], batch[1, :, 4:14, 7:27]
    g = A.volume_grid(0, 1, cv, lv, ov)
    assert cv.data_ptr() % 8 == 4
    assert (g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.out, g.row_pitch, g.plane_pitch) == (20, 10, cv.data_ptr(), 150, lv.data_ptr(), 50,
                                                                                                                          ov.data_ptr(), 50, 2000)
    g = A.volume_grid(0, 3, cv, None, ov, lod_bias=1.0)
    assert (g.lod, g.lod_row_pitch, g.lod_bias) == (None, 0, 1.0)
    # one row of points: a list of ray-march samples
    g = A.volume_grid(0, 32, torch.zeros((1, 1000, 3)), torch.zeros((1, 1000)), torch.zeros((3, 1, 1000)), type=A.TENSOR_F32)
    assert (g.out_x, g.out_y, g.coord_row_pitch, g.lod_row_pitch, g.row_pitch) == (1000, 1, 0, 0, 0)
    # an interleaved view
    g = A.volume_grid(0, 2, coords[0], None, torch.zeros((40, 50, 4), dtype=torch.bfloat16), layout=A.TENSOR_INTERLEAVED, type=A.TENSOR_BF16)
    assert (g.out_x, g.out_y, g.row_pitch, g.plane_pitch) == (50, 40, 200, 0)
    # explicit pointers and pitches
    g = A.volume_grid(1, 4, (4100, 6, 7, 64), (12288, 8), (8192, 16, 9000), lod_bias=2.0)
    assert (g.first_entry, g.level_count, g.out_x, g.out_y, g.coords, g.coord_row_pitch, g.lod, g.lod_row_pitch, g.lod_bias, g.out, g.row_pitch, g.plane_pitch) == \
        (1, 4, 6, 7, 4100, 64, 12288, 8, 2.0, 8192, 16, 9000)
    # what the call cannot express
    out = torch.zeros((3, 40, 50), dtype=torch.float16)
    c = torch.zeros((40, 50, 3), dtype=torch.float32)
    for bad in (dict(coords=c.double()), dict(coords=torch.zeros((40, 50, 2))), dict(coords=torch.zeros((40, 50, 4))[:, :, :3]), dict(coords=c[:, :49]),
                dict(coords=c[:1].expand(40, 50, 3)), dict(coords=torch.zeros((40, 3, 50)).permute(0, 2, 1)), dict(lod=torch.zeros((40, 49))), dict(lod=torch.zeros((40, 50)).double()),
                dict(level_count=0), dict(level_count=33), dict(lod_bias=float("nan")), dict(out=out[0]), dict(out=out.float()[:, :, :49])):
        kw = dict(level_count=3, coords=c, lod=None, out=out, lod_bias=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            A.volume_grid(0, kw["level_count"], kw["coords"], kw["lod"], kw["out"], lod_bias=kw["lod_bias"], type=A.TENSOR_F16)


def test_volume_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    vol = {n: d for n, d in by_short.items() if n.startswith("astc_volume_sample")}
    # one build per tensor type and layout
    assert len(vol) == 6, sorted(by_short)
    for name, d in vol.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        assert d["group_segment_fixed_size"] == 7168, (name, d)
    # ... and the other samplers' kernels are still their six each
    for other in ("astc_lod_sample", "astc_cube_sample"):
        assert len([n for n in by_short if n.startswith(other)]) == 6
