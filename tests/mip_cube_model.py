# SPDX-License-Identifier: Apache-2.0
"""numpy model of ASTCENC_AMD_MIP_EDGE_CUBE (include/astcenc_amd.h, "Cube edges"), bit for bit.

  * source(): the texel a tap reads, worked out from the face frames of the GL cube-map table with integer vectors, exactly as
    the header states the rule (csrc/mip_resample.h carries a table of bytes derived from it);
  * downsample() / chain(): every face is unfolded into a padded square -- its own texels in the middle, the mapped texels of
    the neighbours (and its corner texels) in a border of PAD texels -- and filtered there with the taps, values and sums of
    tests/mip_filter_model.py, tap i of the face at padded index i + PAD.  The alpha-weighted form filters the weighted values
    of tests/mip_weighted_model.py over the same padded squares.

Shared by tests/test_mip_cube_cpu.py (against the header compiled with g++) and tests/test_mip_cube.py (against the GPU)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402
import mip_filter_model as F  # noqa: E402
import mip_weighted_model as W  # noqa: E402

CUBE = 2
ARRAY = F.ARRAY
NONE, ALPHA = W.NONE, W.ALPHA
PAD = 10                                    # taps reach at most 9 texels out of a face (s = 3: 7)
FACES = ("+X", "-X", "+Y", "-Y", "+Z", "-Z")
# the GL cube-map table: major axis, the direction x grows along, the direction y grows along
MAJOR = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))
SDIR = ((0, 0, -1), (0, 0, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (-1, 0, 0))
TDIR = ((0, -1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (0, -1, 0))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def centre(f, x, y, s):
    """The centre of texel (x, y) of face f in doubled integer units: P = s M + U S + V T."""
    u, v = 2 * x + 1 - s, 2 * y + 1 - s
    return tuple(s * MAJOR[f][i] + u * SDIR[f][i] + v * TDIR[f][i] for i in range(3))


def source(f, ix, iy, s):
    """(face, x, y) of the texel that tap (ix, iy) of face f reads."""
    in_x, in_y = 0 <= ix < s, 0 <= iy < s
    if in_x and in_y:
        return f, ix, iy
    if not in_x and not in_y:
        return f, min(max(ix, 0), s - 1), min(max(iy, 0), s - 1)
    if not in_x:
        a, i, w = SDIR[f], ix, tuple((2 * iy + 1 - s) * c for c in TDIR[f])
    else:
        a, i, w = TDIR[f], iy, tuple((2 * ix + 1 - s) * c for c in SDIR[f])
    sg = 1 if i >= s else -1
    kk = min(i - s if i >= s else -1 - i, s - 1)
    p = tuple(sg * s * a[c] + (s - (2 * kk + 1)) * MAJOR[f][c] + w[c] for c in range(3))
    f2 = MAJOR.index(tuple(sg * c for c in a))
    u, v = _dot(p, SDIR[f2]) + s - 1, _dot(p, TDIR[f2]) + s - 1
    assert u % 2 == 0 and v % 2 == 0
    return f2, u // 2, v // 2


@functools.lru_cache(maxsize=64)
def unfold(s):
    """(face, y, x) index arrays [6, s + 2 PAD, s + 2 PAD]: padded texel (iy + PAD, ix + PAD) of face f is source(f, ix, iy, s)."""
    n = s + 2 * PAD
    face = np.empty((6, n, n), np.int64)
    ys = np.empty((6, n, n), np.int64)
    xs = np.empty((6, n, n), np.int64)
    inner = np.arange(s)
    for f in range(6):
        face[f] = f
        ys[f, PAD:PAD + s, PAD:PAD + s] = inner[:, None]
        xs[f, PAD:PAD + s, PAD:PAD + s] = inner[None, :]
        for iy in range(-PAD, s + PAD):
            cols = list(range(-PAD, 0)) + list(range(s, s + PAD)) if 0 <= iy < s else range(-PAD, s + PAD)
            for ix in cols:
                face[f, iy + PAD, ix + PAD], xs[f, iy + PAD, ix + PAD], ys[f, iy + PAD, ix + PAD] = source(f, ix, iy, s)
    return face, ys, xs


def padded(level):
    """level [6 n, s, s, C] -> the unfolded faces [6 n, s + 2 PAD, s + 2 PAD, C]."""
    z, s = level.shape[0], level.shape[1]
    assert z % 6 == 0 and level.shape[2] == s
    face, ys, xs = unfold(s)
    cubes = level.reshape(z // 6, 6, s, s, level.shape[3])
    return cubes[:, face, ys, xs].reshape(z, s + 2 * PAD, s + 2 * PAD, level.shape[3])


@functools.lru_cache(maxsize=256)
def _axis(kind, s):
    """mip_filter_model.axis on the padded square: (idx [K, d] padded texels, w [K, d], valid [K, d])."""
    d = max(1, s >> 1)
    rows = [F.taps(kind, s, j) for j in range(d)]
    k = max(len(w) for _, w in rows)
    idx = np.zeros((k, d), np.int64)
    w = np.zeros((k, d), np.float64)
    valid = np.zeros((k, d), bool)
    for j, (first, ws) in enumerate(rows):
        assert first >= -PAD and first + len(ws) <= s + PAD
        for t, wt in enumerate(ws):
            idx[t, j] = first + t + PAD
            w[t, j] = wt
            valid[t, j] = True
    return idx, w, valid


def _sums(vals, kind, s):
    """vals [Z, s + 2 PAD, s + 2 PAD, C] float64 (padded) -> the row and acc sums of every destination texel, vol = 1.0 * acc."""
    i, w, v = _axis(kind, s)
    rows = F._sum((w[k][None, None, :, None] * vals[:, :, i[k]], v[k][None, None, :, None]) for k in range(len(i)))
    acc = F._sum((w[k][None, :, None, None] * rows[:, i[k]], v[k][None, :, None, None]) for k in range(len(i)))
    return 1.0 * acc


def _plain(level, kind, srgb):
    s = level.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        vol = _sums(F._values(padded(level), srgb), kind, s)
        if level.dtype == np.uint8:                        # (the results of mip_filter_model.downsample)
            out = np.clip(np.floor(vol + 0.5), 0, 255).astype(np.uint8)
            if srgb:
                out[..., :3] = np.searchsorted(M.SRGB_THR, vol[..., :3], side="right").astype(np.uint8)
            return out
        out = vol.astype(np.float32)
        return out.astype(np.float16) if level.dtype == np.float16 else out


def _weighted(level, kind, srgb):
    s = level.shape[1]
    plain = _plain(level, kind, srgb)
    out = plain.copy()
    pad = padded(level)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if level.dtype == np.uint8:                        # (the values and results of mip_weighted_model._windowed)
            a = pad[..., 3:4]
            if srgb:
                vals = a.astype(np.float64) * M.SRGB_LIN[pad[..., :3]]
            else:
                vals = (a.astype(np.uint32) * pad[..., :3].astype(np.uint32)).astype(np.float64)
            vals = np.concatenate([vals, a.astype(np.float64)], axis=-1)
        else:
            f = pad.astype(np.float64)
            vals = np.concatenate([f[..., 3:4] * f[..., :3], f[..., 3:4]], axis=-1)
        vol = _sums(vals, kind, s)
        vol_a = vol[..., 3:4]
        m = vol[..., :3] / vol_a
        if level.dtype == np.uint8:
            if srgb:
                w = np.searchsorted(M.SRGB_THR, m, side="right").astype(np.uint8)
            else:
                w = np.clip(np.floor(m + 0.5), 0, 255)
                w = np.where(np.isnan(w), 0, w).astype(np.uint8)
        else:
            w = W._to_type(m, level.dtype)
        out[..., :3] = np.where(vol_a > 0.0, w, plain[..., :3])
        return out


def downsample(level, kind, weight=NONE, srgb=False):
    """One level of cubes: level [6 n, s, s, 4] (layer l = face l % 6 of cube l / 6) -> the next, same dtype."""
    assert kind in F.KINDS and level.shape[0] % 6 == 0 and level.shape[1] == level.shape[2]
    if level.shape[1] == 1:                                # (one tap on texel 0: never leaves the face)
        return W.downsample(level, ARRAY, kind, F.CLAMP, weight, srgb)
    return _plain(level, kind, srgb) if weight == NONE else _weighted(level, kind, srgb)


def chain(level0, kind, weight=NONE, levels=0, srgb=False):
    """[level 0, level 1, ...] of a [6 n, s, s, 4] array of cubes with edge CUBE; BOX: the box filter's models."""
    if kind == F.BOX:
        return W.chain(level0, ARRAY, F.BOX, F.CLAMP, weight, levels, srgb)
    z, h, w = level0.shape[:3]
    out = [level0]
    for _ in range(1, len(V.level_dims(w, h, z, ARRAY, levels))):
        out.append(downsample(out[-1], kind, weight, srgb))
    return out
