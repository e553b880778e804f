# SPDX-License-Identifier: Apache-2.0
"""numpy model of the windowed mip filters of include/astcenc_amd.h (csrc/mip_resample.h), bit for bit.

  * the taps and weights of every destination texel in Python floats: math.sin is the C library's sin, which the library's host
    code calls too (np.sin's SIMD loops may differ from it in the last bit), math.sqrt is correctly rounded;
  * then the separable float64 arithmetic: row sums over each texel's actual x taps for every source row, the y sums over the
    row sums, the z sums over the slices (an ARRAY layer and a 2D image: the one z tap of weight 1.0), every sum starting at its
    first product and masked where a texel has fewer taps (no zero-weight padding).

Shared by tests/test_mip_filter_cpu.py (against the header compiled with g++) and tests/test_mip_filter.py (against the GPU)."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402

BOX, MITCHELL, LANCZOS3, KAISER = 0, 1, 2, 3
CLAMP, WRAP = 0, 1
ARRAY, VOLUME = V.ARRAY, V.VOLUME
KINDS = (MITCHELL, LANCZOS3, KAISER)
PI = 3.141592653589793


def support(kind):
    return 2 if kind == MITCHELL else 3


def i0(x):
    q = x * 0.5
    q2 = q * q
    term, s = 1.0, 1.0
    for k in range(1, 25):
        term = term * q2 / float(k * k)
        s = s + term
    return s


def sinc(x):
    if x == 0.0:
        return 1.0
    px = PI * x
    return math.sin(px) / px


def evaluate(kind, a):
    if kind == MITCHELL:
        a2 = a * a
        a3 = a2 * a
        if a < 1.0:
            return ((7.0 * a3 - 12.0 * a2) + 16.0 / 3.0) / 6.0
        return ((((-7.0 / 3.0) * a3 + 12.0 * a2) - 20.0 * a) + 32.0 / 3.0) / 6.0
    if kind == LANCZOS3:
        return sinc(a) * sinc(a / 3.0)
    q = a / 3.0
    return (sinc(a) * i0(4.0 * math.sqrt(1.0 - q * q))) / i0(4.0)


def taps(kind, s, j):
    """(first tap index, [weights]) of destination texel j along an axis of s source texels."""
    if s <= 1:
        return 0, [1.0]
    d = s >> 1
    r = float(s) / float(d)
    c = float((2 * j + 1) * s) / float(2 * d)
    S = float(support(kind))
    first, f = None, []
    for i in range(int(c - S * r) - 3, int(c + S * r) + 4):
        t = ((float(i) + 0.5) - c) / r
        a = -t if t < 0.0 else t
        if not a < S:
            continue
        if first is None:
            first = i
        f.append(evaluate(kind, a))
    total = f[0]
    for v in f[1:]:
        total = total + v
    return first, [v / total for v in f]


def source(i, s, edge):
    if 0 <= i < s:
        return i
    if edge == WRAP:
        return i % s                        # (Python's % is non-negative for s > 0)
    return 0 if i < 0 else s - 1


@functools.lru_cache(maxsize=256)
def axis(kind, edge, s):
    """(idx [K, d] source texels, w [K, d] float64, valid [K, d]) of every destination texel, K the largest tap count."""
    d = max(1, s >> 1)
    rows = [taps(kind, s, j) for j in range(d)]
    k = max(len(w) for _, w in rows)
    idx = np.zeros((k, d), np.int64)
    w = np.zeros((k, d), np.float64)
    valid = np.zeros((k, d), bool)
    for j, (first, ws) in enumerate(rows):
        for t, wt in enumerate(ws):
            idx[t, j] = source(first + t, s, edge)
            w[t, j] = wt
            valid[t, j] = True
    return idx, w, valid


def _sum(terms):
    """sum_k terms(k) over an axis's taps: starts at the first product, masked where a texel has fewer taps."""
    out = None
    for prod, ok in terms:
        out = prod if out is None else np.where(ok, out + prod, out)
    return out


def _values(level, srgb):
    if level.dtype == np.uint8:
        v = level.astype(np.float64)
        if srgb:
            v[..., :3] = M.SRGB_LIN[level[..., :3]]
        return v
    return level.astype(np.float64)


def downsample(level, kind, edge, mip_kind=VOLUME, srgb=False):
    """One level: level [Z, H, W, 4] (Z: depth of a VOLUME, layers of an ARRAY) -> the next, same dtype."""
    z, h, w = level.shape[:3]
    ix, wx, vx = axis(kind, edge, w)
    iy, wy, vy = axis(kind, edge, h)
    with np.errstate(invalid="ignore", over="ignore"):
        # x pass over every source row (in chunks of rows, to bound the float64 copy)
        rows = np.empty((z, h, ix.shape[1], 4), np.float64)
        step = max(1, (1 << 22) // max(1, w))
        for y0 in range(0, h, step):
            v = _values(level[:, y0:y0 + step], srgb)
            rows[:, y0:y0 + step] = _sum((wx[k][None, None, :, None] * v[:, :, ix[k]], vx[k][None, None, :, None]) for k in range(len(ix)))
        acc = _sum((wy[k][None, :, None, None] * rows[:, iy[k]], vy[k][None, :, None, None]) for k in range(len(iy)))
        if mip_kind == VOLUME:
            iz, wz, vz = axis(kind, edge, z)
            vol = _sum((wz[k][:, None, None, None] * acc[iz[k]], vz[k][:, None, None, None]) for k in range(len(iz)))
        else:
            vol = 1.0 * acc
        if level.dtype == np.uint8:
            out = np.clip(np.floor(vol + 0.5), 0, 255).astype(np.uint8)
            if srgb:
                out[..., :3] = np.searchsorted(M.SRGB_THR, vol[..., :3], side="right").astype(np.uint8)
            return out
        out = vol.astype(np.float32)
        return out.astype(np.float16) if level.dtype == np.float16 else out


def chain(level0, mip_kind, kind, edge, levels=0, srgb=False):
    """[level 0, level 1, ...] of a [Z, H, W, 4] ARRAY or VOLUME; BOX: the box filter's models."""
    if kind == BOX:
        return V.chain_array(level0, levels, srgb) if mip_kind == ARRAY else V.chain_volume(level0, levels, srgb)
    z, h, w = level0.shape[:3]
    dims = V.level_dims(w, h, z, mip_kind, levels)
    out = [level0]
    for _ in range(1, len(dims)):
        out.append(downsample(out[-1], kind, edge, mip_kind, srgb))
    return out
