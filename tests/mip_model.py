# SPDX-License-Identifier: Apache-2.0
"""numpy model of the mip chain filter of include/astcenc_amd.h (csrc/mip_filter.h), bit for bit.

Shared by tests/test_mip_chain_cpu.py (against the header compiled with g++) and tests/test_mip_chain.py (against the GPU).
Every operation is a separate IEEE operation on whole arrays, in the order the header performs them, so nothing depends on
how numpy vectorises.  The sRGB tables use math.pow -- the C library's pow, which the library's host code calls too --
rather than np.power, whose SIMD loops may differ from it in the last bit."""
import math

import numpy as np


def full_levels(w, h):
    return max(w, h).bit_length()


def level_dims(w, h, levels=0):
    n = full_levels(w, h) if levels == 0 else levels
    return [(max(1, w >> i), max(1, h >> i)) for i in range(n)]


def axis_taps(s):
    """(index arrays, weight arrays, denominator) of every destination texel along an axis of s source texels: lists of
    length 1, 2 or 3 of int arrays of size max(1, s >> 1)."""
    d = max(1, s >> 1)
    j = np.arange(d, dtype=np.int64)
    if s == 1:
        return [j * 0], [np.ones(d, np.int64)], 1
    if s % 2 == 0:
        return [2 * j, 2 * j + 1], [np.ones(d, np.int64), np.ones(d, np.int64)], 2
    n = s >> 1
    return [2 * j, 2 * j + 1, 2 * j + 2], [n - j, np.full(d, n, np.int64), j + 1], s


def _eotf(x):
    return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)


SRGB_LIN = np.array([_eotf(c / 255.0) for c in range(256)], dtype=np.float64)
SRGB_THR = np.array([_eotf((c - 0.5) / 255.0) for c in range(1, 256)], dtype=np.float64)


def _weighted_mean_f64(vals, ix, wx, dx, iy, wy, dy):
    """vals: [H, W, C] float64.  The header's order: rows over x taps, then the y taps, then / (den_x * den_y)."""
    acc = None
    for yi, yw in zip(iy, wy):
        rows = vals[yi]                                             # [Dy, W, C]
        row = None
        for xi, xw in zip(ix, wx):
            p = xw.astype(np.float64)[None, :, None] * rows[:, xi]
            row = p if row is None else row + p
        q = yw.astype(np.float64)[:, None, None] * row
        acc = q if acc is None else acc + q
    return acc / (np.float64(dx) * np.float64(dy))


def downsample(img, srgb=False):
    """One level: img [H, W, 4] of uint8 / float16 / float32 -> the next level, same dtype."""
    h, w = img.shape[0], img.shape[1]
    ix, wx, dx = axis_taps(w)
    iy, wy, dy = axis_taps(h)
    if img.dtype == np.uint8:
        v = img.astype(np.uint64)
        s = None
        for yi, yw in zip(iy, wy):
            for xi, xw in zip(ix, wx):
                t = (yw.astype(np.uint64)[:, None, None] * xw.astype(np.uint64)[None, :, None]) * v[yi][:, xi]
                s = t if s is None else s + t
        den = np.uint64(dx) * np.uint64(dy)
        out = ((np.uint64(2) * s + den) // (np.uint64(2) * den)).astype(np.uint8)
        if srgb:
            mean = _weighted_mean_f64(SRGB_LIN[img[..., :3]], ix, wx, dx, iy, wy, dy)
            out[..., :3] = np.searchsorted(SRGB_THR, mean, side="right").astype(np.uint8)
        return out
    mean = _weighted_mean_f64(img.astype(np.float64), ix, wx, dx, iy, wy, dy)
    with np.errstate(over="ignore"):
        out = mean.astype(np.float32)
        return out.astype(np.float16) if img.dtype == np.float16 else out


def chain(img, levels=0, srgb=False):
    """[level 0 = img, level 1, ...]: the full chain (levels == 0) or the first `levels` levels."""
    n = full_levels(img.shape[1], img.shape[0]) if levels == 0 else levels
    out = [img]
    for _ in range(1, n):
        out.append(downsample(out[-1], srgb))
    return out
