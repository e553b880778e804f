# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_tensors_device, written from the comment in include/astcenc_amd.h alone: per point the taps
of each axis from the binary32 coordinate widened to binary64 (Python integers for the indices), the address mode applied to each
tap index, the image's texels (what the regions call writes) widened to binary64, the x taps' products summed in tap order per
source row, then the y taps' products of those sums, one float64 operation at a time (numpy's float64 multiply and add are IEEE
operations and are never fused), one rounding to float32; then scale, bias, storage and placement of the tensors call
(tests/tensor_model.py).  Nothing here knows how the library does it."""
import math

import numpy as np

import tensor_model as M

NEAREST, BILINEAR = 0, 1
CLAMP, REPEAT, MIRROR, BORDER = 0, 1, 2, 3
LIMIT = 2.0 ** 30


def valid(x, y):
    """Both coordinates finite and no larger than 2^30 in magnitude."""
    return all(math.isfinite(float(v)) and abs(float(v)) <= LIMIT for v in (x, y))


def axis_taps(filter, u):
    """[(index, weight)] in tap order, zero weights left out, of the binary32 coordinate u along one axis."""
    u = np.float64(np.float32(u))
    if filter == NEAREST:
        return [(int(math.floor(u)), np.float64(1.0))]
    t = u - np.float64(0.5)
    i0 = int(math.floor(t))
    f = t - np.float64(i0)
    taps = [(i0, np.float64(1.0) - f), (i0 + 1, f)]
    return [(i, w) for i, w in taps if w != 0.0]


def address(mode, i, S):
    """The texel index of tap index i along an axis of S texels, or None: a BORDER tap outside the image."""
    if mode == CLAMP:
        return min(max(i, 0), S - 1)
    if mode == REPEAT:
        return i % S                            # Python's % is the non-negative remainder
    if mode == MIRROR:
        m = i % (2 * S)
        return m if m < S else 2 * S - 1 - m
    return i if 0 <= i <= S - 1 else None


def sample_point(texels, filter, address_x, address_y, x, y):
    """s[0 .. 3] (float32) of one point of the image texels [H, W, 4] (uint8 / float16 / float32)."""
    if not valid(x, y):
        return np.zeros(4, dtype=np.float32)
    H, W = texels.shape[:2]
    zero = np.zeros(4, dtype=np.float64)
    with np.errstate(all="ignore"):
        acc = None
        for iy, wy in axis_taps(filter, y):
            ky = address(address_y, iy, H)
            r = None
            for ix, wx in axis_taps(filter, x):
                kx = address(address_x, ix, W)
                v = zero if kx is None or ky is None else texels[ky, kx].astype(np.float64)      # exact for all three types
                p = wx * v
                r = p if r is None else r + p
            p = wy * r
            acc = p if acc is None else acc + p
        return acc.astype(np.float32)


def sample_pointwise(texels, filter, address_x, address_y, coords):
    """coords [out_y, out_x, 2] float32 (x then y) -> s [out_y, out_x, 4] float32, point by point."""
    coords = np.asarray(coords, dtype=np.float32)
    out = np.empty(coords.shape[:2] + (4,), dtype=np.float32)
    for j in range(coords.shape[0]):
        for i in range(coords.shape[1]):
            out[j, i] = sample_point(texels, filter, address_x, address_y, coords[j, i, 0], coords[j, i, 1])
    return out


def _axis_arrays(filter, mode, u, S):
    """Per point: the texel indices of taps 0 and 1 (int64, -1: a BORDER tap outside), their weights, and whether tap 1 exists."""
    if filter == NEAREST:
        i0 = np.floor(u).astype(np.int64)
        w = [np.ones_like(u), np.zeros_like(u)]
    else:
        t = u - np.float64(0.5)
        fl = np.floor(t)
        f = t - fl
        i0 = fl.astype(np.int64)
        w = [np.float64(1.0) - f, f]
    idx = []
    for i in (i0, i0 + 1):
        if mode == CLAMP:
            k = np.clip(i, 0, S - 1)
        elif mode == REPEAT:
            k = i % S
        elif mode == MIRROR:
            m = i % (2 * S)
            k = np.where(m < S, m, 2 * S - 1 - m)
        else:
            k = np.where((i >= 0) & (i <= S - 1), i, -1)
        idx.append(k)
    return idx, w, w[1] != 0.0


def sample(texels, filter, address_x, address_y, coords):
    """coords [out_y, out_x, 2] float32 (x then y) -> s [out_y, out_x, 4] float32: sample_point for every point, as array
    operations (the same float64 operations in the same order; tests/test_decode_sample_cpu.py holds the two together)."""
    coords = np.asarray(coords, dtype=np.float32)
    texels = np.asarray(texels)
    H, W = texels.shape[:2]
    x, y = coords[..., 0].astype(np.float64), coords[..., 1].astype(np.float64)
    ok = np.isfinite(x) & np.isfinite(y) & (np.abs(x) <= LIMIT) & (np.abs(y) <= LIMIT)
    x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    kx, wx, two_x = _axis_arrays(filter, address_x, x, W)
    ky, wy, two_y = _axis_arrays(filter, address_y, y, H)
    v64 = texels.astype(np.float64)                                # exact for all three types

    def value(a, b):
        inside = (kx[a] >= 0) & (ky[b] >= 0)
        v = v64[np.where(inside, ky[b], 0), np.where(inside, kx[a], 0)]
        return np.where(inside[..., None], v, 0.0)

    def row(b):
        r = wx[0][..., None] * value(0, b)
        return np.where(two_x[..., None], r + wx[1][..., None] * value(1, b), r)

    with np.errstate(all="ignore"):
        acc = wy[0][..., None] * row(0)
        acc = np.where(two_y[..., None], acc + wy[1][..., None] * row(1), acc)
        return np.where(ok[..., None], acc, 0.0).astype(np.float32)


def convert(texels, filter, address_x, address_y, coords, ttype, channels, scale, bias):
    """-> bits [1, out_y, out_x, channels] (the D, H, W, C of tensor_model.scatter)."""
    return M.convert(sample(texels, filter, address_x, address_y, coords)[None], ttype, channels, scale, bias)


def tensor(texels, filter, address_x, address_y, coords, ttype, layout, channels, scale, bias):
    """The tight tensor of one grid: bits [C, H, W] (planar) or [H, W, C] (interleaved)."""
    t = M.tensor(sample(texels, filter, address_x, address_y, coords)[None], ttype, layout, channels, scale, bias)
    return t[:, 0] if layout == M.PLANAR else t[0]


def tile_shape(out_y):
    """(tw, th) of a grid's tiles: th = min(8, out_y rounded up to a power of two), tw * th = 64."""
    th = 1
    while th < min(out_y, 8):
        th *= 2
    return 64 // th, th


def tiles(out_x, out_y):
    tw, th = tile_shape(out_y)
    return -(-out_x // tw) * -(-out_y // th)


def special_coordinates(size):
    """The coordinates the hand checks name, along an axis of `size` texels: texel centres at both edges, the edges themselves,
    -0.0, tiny values (1e-30 vanishes against 1/2, 2^-53 does not), a negative one, and the invalid ones with their neighbours."""
    big = np.float32(2.0 ** 30)
    nxt = np.nextafter(big, np.float32(np.inf))
    return np.array([0.5, 0.0, -0.0, size - 0.5, size, 1e-30, -3.25, 2.0 ** -53, np.nan, np.inf, -np.inf, big, nxt, -big, -nxt], dtype=np.float32)
