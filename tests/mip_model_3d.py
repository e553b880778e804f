# SPDX-License-Identifier: Apache-2.0
"""numpy model of the mip chains of arrays and volumes (include/astcenc_amd.h, csrc/mip_filter.h), bit for bit.

  * an ARRAY (texture array layers, cube faces) filters every layer with the 2D filter of tests/mip_model.py;
  * a VOLUME adds a z axis with the same taps: for each z tap in increasing slice the 2D sum of that slice (before the 2D
    division), then the float64 sum over the z taps starting at its first product, then / ((den_x * den_y) * den_z); linear
    RGBA8 is the exact rational mean over all three axes, rounded to nearest, ties up.

Shared by tests/test_mip_chain_volume_cpu.py (against the header compiled with g++) and tests/test_mip_chain_volume.py
(against the GPU).  Every operation is a separate IEEE operation on whole arrays, in the order the header performs them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402

ARRAY, VOLUME = 0, 1


def full_levels(w, h, d, kind=VOLUME):
    return max(w, h, d).bit_length() if kind == VOLUME else M.full_levels(w, h)


def level_dims(w, h, d, kind=VOLUME, levels=0):
    n = full_levels(w, h, d, kind) if levels == 0 else levels
    return [(max(1, w >> i), max(1, h >> i), max(1, d >> i) if kind == VOLUME else d) for i in range(n)]


def _acc_2d(vals, ix, wx, iy, wy):
    """vals [Z, H, W, C] float64 -> the 2D acc of every slice (the header's order, no division): [Z, Dy, Dx, C]."""
    acc = None
    for yi, yw in zip(iy, wy):
        rows = vals[:, yi]                                          # [Z, Dy, W, C]
        row = None
        for xi, xw in zip(ix, wx):
            p = xw.astype(np.float64)[None, None, :, None] * rows[:, :, xi]
            row = p if row is None else row + p
        q = yw.astype(np.float64)[None, :, None, None] * row
        acc = q if acc is None else acc + q
    return acc


def _mean_3d_f64(vals, taps):
    (ix, wx, dx), (iy, wy, dy), (iz, wz, dz) = taps
    vol = None
    for zi, zw in zip(iz, wz):
        r = zw.astype(np.float64)[:, None, None, None] * _acc_2d(vals[zi], ix, wx, iy, wy)
        vol = r if vol is None else vol + r
    return vol / ((np.float64(dx) * np.float64(dy)) * np.float64(dz))


def downsample_volume(vol, srgb=False):
    """One level of a volume: vol [D, H, W, 4] of uint8 / float16 / float32 -> the next level, same dtype."""
    d, h, w = vol.shape[0], vol.shape[1], vol.shape[2]
    taps = (M.axis_taps(w), M.axis_taps(h), M.axis_taps(d))
    (ix, wx, dx), (iy, wy, dy), (iz, wz, dz) = taps
    if vol.dtype == np.uint8:
        v = vol.astype(np.uint64)
        s = None
        for zi, zw in zip(iz, wz):
            for yi, yw in zip(iy, wy):
                for xi, xw in zip(ix, wx):
                    wt = (xw.astype(np.uint64)[None, None, :] * yw.astype(np.uint64)[None, :, None]) * zw.astype(np.uint64)[:, None, None]
                    t = wt[..., None] * v[zi][:, yi][:, :, xi]
                    s = t if s is None else s + t
        den = np.uint64(dx) * np.uint64(dy) * np.uint64(dz)
        out = ((np.uint64(2) * s + den) // (np.uint64(2) * den)).astype(np.uint8)
        if srgb:
            mean = _mean_3d_f64(M.SRGB_LIN[vol[..., :3]], taps)
            out[..., :3] = np.searchsorted(M.SRGB_THR, mean, side="right").astype(np.uint8)
        return out
    mean = _mean_3d_f64(vol.astype(np.float64), taps)
    with np.errstate(over="ignore"):
        out = mean.astype(np.float32)
        return out.astype(np.float16) if vol.dtype == np.float16 else out


def chain_volume(vol, levels=0, srgb=False):
    """[level 0 = vol, level 1, ...] of a [D, H, W, 4] volume: every axis halves."""
    n = full_levels(vol.shape[2], vol.shape[1], vol.shape[0]) if levels == 0 else levels
    out = [vol]
    for _ in range(1, n):
        out.append(downsample_volume(out[-1], srgb))
    return out


def chain_array(layers, levels=0, srgb=False):
    """[level 0 = layers, level 1, ...] of a [L, H, W, 4] array: every layer through the 2D chain, the layer count kept."""
    per = [M.chain(layers[i], levels, srgb) for i in range(layers.shape[0])]
    return [np.stack([p[k] for p in per]) for k in range(len(per[0]))]
