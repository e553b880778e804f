# SPDX-License-Identifier: Apache-2.0
"""numpy model of alpha-weighted mip filtering (include/astcenc_amd.h, csrc/mip_weighted.h), bit for bit.

Built on the plain models (mip_model.py, mip_model_3d.py, mip_filter_model.py): their taps, sums, sRGB tables and half
conversions.  Channel 3 of every level, and channels 0-2 wherever the footprint has no positive alpha weight, are the plain
model's; elsewhere channels 0-2 are the alpha-weighted mean, computed in the header's order:

  * box, linear U8: SA = sum W a, SP_c = sum W a c in integers, (2 SP_c + SA) // (2 SA);
  * box, sRGB U8 and floats: the plain row / acc / vol sums over (double)a * lin[c] or (double)a * (double)c, divided by SA
    (sRGB) or by volA, the plain sums over (double)a (floats);
  * windowed filters: the plain separable sums over those values (linear U8: (double)(a * c)), m = volP_c / volA where
    volA > 0.0.

Shared by tests/test_mip_weighted_cpu.py (against the header compiled with g++) and tests/test_mip_weighted.py (the GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402
import mip_filter_model as F  # noqa: E402

NONE, ALPHA = 0, 1
ARRAY, VOLUME = V.ARRAY, V.VOLUME
BOX, MITCHELL, LANCZOS3, KAISER = F.BOX, F.MITCHELL, F.LANCZOS3, F.KAISER
CLAMP, WRAP = F.CLAMP, F.WRAP


def _box_taps(level, mip_kind):
    z, h, w = level.shape[:3]
    if mip_kind == VOLUME:
        tz = M.axis_taps(z)
    else:                                   # a layer reads its own slice: the taps of depth 1
        tz = ([np.arange(z, dtype=np.int64)], [np.ones(z, np.int64)], 1)
    return M.axis_taps(w), M.axis_taps(h), tz


def _box_sums(vals, taps):
    """vals [Z, H, W, C] float64 -> the box filter's vol sums (row, acc, vol; no division)."""
    (ix, wx, _), (iy, wy, _), (iz, wz, _) = taps
    vol = None
    for zi, zw in zip(iz, wz):
        r = zw.astype(np.float64)[:, None, None, None] * V._acc_2d(vals[zi], ix, wx, iy, wy)
        vol = r if vol is None else vol + r
    return vol


def _plain_box(level, mip_kind, srgb):
    if mip_kind == VOLUME:
        return V.downsample_volume(level, srgb)
    return np.stack([M.downsample(level[i], srgb) for i in range(level.shape[0])])


def _to_type(m, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        out = m.astype(np.float32)
        return out.astype(np.float16) if dtype == np.float16 else out


def _box(level, mip_kind, srgb):
    plain = _plain_box(level, mip_kind, srgb)
    taps = _box_taps(level, mip_kind)
    (ix, wx, _), (iy, wy, _), (iz, wz, _) = taps
    out = plain.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if level.dtype == np.uint8:
            v = level.astype(np.uint64)
            sa, sp = None, None
            for zi, zw in zip(iz, wz):
                for yi, yw in zip(iy, wy):
                    for xi, xw in zip(ix, wx):
                        wt = (xw.astype(np.uint64)[None, None, :] * yw.astype(np.uint64)[None, :, None]) * zw.astype(np.uint64)[:, None, None]
                        t = v[zi][:, yi][:, :, xi]
                        wa = wt * t[..., 3]
                        p = wa[..., None] * t[..., :3]
                        sa = wa if sa is None else sa + wa
                        sp = p if sp is None else sp + p
            on = sa > 0
            if srgb:
                vals = level[..., 3:4].astype(np.float64) * M.SRGB_LIN[level[..., :3]]
                mean = _box_sums(vals, taps) / sa.astype(np.float64)[..., None]
                w = np.searchsorted(M.SRGB_THR, mean, side="right").astype(np.uint8)
            else:
                safe = np.maximum(sa, np.uint64(1))[..., None]
                w = ((np.uint64(2) * sp + sa[..., None]) // (np.uint64(2) * safe)).astype(np.uint8)
            out[..., :3] = np.where(on[..., None], w, plain[..., :3])
            return out
        vals = level.astype(np.float64)
        vol_p = _box_sums(vals[..., 3:4] * vals[..., :3], taps)
        vol_a = _box_sums(vals[..., 3:4], taps)
        w = _to_type(vol_p / vol_a, level.dtype)
        out[..., :3] = np.where(vol_a > 0.0, w, plain[..., :3])
        return out


def _windowed_sums(vals, kind, edge, mip_kind):
    """vals [Z, H, W, C] float64 -> the separable sums of mip_filter_model.downsample."""
    z, h, w = vals.shape[:3]
    ix, wx, vx = F.axis(kind, edge, w)
    iy, wy, vy = F.axis(kind, edge, h)
    # x pass over every source row (in chunks of rows, to bound the temporaries)
    rows = np.empty((z, h, ix.shape[1], vals.shape[3]), np.float64)
    step = max(1, (1 << 22) // max(1, w))
    for y0 in range(0, h, step):
        v = vals[:, y0:y0 + step]
        rows[:, y0:y0 + step] = F._sum((wx[k][None, None, :, None] * v[:, :, ix[k]], vx[k][None, None, :, None]) for k in range(len(ix)))
    acc = F._sum((wy[k][None, :, None, None] * rows[:, iy[k]], vy[k][None, :, None, None]) for k in range(len(iy)))
    if mip_kind == VOLUME:
        iz, wz, vz = F.axis(kind, edge, z)
        return F._sum((wz[k][:, None, None, None] * acc[iz[k]], vz[k][:, None, None, None]) for k in range(len(iz)))
    return 1.0 * acc


def _windowed(level, kind, edge, mip_kind, srgb):
    plain = F.downsample(level, kind, edge, mip_kind, srgb)
    out = plain.copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if level.dtype == np.uint8:
            a = level[..., 3:4]
            if srgb:
                vals = a.astype(np.float64) * M.SRGB_LIN[level[..., :3]]
            else:
                vals = (a.astype(np.uint32) * level[..., :3].astype(np.uint32)).astype(np.float64)
            vals = np.concatenate([vals, a.astype(np.float64)], axis=-1)
        else:
            f = level.astype(np.float64)
            vals = np.concatenate([f[..., 3:4] * f[..., :3], f[..., 3:4]], axis=-1)
        vol = _windowed_sums(vals, kind, edge, mip_kind)
        vol_a = vol[..., 3:4]
        m = vol[..., :3] / vol_a
        if level.dtype == np.uint8:
            if srgb:
                w = np.searchsorted(M.SRGB_THR, m, side="right").astype(np.uint8)
            else:
                w = np.clip(np.floor(m + 0.5), 0, 255)
                w = np.where(np.isnan(w), 0, w).astype(np.uint8)       # (only where volA > 0.0 fails: not taken)
        else:
            w = _to_type(m, level.dtype)
        out[..., :3] = np.where(vol_a > 0.0, w, plain[..., :3])
        return out


def downsample(level, mip_kind, filter_kind, edge, weight, srgb=False):
    """One level of a [Z, H, W, 4] ARRAY or VOLUME."""
    if weight == NONE:
        return F.chain(level, mip_kind, filter_kind, edge, 2, srgb)[1]
    if filter_kind == BOX:
        return _box(level, mip_kind, srgb)
    return _windowed(level, filter_kind, edge, mip_kind, srgb)


def chain(level0, mip_kind, filter_kind, edge, weight, levels=0, srgb=False):
    """[level 0, level 1, ...] of a [Z, H, W, 4] ARRAY or VOLUME with astcenc_amd_mip_weighting.weight = `weight`."""
    if weight == NONE:
        return F.chain(level0, mip_kind, filter_kind, edge, levels, srgb)
    z, h, w = level0.shape[:3]
    out = [level0]
    for _ in range(1, len(V.level_dims(w, h, z, mip_kind, levels))):
        out.append(downsample(out[-1], mip_kind, filter_kind, edge, weight, srgb))
    return out
