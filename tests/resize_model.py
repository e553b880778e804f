# SPDX-License-Identifier: Apache-2.0
"""numpy / Python-float model of astcenc_amd_resize_image_device (include/astcenc_amd.h, csrc/mip_resize.h), bit for bit.

Built on the chain's models (mip_model.py, mip_filter_model.py): their filter functions, sRGB tables, masked sums and half
conversions.  New here are the taps of a general ratio -- the windowed kinds with c = (2j + 1) s / (2d) and scale = max(r, 1),
the box as exact integer overlaps over den = s / gcd(s, d), an axis that keeps its size (or has one texel) as one tap of 1.0 --
and astcenc_amd_resize_dims in Python integers.  The sums are the chain's: float64 row / acc / vol in increasing tap order, each
starting at its first product and masked where a texel has fewer taps; exact integers for the box on U8 data.

Shared by tests/test_resize_cpu.py (against the header compiled with g++) and tests/test_resize.py (against the GPU)."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_filter_model as F  # noqa: E402

BOX, MITCHELL, LANCZOS3, KAISER = F.BOX, F.MITCHELL, F.LANCZOS3, F.KAISER
CLAMP, WRAP = F.CLAMP, F.WRAP
ARRAY, VOLUME = F.ARRAY, F.VOLUME
NONE, ALPHA = 0, 1
FILTERS = (BOX, MITCHELL, LANCZOS3, KAISER)
POW2_NONE, POW2_NEAREST, POW2_NEXT, POW2_PREVIOUS = 0, 1, 2, 3


def passes(s, d):
    return s <= 1 or d == s


def box_taps(s, d, j):
    """(first, [integer weights], den) of the box."""
    g = math.gcd(s, d)
    sp, dp = s // g, d // g
    lo, hi = j * sp, (j + 1) * sp
    first, last = lo // dp, (hi - 1) // dp
    return first, [min((i + 1) * dp, hi) - max(i * dp, lo) for i in range(first, last + 1)], sp


def window_taps(kind, s, d, j):
    """(first, [float weights]) of a windowed kind."""
    r = float(s) / float(d)
    scale = r if d < s else 1.0
    c = float((2 * j + 1) * s) / float(2 * d)
    S = float(F.support(kind))

    def at(i):
        t = ((float(i) + 0.5) - c) / scale
        return -t if t < 0.0 else t

    lo, hi = math.floor(c - S * scale) - 2, math.floor(c + S * scale) + 2
    while not at(lo) < S:
        lo += 1
    while not at(hi) < S:
        hi -= 1
    f = [F.evaluate(kind, at(i)) for i in range(lo, hi + 1)]
    total = f[0]
    for v in f[1:]:
        total = total + v
    return lo, [v / total for v in f]


def taps(kind, s, d, j):
    """(first tap index, [weights], den) of destination texel j along an axis of s source texels made into d."""
    if passes(s, d):
        return (0 if s <= 1 else j), [1.0], 1
    if kind == BOX:
        first, w, den = box_taps(s, d, j)
        return first, [float(v) for v in w], den
    first, w = window_taps(kind, s, d, j)
    return first, w, 1


@functools.lru_cache(maxsize=64)
def axis(kind, edge, s, d):
    """(idx [K, d] source texels, w [K, d] float64, valid [K, d], den) of every destination texel, K the largest tap count."""
    rows = [taps(kind, s, d, j) for j in range(d)]
    k = max(len(w) for _, w, _ in rows)
    idx = np.zeros((k, d), np.int64)
    w = np.zeros((k, d), np.float64)
    valid = np.zeros((k, d), bool)
    for j, (first, ws, _) in enumerate(rows):
        n = len(ws)
        idx[:n, j] = [F.source(first + t, s, edge) for t in range(n)]
        w[:n, j] = ws
        valid[:n, j] = True
    return idx, w, valid, rows[0][2]


def _one_tap(n):
    return np.arange(n, dtype=np.int64)[None], np.ones((1, n), np.float64), np.ones((1, n), bool), 1


def _sum(terms, ints):
    """Integers: a plain sum (absent taps have weight 0, which is exact).  Floats: mip_filter_model._sum."""
    if not ints:
        return F._sum(terms)
    out = None
    for prod, _ in terms:
        out = prod if out is None else out + prod
    return out


def _sums(vals, ax, ay, az, ints=False):
    """vals [Z, H, W, C] (float64, or uint64 with ints) -> vol [Dz, Dy, Dx, C]: row over x, acc over y, vol over z."""
    t = np.uint64 if ints else np.float64
    (ix, wx, vx, _), (iy, wy, vy, _), (iz, wz, vz, _) = ax, ay, az
    z, h = vals.shape[:2]
    with np.errstate(invalid="ignore", over="ignore"):
        rows = np.empty((z, h, ix.shape[1], vals.shape[3]), t)
        step = max(1, (1 << 21) // max(1, ix.shape[1]))
        for y0 in range(0, h, step):
            v = vals[:, y0:y0 + step]
            rows[:, y0:y0 + step] = _sum(((wx[k].astype(t)[None, None, :, None] * v[:, :, ix[k]], vx[k][None, None, :, None])
                                          for k in range(len(ix))), ints)
        acc = np.empty((z, iy.shape[1]) + rows.shape[2:], t)
        step = max(1, (1 << 21) // max(1, ix.shape[1]))
        for y0 in range(0, iy.shape[1], step):
            y1 = y0 + step
            acc[:, y0:y1] = _sum(((wy[k, y0:y1].astype(t)[None, :, None, None] * rows[:, iy[k, y0:y1]], vy[k, y0:y1][None, :, None, None])
                                  for k in range(len(iy))), ints)
        del rows
        return _sum(((wz[k].astype(t)[:, None, None, None] * acc[iz[k]], vz[k][:, None, None, None]) for k in range(len(iz))), ints)


def _round_mean(s, den):
    den = np.uint64(den) if not isinstance(den, np.ndarray) else den
    return (np.uint64(2) * s + den) // (np.uint64(2) * den)


def _to_type(m, dtype):
    with np.errstate(over="ignore", invalid="ignore"):
        out = m.astype(np.float32)
        return out.astype(np.float16) if dtype == np.float16 else out


def resize(level, size, mip_kind=VOLUME, kind=LANCZOS3, edge=CLAMP, weight=NONE, srgb=False):
    """level [Z, H, W, 4] -> [d, h, w, 4] of the same dtype; size = (w, h) (depth or layers kept) or (w, h, d)."""
    z, h, w = level.shape[:3]
    ow, oh, od = (tuple(size) + (z,))[:3]
    assert mip_kind == VOLUME or od == z
    ax, ay = axis(kind, edge, w, ow), axis(kind, edge, h, oh)
    az = axis(kind, edge, z, od) if mip_kind == VOLUME else _one_tap(z)
    u8, box = level.dtype == np.uint8, kind == BOX
    den = ax[3] * ay[3] * az[3]
    dden = (float(ax[3]) * float(ay[3])) * float(az[3])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if u8:
            a = level[..., 3:4]
            lin = M.SRGB_LIN[level[..., :3]] if srgb else level[..., :3].astype(np.float64)
            ac = a.astype(np.float64) * lin if srgb else (a.astype(np.uint32) * level[..., :3].astype(np.uint32)).astype(np.float64)
            fvals = np.concatenate([lin, a.astype(np.float64)] + ([ac] if weight == ALPHA else []), axis=-1)
        else:
            f = level.astype(np.float64)
            fvals = np.concatenate([f] + ([f[..., 3:4] * f[..., :3]] if weight == ALPHA else []), axis=-1)
        vol = _sums(fvals, ax, ay, az)
        if u8 and box:
            # exact integers: the channels and, weighted, alpha x channel
            c = level.astype(np.uint64)
            ivals = np.concatenate([c] + ([c[..., 3:4] * c[..., :3]] if weight == ALPHA else []), axis=-1)
            isum = _sums(ivals, ax, ay, az, ints=True)
            out = _round_mean(isum[..., :4], den).astype(np.uint8)
            sa = isum[..., 3:4]
            if srgb:
                out[..., :3] = np.searchsorted(M.SRGB_THR, vol[..., :3] / dden, side="right").astype(np.uint8)
                if weight == ALPHA:
                    wc = np.searchsorted(M.SRGB_THR, vol[..., 4:7] / sa.astype(np.float64), side="right").astype(np.uint8)
                    out[..., :3] = np.where(sa > 0, wc, out[..., :3])
            elif weight == ALPHA:
                wc = _round_mean(isum[..., 4:7], np.maximum(sa, np.uint64(1))).astype(np.uint8)
                out[..., :3] = np.where(sa > 0, wc, out[..., :3])
            return out
        if box:
            plain = vol[..., :4] / dden
        else:
            plain = vol[..., :4]
        m = vol[..., 4:7] / vol[..., 3:4] if weight == ALPHA else None
        on = vol[..., 3:4] > 0.0
        if u8:
            out = np.clip(np.floor(plain + 0.5), 0, 255).astype(np.uint8)
            if srgb:
                out[..., :3] = np.searchsorted(M.SRGB_THR, plain[..., :3], side="right").astype(np.uint8)
            if weight == ALPHA:
                if srgb:
                    wc = np.searchsorted(M.SRGB_THR, m, side="right").astype(np.uint8)
                else:
                    wc = np.clip(np.floor(m + 0.5), 0, 255)
                    wc = np.where(np.isnan(wc), 0, wc).astype(np.uint8)       # (only where volA > 0.0 fails: not taken)
                out[..., :3] = np.where(on, wc, out[..., :3])
            return out
        out = _to_type(plain, level.dtype)
        if weight == ALPHA:
            out[..., :3] = np.where(on, _to_type(m, level.dtype), out[..., :3])
        return out


def _pow2(v, mode):
    prev = 1 << (v.bit_length() - 1)
    if mode == POW2_PREVIOUS or prev == v:
        return prev
    if mode == POW2_NEXT:
        return 2 * prev
    return prev if v - prev < 2 * prev - v else 2 * prev


def resize_dims(x, y, max_dim=0, pow2=POW2_NONE):
    """astcenc_amd_resize_dims: (out_x, out_y), or None for ASTCENC_ERR_BAD_PARAM."""
    if x <= 0 or y <= 0 or pow2 not in (0, 1, 2, 3):
        return None
    v, L = [x, y], max(x, y)
    if max_dim and L > max_dim:
        v = [max_dim if t == L else max(1, (t * max_dim + L // 2) // L) for t in v]
    if pow2:
        p = [_pow2(t, pow2) for t in v]
        v = [_pow2(t, POW2_PREVIOUS) if max_dim and q > max_dim else q for t, q in zip(v, p)]
    if max(v) > 1 << 31:
        return None
    return tuple(v)
