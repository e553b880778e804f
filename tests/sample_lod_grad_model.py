# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_lod_grad_device, written from the comment in include/astcenc_amd.h alone: per point the
forward call's validity, lambda', lambda_c, l0 and g (tests/sample_lod_model.py); the upstream a[c] = grad_out[c] * scale[c] as one
float64 product; per level that is part of the point the forward level sample s_l (sample_lod_model.level_point) and
S_l = sum a[c] s_l[c], and under BILINEAR the differences along x over the forward y taps and along y over the forward x taps --
both indices of the differenced axis always addressed -- summed against a[c] and multiplied by the level's size; grad_coords as
one level's D or the blend of two (two products, one sum, one rounding to float32), grad_lod as S_(l0+1) - S_l0 where lambda' is not
clamped under MIP_LINEAR and +0.0 elsewhere; a NaN gradient is the canonical quiet NaN.  Every product, difference and sum is
one float64 operation (numpy never fuses), every sum starts as its first product.  Nothing here knows how the library does it."""
import math

import numpy as np

import sample_lod_model as L
import sample_model as S

QNAN = np.uint32(0x7FC00000)


def upstream(grad_out, scale):
    """a[..., c] (float64) of grad_out [..., channels] -- float32, float16 or the float32 widening of bfloat16 -- and scale[c]."""
    g = np.asarray(grad_out).astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        return g * np.asarray(scale, dtype=np.float32)[: g.shape[-1]].astype(np.float64)


def _sum(products):
    acc = None
    for p in products:
        acc = p if acc is None else acc + p
    return acc


def level_terms(texels, filter, address_x, address_y, u, v, a):
    """(Dx_l, Dy_l, S_l), float64, of a valid point in the level texels [H, W, 4] for the upstream a[0 .. channels)."""
    H, W = texels.shape[:2]
    with np.errstate(all="ignore"):
        s = L.level_point(texels, filter, address_x, address_y, u, v)
        S_l = _sum(a[c] * np.float64(s[c]) for c in range(len(a)))
        if filter == S.NEAREST:
            return np.float64(0.0), np.float64(0.0), S_l
        x, y = np.float64(np.float32(u)) * np.float64(W), np.float64(np.float32(v)) * np.float64(H)
        ix0, iy0 = int(math.floor(x - np.float64(0.5))), int(math.floor(y - np.float64(0.5)))
        kx = [S.address(address_x, ix0 + k, W) for k in (0, 1)]
        ky = [S.address(address_y, iy0 + k, H) for k in (0, 1)]

        def val(a_, b_, c):
            return np.float64(0.0) if kx[a_] is None or ky[b_] is None else np.float64(texels[ky[b_], kx[a_], c])

        xt, yt = L.axis_taps(filter, x), L.axis_taps(filter, y)
        dsdx = [_sum(w * (val(1, i - iy0, c) - val(0, i - iy0, c)) for i, w in yt) for c in range(len(a))]
        dsdy = [_sum(w * (val(i - ix0, 1, c) - val(i - ix0, 0, c)) for i, w in xt) for c in range(len(a))]
        Dx = _sum(a[c] * dsdx[c] for c in range(len(a))) * np.float64(W)
        Dy = _sum(a[c] * dsdy[c] for c in range(len(a))) * np.float64(H)
        return Dx, Dy, S_l


def unclamped(mip_filter, level_count, lam):
    """grad_lod is a difference of levels: MIP_LINEAR and 0 <= lambda' < level_count - 1."""
    return mip_filter == L.MIP_LINEAR and 0.0 <= float(lam) < float(level_count - 1)


def _store(x):
    """float64 -> the float32 that is stored: one rounding, NaNs canonical."""
    with np.errstate(all="ignore"):
        f = np.asarray(x, dtype=np.float64).astype(np.float32)
    return np.where(np.isnan(f), QNAN.view(np.float32), f).astype(np.float32)


def grad_point(chain, filter, address_x, address_y, mip_filter, u, v, lod, lod_bias, a, want_lod=True):
    """(dL/du, dL/dv, dL/dlod) as float32 of one point; `a` the upstream float64 values of its channels.  want_lod False: grad_lod
    is NULL -- the third value is None and a level of weight zero is not read."""
    zero = np.float32(0.0)
    lam = L.lambda_prime(lod, lod_bias)
    if not L.valid(u, v, lam):
        return zero, zero, (zero if want_lod else None)
    pairs = L.levels(mip_filter, len(chain), lam)
    l0 = pairs[0][0]
    t0 = level_terms(chain[l0], filter, address_x, address_y, u, v, a)
    t1 = None
    with np.errstate(all="ignore"):
        if len(pairs) == 2:
            t1 = level_terms(chain[l0 + 1], filter, address_x, address_y, u, v, a)
            w0, g = pairs[0][1], pairs[1][1]
            gu, gv = _store(w0 * t0[0] + g * t1[0]), _store(w0 * t0[1] + g * t1[1])
        else:
            gu, gv = _store(t0[0]), _store(t0[1])
        if not want_lod:
            return gu[()], gv[()], None
        if not unclamped(mip_filter, len(chain), lam):
            return gu[()], gv[()], zero
        if t1 is None:
            t1 = level_terms(chain[l0 + 1], filter, address_x, address_y, u, v, a)
        return gu[()], gv[()], _store(t1[2] - t0[2])[()]


def grad_pointwise(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias, a, want_lod=True):
    """coords [H, W, 2], lod [H, W] or None, a [H, W, channels] float64 -> grad_coords [H, W, 2], grad_lod [H, W] (or None), float32."""
    coords = np.asarray(coords, dtype=np.float32)
    gc = np.empty(coords.shape[:2] + (2,), dtype=np.float32)
    gl = np.empty(coords.shape[:2], dtype=np.float32) if want_lod else None
    for j in range(coords.shape[0]):
        for i in range(coords.shape[1]):
            r = grad_point(chain, filter, address_x, address_y, mip_filter, coords[j, i, 0], coords[j, i, 1], None if lod is None else lod[j, i], lod_bias, a[j, i], want_lod)
            gc[j, i] = r[:2]
            if want_lod:
                gl[j, i] = r[2]
    return gc, gl


def level_terms_arrays(texels, filter, address_x, address_y, coords, a):
    """level_terms of every point taken as valid (invalid ones at (0, 0)), as array operations: (Dx, Dy, S), float64 [H, W]."""
    coords = np.asarray(coords, dtype=np.float32)
    texels = np.asarray(texels)
    H, W = texels.shape[:2]
    n = a.shape[-1]
    with np.errstate(all="ignore"):
        s = L.level_sample(texels, filter, address_x, address_y, coords).astype(np.float64)
        S_l = _sum(a[..., c] * s[..., c] for c in range(n))
        if filter == S.NEAREST:
            return np.zeros_like(S_l), np.zeros_like(S_l), S_l
        u, v = coords[..., 0].astype(np.float64), coords[..., 1].astype(np.float64)
        fine = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= L.LIMIT) & (np.abs(v) <= L.LIMIT)
        x, y = np.where(fine, u, 0.0) * np.float64(W), np.where(fine, v, 0.0) * np.float64(H)
        kx, wx, two_x = S._axis_arrays(filter, address_x, x, W)
        ky, wy, two_y = S._axis_arrays(filter, address_y, y, H)
        def value(a_, b_):
            inside = (kx[a_] >= 0) & (ky[b_] >= 0)
            val = texels[np.where(inside, ky[b_], 0), np.where(inside, kx[a_], 0)][..., :n].astype(np.float64)      # exact for all three types
            return np.where(inside[..., None], val, 0.0)

        # (a selection, not a product: a tap that is in no sum cannot reach the result)
        dsdx = wy[0][..., None] * (value(1, 0) - value(0, 0))
        dsdx = np.where(two_y[..., None], dsdx + wy[1][..., None] * (value(1, 1) - value(0, 1)), dsdx)
        dsdy = wx[0][..., None] * (value(0, 1) - value(0, 0))
        dsdy = np.where(two_x[..., None], dsdy + wx[1][..., None] * (value(1, 1) - value(1, 0)), dsdy)
        Dx = _sum(a[..., c] * dsdx[..., c] for c in range(n)) * np.float64(W)
        Dy = _sum(a[..., c] * dsdy[..., c] for c in range(n)) * np.float64(H)
        return Dx, Dy, S_l


def grad(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias, a, want_lod=True):
    """grad_pointwise as array operations (tests/test_decode_lod_grad_cpu.py holds the two together): every level is evaluated at
    every point and a point selects its own."""
    coords = np.asarray(coords, dtype=np.float32)
    ok, l0, l1, g = L.level_arrays(mip_filter, len(chain), coords, lod, lod_bias)
    with np.errstate(all="ignore"):
        lam = (np.zeros(coords.shape[:2], dtype=np.float32) if lod is None else np.asarray(lod, dtype=np.float32)) + np.float32(lod_bias)
    slope = ok & (mip_filter == L.MIP_LINEAR) & (lam >= 0.0) & (lam < np.float32(len(chain) - 1))
    upper = np.where(slope & want_lod, l0 + 1, l1)          # the level above l0 whose terms the point needs, -1: none
    zeros = np.zeros(ok.shape, dtype=np.float64)
    t0, t1 = [zeros, zeros, zeros], [zeros, zeros, zeros]
    for l, texels in enumerate(chain):
        if not (ok & ((l0 == l) | (upper == l))).any():
            continue
        t = level_terms_arrays(texels, filter, address_x, address_y, coords, a)
        t0 = [np.where(l0 == l, t[k], t0[k]) for k in range(3)]
        t1 = [np.where(upper == l, t[k], t1[k]) for k in range(3)]
    with np.errstate(all="ignore"):
        w0 = np.float64(1.0) - g
        out = []
        for k in range(2):
            both = w0 * t0[k] + g * t1[k]
            out.append(np.where(ok, _store(np.where(l1 >= 0, both, t0[k])), np.float32(0.0)))
        gc = np.stack(out, axis=-1).astype(np.float32)
        if not want_lod:
            return gc, None
        gl = np.where(slope, _store(t1[2] - t0[2]), np.float32(0.0)).astype(np.float32)
    return gc, gl
