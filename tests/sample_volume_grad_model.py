# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_volume_grad_device, written from the comment in include/astcenc_amd.h alone, on top of
tests/sample_volume_model.py (the forward call: validity, levels, level coordinates, the level sample) and
tests/sample_lod_grad_model.py (the upstream a[c], the storage, the rule of grad_lod): per level that is part of the point
S_l = sum a[c] s_l[c] and, under BILINEAR, the differences along each axis -- both indices of the differenced axis always
addressed, with that axis's mode -- summed over the forward taps of the two other axes, innermost over the first remaining axis,
then against a[c], then multiplied by the level's size along the axis; grad_coords as one level's D or the blend of two (two
products, one sum, one rounding to float32), grad_lod as S_(l0+1) - S_l0 where lambda' is not clamped under MIP_LINEAR and +0.0
elsewhere.  Every product, difference and sum is one float64 operation (numpy never fuses), every sum starts as its first
product.  A level is an array [D, H, W, 4].  Nothing here knows how the library does it."""
import math

import numpy as np

import sample_lod_grad_model as G
import sample_lod_model as L
import sample_model as S
import sample_volume_model as V

QNAN = G.QNAN
upstream = G.upstream
unclamped = G.unclamped
_sum = G._sum
_store = G._store


def level_terms(texels, filter, address, u, v, w, a):
    """(Dx_l, Dy_l, Dz_l, S_l), float64, of a valid point in the level texels [D, H, W, 4] for the upstream a[0 .. channels);
    address = (address_x, address_y, address_z)."""
    D, H, W = texels.shape[:3]
    n = len(a)
    with np.errstate(all="ignore"):
        s = V.level_point(texels, filter, address, u, v, w)
        S_l = _sum(a[c] * np.float64(s[c]) for c in range(n))
        if filter == S.NEAREST:
            zero = np.float64(0.0)
            return zero, zero, zero, S_l
        x, y, z = V.level_coordinates(texels, u, v, w)
        i0 = [int(math.floor(t - np.float64(0.5))) for t in (x, y, z)]
        k = [[S.address(address[axis], i0[axis] + t, size) for t in (0, 1)] for axis, size in enumerate((W, H, D))]

        def val(ta, tb, tc, c):
            if k[0][ta] is None or k[1][tb] is None or k[2][tc] is None:
                return np.float64(0.0)
            return np.float64(texels[k[2][tc], k[1][tb], k[0][ta], c])

        xt, yt, zt = (L.axis_taps(filter, t) for t in (x, y, z))
        # (a forward tap (index, weight) of an axis is tap index - i0 of that axis)
        dsdx = [_sum(wz * _sum(wy * (val(1, iy - i0[1], iz - i0[2], c) - val(0, iy - i0[1], iz - i0[2], c)) for iy, wy in yt) for iz, wz in zt) for c in range(n)]
        dsdy = [_sum(wz * _sum(wx * (val(ix - i0[0], 1, iz - i0[2], c) - val(ix - i0[0], 0, iz - i0[2], c)) for ix, wx in xt) for iz, wz in zt) for c in range(n)]
        dsdz = [_sum(wy * _sum(wx * (val(ix - i0[0], iy - i0[1], 1, c) - val(ix - i0[0], iy - i0[1], 0, c)) for ix, wx in xt) for iy, wy in yt) for c in range(n)]
        Dx = _sum(a[c] * dsdx[c] for c in range(n)) * np.float64(W)
        Dy = _sum(a[c] * dsdy[c] for c in range(n)) * np.float64(H)
        Dz = _sum(a[c] * dsdz[c] for c in range(n)) * np.float64(D)
        return Dx, Dy, Dz, S_l


def grad_point(chain, filter, address, mip_filter, u, v, w, lod, lod_bias, a, want_lod=True):
    """(dL/du, dL/dv, dL/dw, dL/dlod) as float32 of one point; `a` the upstream float64 values of its channels.  want_lod False:
    grad_lod is NULL -- the fourth value is None and a level of weight zero is not read."""
    zero = np.float32(0.0)
    lam = L.lambda_prime(lod, lod_bias)
    if not V.valid(u, v, w, lam):
        return zero, zero, zero, (zero if want_lod else None)
    pairs = L.levels(mip_filter, len(chain), lam)
    l0 = pairs[0][0]
    t0 = level_terms(chain[l0], filter, address, u, v, w, a)
    t1 = None
    with np.errstate(all="ignore"):
        if len(pairs) == 2:
            t1 = level_terms(chain[l0 + 1], filter, address, u, v, w, a)
            w0, g = pairs[0][1], pairs[1][1]
            gc = [_store(w0 * t0[k] + g * t1[k])[()] for k in range(3)]
        else:
            gc = [_store(t0[k])[()] for k in range(3)]
        if not want_lod:
            return gc[0], gc[1], gc[2], None
        if not unclamped(mip_filter, len(chain), lam):
            return gc[0], gc[1], gc[2], zero
        if t1 is None:
            t1 = level_terms(chain[l0 + 1], filter, address, u, v, w, a)
        return gc[0], gc[1], gc[2], _store(t1[3] - t0[3])[()]


def grad_pointwise(chain, filter, address, mip_filter, coords, lod, lod_bias, a, want_lod=True):
    """coords [H, W, 3], lod [H, W] or None, a [H, W, channels] float64 -> grad_coords [H, W, 3], grad_lod [H, W] (or None), float32."""
    coords = np.asarray(coords, dtype=np.float32)
    gc = np.empty(coords.shape[:2] + (3,), dtype=np.float32)
    gl = np.empty(coords.shape[:2], dtype=np.float32) if want_lod else None
    for j in range(coords.shape[0]):
        for i in range(coords.shape[1]):
            r = grad_point(chain, filter, address, mip_filter, coords[j, i, 0], coords[j, i, 1], coords[j, i, 2], None if lod is None else lod[j, i], lod_bias, a[j, i],
                           want_lod)
            gc[j, i] = r[:3]
            if want_lod:
                gl[j, i] = r[3]
    return gc, gl


def level_terms_arrays(texels, filter, address, coords, a):
    """level_terms of every point taken as valid (invalid ones at (0, 0, 0)), as array operations: (Dx, Dy, Dz, S), float64 [H, W]."""
    coords = np.asarray(coords, dtype=np.float32)
    texels = np.asarray(texels)
    D, H, W = texels.shape[:3]
    n = a.shape[-1]
    with np.errstate(all="ignore"):
        s = V.level_sample(texels, filter, address, coords).astype(np.float64)
        S_l = _sum(a[..., c] * s[..., c] for c in range(n))
        if filter == S.NEAREST:
            return np.zeros_like(S_l), np.zeros_like(S_l), np.zeros_like(S_l), S_l
        fine = V._fine(coords)
        c64 = np.where(fine[..., None], coords.astype(np.float64), 0.0)
        x, y, z = c64[..., 0] * np.float64(W), c64[..., 1] * np.float64(H), c64[..., 2] * np.float64(D)
        kx, wx, two_x = S._axis_arrays(filter, address[0], x, W)
        ky, wy, two_y = S._axis_arrays(filter, address[1], y, H)
        kz, wz, two_z = S._axis_arrays(filter, address[2], z, D)

        def value(ta, tb, tc):
            inside = (kx[ta] >= 0) & (ky[tb] >= 0) & (kz[tc] >= 0)
            val = texels[np.where(inside, kz[tc], 0), np.where(inside, ky[tb], 0), np.where(inside, kx[ta], 0)][..., :n].astype(np.float64)    # exact for all three types
            return np.where(inside[..., None], val, 0.0)

        def over(w_, two, p0, p1):
            # (a selection, not a product: a tap that is in no sum cannot reach the result; p1 is formed only to be selected from)
            r = w_[0][..., None] * p0()
            return np.where(two[..., None], r + w_[1][..., None] * p1(), r)

        dsdx = over(wz, two_z, lambda: over(wy, two_y, lambda: value(1, 0, 0) - value(0, 0, 0), lambda: value(1, 1, 0) - value(0, 1, 0)),
                    lambda: over(wy, two_y, lambda: value(1, 0, 1) - value(0, 0, 1), lambda: value(1, 1, 1) - value(0, 1, 1)))
        dsdy = over(wz, two_z, lambda: over(wx, two_x, lambda: value(0, 1, 0) - value(0, 0, 0), lambda: value(1, 1, 0) - value(1, 0, 0)),
                    lambda: over(wx, two_x, lambda: value(0, 1, 1) - value(0, 0, 1), lambda: value(1, 1, 1) - value(1, 0, 1)))
        dsdz = over(wy, two_y, lambda: over(wx, two_x, lambda: value(0, 0, 1) - value(0, 0, 0), lambda: value(1, 0, 1) - value(1, 0, 0)),
                    lambda: over(wx, two_x, lambda: value(0, 1, 1) - value(0, 1, 0), lambda: value(1, 1, 1) - value(1, 1, 0)))
        Dx = _sum(a[..., c] * dsdx[..., c] for c in range(n)) * np.float64(W)
        Dy = _sum(a[..., c] * dsdy[..., c] for c in range(n)) * np.float64(H)
        Dz = _sum(a[..., c] * dsdz[..., c] for c in range(n)) * np.float64(D)
        return Dx, Dy, Dz, S_l


def grad(chain, filter, address, mip_filter, coords, lod, lod_bias, a, want_lod=True):
    """grad_pointwise as array operations (tests/test_decode_volume_grad_cpu.py holds the two together): every level some point
    needs is evaluated at every point and a point selects its own."""
    coords = np.asarray(coords, dtype=np.float32)
    ok, l0, l1, g = V.level_arrays(mip_filter, len(chain), coords, lod, lod_bias)
    with np.errstate(all="ignore"):
        lam = (np.zeros(coords.shape[:2], dtype=np.float32) if lod is None else np.asarray(lod, dtype=np.float32)) + np.float32(lod_bias)
    slope = ok & (mip_filter == L.MIP_LINEAR) & (lam >= 0.0) & (lam < np.float32(len(chain) - 1))
    upper = np.where(slope & want_lod, l0 + 1, l1)          # the level above l0 whose terms the point needs, -1: none
    zeros = np.zeros(ok.shape, dtype=np.float64)
    t0, t1 = [zeros] * 4, [zeros] * 4
    for l, texels in enumerate(chain):
        if not (ok & ((l0 == l) | (upper == l))).any():
            continue
        t = level_terms_arrays(texels, filter, address, coords, a)
        t0 = [np.where(l0 == l, t[k], t0[k]) for k in range(4)]
        t1 = [np.where(upper == l, t[k], t1[k]) for k in range(4)]
    with np.errstate(all="ignore"):
        w0 = np.float64(1.0) - g
        out = []
        for k in range(3):
            both = w0 * t0[k] + g * t1[k]
            out.append(np.where(ok, _store(np.where(l1 >= 0, both, t0[k])), np.float32(0.0)))
        gc = np.stack(out, axis=-1).astype(np.float32)
        if not want_lod:
            return gc, None
        gl = np.where(slope, _store(t1[3] - t0[3]), np.float32(0.0)).astype(np.float32)
    return gc, gl
