# SPDX-License-Identifier: Apache-2.0
"""numpy model of the mip chain options of include/astcenc_amd.h (csrc/mip_post.h), bit for bit.

levels(options) == post(levels(no options)): the chain of tests/mip_model.py / tests/mip_model_3d.py, then, on levels 1 .. n-1,
  * NORMALIZE: channels 0-2 renormalised as unit vectors (float64, one IEEE operation at a time, true division, IEEE sqrt);
  * ALPHA_COVERAGE: per surface (a level of a 2D image or volume, a (level, layer) of an array) the alpha remapped so that the
    covered share of level 0 is kept; the target count k uses Python integers.

Shared by tests/test_mip_options_cpu.py (against the header compiled with g++) and tests/test_mip_options.py (against the GPU)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402

NORMALIZE, ALPHA_COVERAGE = 0x1, 0x2
ARRAY, VOLUME = V.ARRAY, V.VOLUME


# ---- NORMALIZE ----

def normalize_u8(rgb):
    """uint8 [..., 3] -> the renormalised codes."""
    v = (2 * rgb.astype(np.int64) - 255).astype(np.float64) / 255.0
    len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
    n = v / np.sqrt(len2)[..., None]
    q = np.floor((n + 1.0) * 127.5 + 0.5)
    return np.clip(q, 0, 255).astype(np.uint8)


def normalize_float(rgb):
    """float16 / float32 [..., 3] -> renormalised (a texel whose len2 is 0 or not finite keeps its bits)."""
    v = 2.0 * rgb.astype(np.float64) - 1.0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        len2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        ok = np.isfinite(len2) & (len2 != 0)
        n = v / np.sqrt(np.where(ok, len2, 1.0))[..., None]
        out = ((n + 1.0) * 0.5).astype(np.float32)
    if rgb.dtype == np.float16:
        out = out.astype(np.float16)
    res = rgb.copy()
    res[ok] = out[ok]
    return res


def normalize(level):
    """A level [..., 4]: channels 0-2 renormalised, channel 3 kept."""
    out = level.copy()
    out[..., :3] = normalize_u8(level[..., :3]) if level.dtype == np.uint8 else normalize_float(level[..., :3])
    return out


# ---- ALPHA_COVERAGE ----

def u8_threshold(cutoff):
    c = float(np.float32(cutoff)) * 255.0
    return next(t for t in range(1, 256) if float(t) >= c or t == 255)


def bounds(cutoff, dtype):
    """(hi, lo): the smallest / largest value of dtype that is >= / < cutoff, as float32."""
    c = np.float32(cutoff)
    if dtype == np.float32:
        return c, np.float32(np.nextafter(c, np.float32(0)))
    h = np.float16(c)
    if np.float32(h) < c:
        h = np.nextafter(h, np.float16(np.inf))
    return np.float32(h), np.float32(np.nextafter(h, np.float16(0)))


def covered(alpha, cutoff):
    """Boolean mask of the covered alphas (uint8 codes or floats)."""
    if alpha.dtype == np.uint8:
        return alpha >= u8_threshold(cutoff)
    with np.errstate(invalid="ignore"):
        return alpha.astype(np.float64) >= float(np.float32(cutoff))


def target(c0, n, n0):
    return (2 * int(c0) * int(n) + int(n0)) // (2 * int(n0))


def keys(alpha):
    """Order-preserving integer keys (NaN -> 0, below everything)."""
    if alpha.dtype == np.uint8:
        return alpha.astype(np.int64)
    bits = alpha.view(np.uint16 if alpha.dtype == np.float16 else np.uint32).astype(np.int64)
    sign = 0x8000 if alpha.dtype == np.float16 else 0x80000000
    full = 2 * sign - 1
    k = np.where(bits & sign, ~bits & full, bits | sign)
    return np.where(np.isnan(alpha), 0, k)


def kth_largest(alpha, k):
    """The k-th largest alpha (1-based, ties counted individually) by the keys above."""
    order = np.argsort(-keys(alpha.ravel()), kind="stable")
    return alpha.ravel()[order[k - 1]]


def remap_u8(a, ak, t):
    a = a.astype(np.int64)
    q = (2 * a * t + int(ak)) // (2 * int(ak))
    return np.where(a >= int(ak), np.minimum(255, q), np.minimum(t - 1, q)).astype(np.uint8)


def remap_float(a, ak, cutoff, dtype):
    hi, lo = bounds(cutoff, dtype)
    c = float(np.float32(cutoff))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        r = ((a.astype(np.float64) * c) / float(ak)).astype(np.float32)
        if dtype == np.float16:
            r = r.astype(np.float16).astype(np.float32)
        up = a.astype(np.float64) >= float(ak)
        out = np.where(up, np.maximum(hi, np.minimum(r, np.float32(1.0))), np.minimum(r, lo)).astype(dtype)
    return np.where(np.isnan(a), a, out)


def cover_surface(surface_alpha, c0, n0, cutoff):
    """The remapped alphas of one surface (any shape) whose level-0 surface has c0 of n0 texels covered."""
    k = target(c0, surface_alpha.size, n0)
    if k == 0:
        return surface_alpha.copy()
    ak = kth_largest(surface_alpha, k)
    if surface_alpha.dtype == np.uint8:
        if ak == 0:
            return surface_alpha.copy()
        return remap_u8(surface_alpha, ak, u8_threshold(cutoff))
    if not (np.isfinite(ak) and ak > 0):
        return surface_alpha.copy()
    return remap_float(surface_alpha, ak, cutoff, surface_alpha.dtype.type)


# ---- the whole chain ----

def post(levels, kind, flags, cutoff=0.5):
    """levels: the plain chain ([Z, H, W, 4] per level, level 0 first) of an ARRAY or a VOLUME (a 2D image: a VOLUME of depth
    1) -> the chain with the options applied.  Level 0 is returned as it is."""
    out = [levels[0]]
    layers = levels[0].shape[0] if kind == ARRAY else 1
    top = [levels[0][l] if kind == ARRAY else levels[0] for l in range(layers)]
    c0 = [int(covered(t[..., 3], cutoff).sum()) for t in top]
    n0 = top[0][..., 3].size
    for lv in levels[1:]:
        lv = lv.copy()
        if flags & NORMALIZE:
            lv = normalize(lv)
        if flags & ALPHA_COVERAGE:
            for l in range(layers):
                surf = lv[l] if kind == ARRAY else lv
                surf[..., 3] = cover_surface(surf[..., 3], c0[l], n0, cutoff)
        out.append(lv)
    return out


def chain(level0, kind, flags, cutoff=0.5, levels=0):
    """The chain of level0 ([Z, H, W, 4]) with options, from the plain filter's models."""
    plain = V.chain_array(level0, levels) if kind == ARRAY else V.chain_volume(level0, levels)
    return post(plain, kind, flags, cutoff)
