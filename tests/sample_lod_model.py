# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_lod_tensors_device, written from the comment in include/astcenc_amd.h alone: per point
lambda' = lod + lod_bias (one float32 addition), the validity rule, lambda clamped to the chain, the one level of MIP_NEAREST or
the two levels and their weights of MIP_LINEAR (a level of weight zero left out), per level the exact binary64 level coordinates
u W and v H, the sample of that level as tests/sample_model.py defines it for an entry -- its taps, addressing and sums, with
the level coordinate in the place of the widened binary32 one (sample_model.sample takes binary32 coordinates, so the level form
is written here, pointwise on sample_model.address and as arrays on its axis arrays) -- and the blend: two float64 products and
one float64 sum, one rounding to float32; then scale, bias, storage and placement of the tensors call (tests/tensor_model.py).
Nothing here knows how the library does it."""
import math

import numpy as np

import sample_model as S
import tensor_model as M

MIP_NEAREST, MIP_LINEAR = 0, 1
LIMIT = 2.0 ** 14
MAX_LEVELS = 32


def lambda_prime(lod, lod_bias):
    """lod + lod_bias as one float32 addition; lod None: +0.0."""
    with np.errstate(all="ignore"):
        return np.float32(0.0 if lod is None else lod) + np.float32(lod_bias)


def valid(u, v, lam):
    """u and v finite and no larger than 2^14 in magnitude, lambda' not a NaN."""
    return all(math.isfinite(float(c)) and abs(float(c)) <= LIMIT for c in (u, v)) and not math.isnan(float(lam))


def levels(mip_filter, level_count, lam):
    """[(level, weight)] of a lambda' that is not a NaN, a level of weight zero left out."""
    lc = np.float32(min(max(float(lam), 0.0), float(level_count - 1)))
    if mip_filter == MIP_NEAREST:
        return [(int(math.ceil(np.float64(lc) + np.float64(0.5))) - 1, np.float64(1.0))]
    l0 = int(math.floor(lc))
    g = np.float64(lc) - np.float64(l0)
    if g == 0.0:
        return [(l0, np.float64(1.0))]
    return [(l0, np.float64(1.0) - g), (l0 + 1, g)]


def axis_taps(filter, x):
    """[(index, weight)] in tap order, zero weights left out, of the binary64 level coordinate x along one axis."""
    x = np.float64(x)
    if filter == S.NEAREST:
        return [(int(math.floor(x)), np.float64(1.0))]
    t = x - np.float64(0.5)
    i0 = int(math.floor(t))
    f = t - np.float64(i0)
    taps = [(i0, np.float64(1.0) - f), (i0 + 1, f)]
    return [(i, w) for i, w in taps if w != 0.0]


def level_point(texels, filter, address_x, address_y, u, v):
    """s_l[0 .. 3] (float32) of a valid point in the level texels [H, W, 4]: sample_model.sample_point's sums at (u W, v H)."""
    H, W = texels.shape[:2]
    x, y = np.float64(np.float32(u)) * np.float64(W), np.float64(np.float32(v)) * np.float64(H)
    zero = np.zeros(4, dtype=np.float64)
    with np.errstate(all="ignore"):
        acc = None
        for iy, wy in axis_taps(filter, y):
            ky = S.address(address_y, iy, H)
            r = None
            for ix, wx in axis_taps(filter, x):
                kx = S.address(address_x, ix, W)
                val = zero if kx is None or ky is None else texels[ky, kx].astype(np.float64)
                p = wx * val
                r = p if r is None else r + p
            p = wy * r
            acc = p if acc is None else acc + p
        return acc.astype(np.float32)


def sample_point(chain, filter, address_x, address_y, mip_filter, u, v, lod, lod_bias):
    """s[0 .. 3] (float32) of one point of the chain [texels [H_l, W_l, 4] per level]."""
    lam = lambda_prime(lod, lod_bias)
    if not valid(u, v, lam):
        return np.zeros(4, dtype=np.float32)
    pairs = levels(mip_filter, len(chain), lam)
    s = [level_point(chain[l], filter, address_x, address_y, u, v) for l, _ in pairs]
    if len(pairs) == 1:
        return s[0]
    with np.errstate(all="ignore"):
        p0 = pairs[0][1] * s[0].astype(np.float64)
        p1 = pairs[1][1] * s[1].astype(np.float64)
        return (p0 + p1).astype(np.float32)


def sample_pointwise(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias):
    """coords [out_y, out_x, 2] float32 (u then v), lod [out_y, out_x] float32 or None -> s [out_y, out_x, 4] float32, point by point."""
    coords = np.asarray(coords, dtype=np.float32)
    out = np.empty(coords.shape[:2] + (4,), dtype=np.float32)
    for j in range(coords.shape[0]):
        for i in range(coords.shape[1]):
            out[j, i] = sample_point(chain, filter, address_x, address_y, mip_filter, coords[j, i, 0], coords[j, i, 1], None if lod is None else lod[j, i], lod_bias)
    return out


def level_arrays(mip_filter, level_count, coords, lod, lod_bias):
    """Per point: valid, l0, l1 (-1: one level), g (float64)."""
    coords = np.asarray(coords, dtype=np.float32)
    u, v = coords[..., 0].astype(np.float64), coords[..., 1].astype(np.float64)
    with np.errstate(all="ignore"):
        lam = (np.zeros(coords.shape[:2], dtype=np.float32) if lod is None else np.asarray(lod, dtype=np.float32)) + np.float32(lod_bias)
    assert lam.dtype == np.float32
    ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT) & ~np.isnan(lam)
    lc = np.minimum(np.maximum(np.where(ok, lam, np.float32(0.0)), np.float32(0.0)), np.float32(level_count - 1)).astype(np.float64)
    if mip_filter == MIP_NEAREST:
        l0 = (np.ceil(lc + np.float64(0.5)) - 1.0).astype(np.int64)
        g = np.zeros_like(lc)
    else:
        fl = np.floor(lc)
        l0, g = fl.astype(np.int64), lc - fl
    l1 = np.where(g != 0.0, l0 + 1, -1)
    return ok, l0, l1, g


def level_sample(texels, filter, address_x, address_y, coords):
    """s_l [out_y, out_x, 4] float32 of every point taken as valid (invalid ones at (0, 0)): level_point as array operations -- the
    float64 operations of sample_model.sample in the same order, from the exact products u W and v H."""
    coords = np.asarray(coords, dtype=np.float32)
    texels = np.asarray(texels)
    H, W = texels.shape[:2]
    u, v = coords[..., 0].astype(np.float64), coords[..., 1].astype(np.float64)
    fine = np.isfinite(u) & np.isfinite(v) & (np.abs(u) <= LIMIT) & (np.abs(v) <= LIMIT)
    x, y = np.where(fine, u, 0.0) * np.float64(W), np.where(fine, v, 0.0) * np.float64(H)
    kx, wx, two_x = S._axis_arrays(filter, address_x, x, W)
    ky, wy, two_y = S._axis_arrays(filter, address_y, y, H)
    v64 = texels.astype(np.float64)

    def value(a, b):
        inside = (kx[a] >= 0) & (ky[b] >= 0)
        val = v64[np.where(inside, ky[b], 0), np.where(inside, kx[a], 0)]
        return np.where(inside[..., None], val, 0.0)

    def row(b):
        r = wx[0][..., None] * value(0, b)
        return np.where(two_x[..., None], r + wx[1][..., None] * value(1, b), r)

    with np.errstate(all="ignore"):
        acc = wy[0][..., None] * row(0)
        acc = np.where(two_y[..., None], acc + wy[1][..., None] * row(1), acc)
        return acc.astype(np.float32)


def sample(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias):
    """sample_point for every point, as array operations (tests/test_decode_lod_cpu.py holds the two together): every level is
    sampled at every point and a point selects its own -- a selection, not a product, so a level it does not have cannot reach it."""
    ok, l0, l1, g = level_arrays(mip_filter, len(chain), coords, lod, lod_bias)
    shape = ok.shape + (4,)
    s0, s1 = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    for l, texels in enumerate(chain):
        if not ((l0 == l) | (l1 == l)).any():
            continue
        s = level_sample(texels, filter, address_x, address_y, coords)
        s0 = np.where((l0 == l)[..., None], s, s0)
        s1 = np.where((l1 == l)[..., None], s, s1)
    with np.errstate(all="ignore"):
        w0 = np.float64(1.0) - g
        both = (w0[..., None] * s0.astype(np.float64) + g[..., None] * s1.astype(np.float64)).astype(np.float32)
    out = np.where((l1 >= 0)[..., None], both, s0)
    return np.where(ok[..., None], out, np.float32(0.0)).astype(np.float32)


def convert(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias, ttype, channels, scale, bias):
    """-> bits [1, out_y, out_x, channels] (the D, H, W, C of tensor_model.scatter)."""
    return M.convert(sample(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias)[None], ttype, channels, scale, bias)


def tensor(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias, ttype, layout, channels, scale, bias):
    """The tight tensor of one grid: bits [C, H, W] (planar) or [H, W, C] (interleaved)."""
    t = M.tensor(sample(chain, filter, address_x, address_y, mip_filter, coords, lod, lod_bias)[None], ttype, layout, channels, scale, bias)
    return t[:, 0] if layout == M.PLANAR else t[0]


def chain_dims(dim_x, dim_y, level_count=0):
    """The sizes of the mip chain of a dim_x x dim_y image: level i is max(1, dim >> i); 0 levels: down to 1 x 1."""
    dims = []
    while True:
        dims.append((max(1, dim_x >> len(dims)), max(1, dim_y >> len(dims))))
        if len(dims) == level_count or dims[-1] == (1, 1):
            return dims


def special_coordinates():
    """The normalised coordinates the hand checks name: the edges, a texel centre of a 17-texel axis, -0.0, tiny and negative
    values, the invalid ones with their neighbours."""
    big = np.float32(LIMIT)
    nxt = np.nextafter(big, np.float32(np.inf))
    return np.array([0.5, 0.0, -0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1e-30, -0.25, 1.5 / 17.0, np.nan, np.inf, -np.inf, big, nxt, -big, -nxt],
                    dtype=np.float32)


def special_lambdas(level_count):
    top = level_count - 1
    return np.array([-1.0, 0.0, -0.0, 0.5, 1.0, 1.5, top, top + 3.0, np.inf, -np.inf, np.nan, np.nextafter(np.float32(0.5), np.float32(0.0)),
                     np.nextafter(np.float32(0.5), np.float32(1.0)), 1e-30, top - 0.25], dtype=np.float32)
