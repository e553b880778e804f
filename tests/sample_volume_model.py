# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_volume_tensors_device, written from the comment in include/astcenc_amd.h alone: per point
lambda' and the levels as tests/sample_lod_model.py has them (the comment refers to the lod call for both), the validity rule
with w added, per level the exact binary64 level coordinates u W, v H and w D, on each axis the taps of sample_lod_model.axis_taps
and the addressing of sample_model.address with that axis's mode, a BORDER tap outside on any axis as +0.0, and the sums: a row
per (y tap, z tap) over the x taps, a plane per z tap over the rows, then the z taps over the planes, one float64 operation at a
time, one rounding to float32 per level; then the lod call's blend and the tensors call's scale, bias, storage and placement
(tests/tensor_model.py).  A level is an array [D, H, W, 4].  Nothing here knows how the library does it."""
import math

import numpy as np

import sample_lod_model as L
import sample_model as S
import tensor_model as M

LIMIT = L.LIMIT


def valid(u, v, w, lam):
    """u, v and w finite and no larger than 2^14 in magnitude, lambda' not a NaN."""
    return all(math.isfinite(float(c)) and abs(float(c)) <= LIMIT for c in (u, v, w)) and not math.isnan(float(lam))


def level_coordinates(texels, u, v, w):
    D, H, W = texels.shape[:3]
    return (np.float64(np.float32(u)) * np.float64(W), np.float64(np.float32(v)) * np.float64(H), np.float64(np.float32(w)) * np.float64(D))


def point_taps(texels, filter, address, u, v, w):
    """The taps of a valid point in a level, in sum order: [(kx, ky, kz) or None for a BORDER tap outside] with the tap slot
    (x tap + 2 * y tap + 4 * z tap); taps of weight zero are not among them."""
    D, H, W = texels.shape[:3]
    x, y, z = level_coordinates(texels, u, v, w)
    taps = []
    for c, (iz, _) in enumerate(L.axis_taps(filter, z)):
        for b, (iy, _) in enumerate(L.axis_taps(filter, y)):
            for a, (ix, _) in enumerate(L.axis_taps(filter, x)):
                k = (S.address(address[0], ix, W), S.address(address[1], iy, H), S.address(address[2], iz, D))
                taps.append((a + 2 * b + 4 * c, None if None in k else k))
    return taps


def level_point(texels, filter, address, u, v, w):
    """s_l[0 .. 3] (float32) of a valid point in the level texels [D, H, W, 4]; address = (address_x, address_y, address_z)."""
    D, H, W = texels.shape[:3]
    x, y, z = level_coordinates(texels, u, v, w)
    zero = np.zeros(4, dtype=np.float64)
    with np.errstate(all="ignore"):
        acc = None
        for iz, wz in L.axis_taps(filter, z):
            kz = S.address(address[2], iz, D)
            plane = None
            for iy, wy in L.axis_taps(filter, y):
                ky = S.address(address[1], iy, H)
                r = None
                for ix, wx in L.axis_taps(filter, x):
                    kx = S.address(address[0], ix, W)
                    val = zero if kx is None or ky is None or kz is None else texels[kz, ky, kx].astype(np.float64)
                    p = wx * val
                    r = p if r is None else r + p
                p = wy * r
                plane = p if plane is None else plane + p
            p = wz * plane
            acc = p if acc is None else acc + p
        return acc.astype(np.float32)


def sample_point(chain, filter, address, mip_filter, u, v, w, lod, lod_bias):
    """s[0 .. 3] (float32) of one point of the chain [texels [D_l, H_l, W_l, 4] per level]."""
    lam = L.lambda_prime(lod, lod_bias)
    if not valid(u, v, w, lam):
        return np.zeros(4, dtype=np.float32)
    pairs = L.levels(mip_filter, len(chain), lam)
    s = [level_point(chain[l], filter, address, u, v, w) for l, _ in pairs]
    if len(pairs) == 1:
        return s[0]
    with np.errstate(all="ignore"):
        p0 = pairs[0][1] * s[0].astype(np.float64)
        p1 = pairs[1][1] * s[1].astype(np.float64)
        return (p0 + p1).astype(np.float32)


def sample_pointwise(chain, filter, address, mip_filter, coords, lod, lod_bias):
    """coords [out_y, out_x, 3] float32, lod [out_y, out_x] float32 or None -> s [out_y, out_x, 4] float32, point by point."""
    coords = np.asarray(coords, dtype=np.float32)
    out = np.empty(coords.shape[:2] + (4,), dtype=np.float32)
    for j in range(coords.shape[0]):
        for i in range(coords.shape[1]):
            out[j, i] = sample_point(chain, filter, address, mip_filter, coords[j, i, 0], coords[j, i, 1], coords[j, i, 2], None if lod is None else lod[j, i], lod_bias)
    return out


def _fine(coords):
    c = np.asarray(coords, dtype=np.float32).astype(np.float64)
    return (np.isfinite(c) & (np.abs(c) <= LIMIT)).all(axis=-1)


def level_arrays(mip_filter, level_count, coords, lod, lod_bias):
    """Per point: valid, l0, l1 (-1: one level), g (float64): sample_lod_model.level_arrays with w among the coordinates."""
    coords = np.asarray(coords, dtype=np.float32)
    ok, l0, l1, g = L.level_arrays(mip_filter, level_count, coords[..., :2], lod, lod_bias)
    fine = _fine(coords)
    # (a point that w alone makes invalid: its lambda was clamped as a valid one's, which only selects levels nobody stores)
    return ok & fine, l0, l1, g


def level_sample(texels, filter, address, coords):
    """s_l [out_y, out_x, 4] float32 of every point taken as valid (invalid ones at (0, 0, 0)): level_point as array operations."""
    coords = np.asarray(coords, dtype=np.float32)
    texels = np.asarray(texels)
    D, H, W = texels.shape[:3]
    fine = _fine(coords)
    c64 = np.where(fine[..., None], coords.astype(np.float64), 0.0)
    x, y, z = c64[..., 0] * np.float64(W), c64[..., 1] * np.float64(H), c64[..., 2] * np.float64(D)
    kx, wx, two_x = S._axis_arrays(filter, address[0], x, W)
    ky, wy, two_y = S._axis_arrays(filter, address[1], y, H)
    kz, wz, two_z = S._axis_arrays(filter, address[2], z, D)
    v64 = texels.astype(np.float64)

    def value(a, b, c):
        inside = (kx[a] >= 0) & (ky[b] >= 0) & (kz[c] >= 0)
        val = v64[np.where(inside, kz[c], 0), np.where(inside, ky[b], 0), np.where(inside, kx[a], 0)]
        return np.where(inside[..., None], val, 0.0)

    def row(b, c):
        r = wx[0][..., None] * value(0, b, c)
        return np.where(two_x[..., None], r + wx[1][..., None] * value(1, b, c), r)

    def plane(c):
        p = wy[0][..., None] * row(0, c)
        return np.where(two_y[..., None], p + wy[1][..., None] * row(1, c), p)

    with np.errstate(all="ignore"):
        acc = wz[0][..., None] * plane(0)
        acc = np.where(two_z[..., None], acc + wz[1][..., None] * plane(1), acc)
        return acc.astype(np.float32)


def sample(chain, filter, address, mip_filter, coords, lod, lod_bias):
    """sample_point for every point, as array operations (tests/test_decode_volume_cpu.py holds the two together): every level
    some point has is sampled at every point and a point selects its own."""
    ok, l0, l1, g = level_arrays(mip_filter, len(chain), coords, lod, lod_bias)
    shape = ok.shape + (4,)
    s0, s1 = np.zeros(shape, dtype=np.float32), np.zeros(shape, dtype=np.float32)
    for l, texels in enumerate(chain):
        if not (ok & ((l0 == l) | (l1 == l))).any():
            continue
        s = level_sample(texels, filter, address, coords)
        s0 = np.where((l0 == l)[..., None], s, s0)
        s1 = np.where((l1 == l)[..., None], s, s1)
    with np.errstate(all="ignore"):
        w0 = np.float64(1.0) - g
        both = (w0[..., None] * s0.astype(np.float64) + g[..., None] * s1.astype(np.float64)).astype(np.float32)
    out = np.where((l1 >= 0)[..., None], both, s0)
    return np.where(ok[..., None], out, np.float32(0.0)).astype(np.float32)


def tensor(chain, filter, address, mip_filter, coords, lod, lod_bias, ttype, layout, channels, scale, bias):
    """The tight tensor of one grid: bits [C, H, W] (planar) or [H, W, C] (interleaved)."""
    t = M.tensor(sample(chain, filter, address, mip_filter, coords, lod, lod_bias)[None], ttype, layout, channels, scale, bias)
    return t[:, 0] if layout == M.PLANAR else t[0]


def texel_centres(texels):
    """coords [D * H, W, 3] float32 of the texel centres of a level, slice by slice, row by row."""
    D, H, W = texels.shape[:3]
    c = np.empty((D, H, W, 3), dtype=np.float64)
    c[..., 0] = ((np.arange(W) + 0.5) / W)[None, None, :]
    c[..., 1] = ((np.arange(H) + 0.5) / H)[None, :, None]
    c[..., 2] = ((np.arange(D) + 0.5) / D)[:, None, None]
    return c.reshape(D * H, W, 3).astype(np.float32)


# ---- the inputs the tests share (tests/test_decode_volume_cpu.py asserts what they reach, tests/test_decode_volume.py runs them) ----

CHAIN = [(20, 14, 9), (10, 7, 4), (5, 3, 2), (2, 1, 1), (1, 1, 1)]      # (W, H, D) per level
GRIDS = [(70, 1), (33, 3), (19, 11)]                                    # 64 x 1, 16 x 4 and 8 x 8 tiles, each with a ragged last tile
FOOTPRINTS_2D = [(4, 4, 1), (6, 6, 1), (8, 5, 1)]
FOOTPRINTS_3D = [(3, 3, 3), (4, 4, 3), (5, 5, 4), (6, 6, 6)]


def constructed_points(footprint):
    """Triples that reach the named cases on level 0 of CHAIN: a second tap of weight zero on each axis separately (2.5 of 20,
    3.5 of 14, 4.5 of 9), all three at once, the eight taps of a point in one block and in eight blocks of `footprint`, the
    unit cube's corners, and invalid points of every kind with their valid neighbours."""
    W, H, D = CHAIN[0]
    bx, by, bz = footprint
    big = np.float32(LIMIT)
    nxt = np.nextafter(big, np.float32(np.inf))
    pts = [(0.125, 0.3, 0.3), (0.3, 0.25, 0.3), (0.3, 0.3, 0.5), (0.125, 0.25, 0.5),
           (1.0 / W, 1.0 / H, 1.0 / D), (bx / W, by / H, min(bz, D - 1) / D),
           (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.0, 1.0, -0.0), (1.0, 0.0, 1.0)]
    for axis in range(3):
        for bad in (np.nan, np.inf, -np.inf, nxt, -nxt):
            p = [0.4, 0.6, 0.2]
            p[axis] = bad
            pts.append(tuple(p))
        for good in (big, -big):
            p = [0.4, 0.6, 0.2]
            p[axis] = good
            pts.append(tuple(p))
    return np.array(pts, dtype=np.float32)


def seeded_points(rng, n):
    """Half near faces, edges and corners of the unit cube -- one, two or three coordinates within 0.08 of 0 or 1, inside and
    outside -- the rest anywhere in [-1.5, 2.5]."""
    near = rng.uniform(0.0, 1.0, size=(n // 2, 3))
    snap = rng.integers(0, 2, size=near.shape).astype(bool)
    snap[np.arange(len(near)), rng.integers(0, 3, size=len(near))] = True
    at = rng.integers(0, 2, size=near.shape) + rng.uniform(-0.08, 0.08, size=near.shape)
    near = np.where(snap, at, near)
    anywhere = rng.uniform(-1.5, 2.5, size=(n - n // 2, 3))
    pts = np.concatenate([near, anywhere]).astype(np.float32)
    return pts[rng.permutation(n)]


def seeded_lods(rng, shape, levels, keep=0):
    """Lambdas over [-1, levels + 0.5] with integers, halves, the infinities and a NaN among them; the first `keep` are +0.0."""
    lod = rng.uniform(-1.0, levels + 0.5, size=shape).astype(np.float32)
    flat = lod.reshape(-1)
    keep = min(keep, flat.size)
    rest = keep + rng.permutation(flat.size - keep)
    whole = rest[:len(rest) // 8]
    flat[whole] = np.floor(flat[whole])
    special = np.array([0.0, 1.0, levels - 1.0, np.inf, -np.inf, 0.5, 1.5, np.nan, -0.0, 2.0], dtype=np.float32)
    at = rest[len(whole):len(whole) + len(special)]
    flat[at] = special[:len(at)]
    flat[:keep] = 0.0
    return lod


def grid_inputs(seed, ox, oy, footprint, levels=len(CHAIN)):
    """coords [oy, ox, 3] and lod [oy, ox] of the grid the tests name by (seed, size, footprint): the constructed points first,
    at lambda 0, then seeded ones."""
    rng = np.random.default_rng(seed)
    c = constructed_points(footprint)
    pts = seeded_points(rng, ox * oy)
    k = min(len(c), ox * oy)
    pts[:k] = c[:k]
    return pts.reshape(oy, ox, 3), seeded_lods(rng, (oy, ox), levels, keep=k)


def tile_points(ox, oy):
    """The (j, i) index arrays of the points of every tile of an ox x oy grid, tile by tile."""
    tw, th = S.tile_shape(oy)
    for j0 in range(0, oy, th):
        for i0 in range(0, ox, tw):
            yield [(j, i) for j in range(j0, min(j0 + th, oy)) for i in range(i0, min(i0 + tw, ox))]


def coverage(dims, footprint, filter, address, mip_filter, coords, lod, lod_bias):
    """What a grid reaches on the chain of sizes `dims`, from the model alone: the set of (axis, side) with a tap index outside
    (side 0 below 0, 1 above S - 1), the axes on which some point has a second tap of weight zero while the other two axes have
    two taps, the set of distinct-block counts over a point's taps (a BORDER tap outside has no block), the most distinct
    blocks any tile's pass over one level lists, whether some valid point blends two levels / has g = 0, and the invalid points."""
    coords = np.asarray(coords, dtype=np.float32)
    oy, ox = coords.shape[:2]
    outside, zero_axes, block_counts, most, blended, single, invalid = set(), set(), set(), 0, False, False, 0
    bx, by, bz = footprint
    for tile in tile_points(ox, oy):
        per_level = {}
        for j, i in tile:
            u, v, w = coords[j, i]
            lam = L.lambda_prime(None if lod is None else lod[j, i], lod_bias)
            if not valid(u, v, w, lam):
                invalid += 1
                continue
            pairs = L.levels(mip_filter, len(dims), lam)
            if mip_filter == L.MIP_LINEAR:
                blended = blended or len(pairs) == 2
                single = single or len(pairs) == 1
            for l, _ in pairs:
                W, H, D = dims[l]
                x, y, z = np.float64(u) * W, np.float64(v) * H, np.float64(w) * D
                taps = [L.axis_taps(filter, c) for c in (x, y, z)]
                blocks = set()
                for axis, (ts, size) in enumerate(zip(taps, (W, H, D))):
                    for idx, _ in ts:
                        if idx < 0:
                            outside.add((axis, 0))
                        if idx > size - 1:
                            outside.add((axis, 1))
                    if filter == S.BILINEAR and len(ts) == 1 and all(len(o) == 2 for k, o in enumerate(taps) if k != axis):
                        zero_axes.add(axis)
                for iz, _ in taps[2]:
                    for iy, _ in taps[1]:
                        for ix, _ in taps[0]:
                            k = (S.address(address[0], ix, W), S.address(address[1], iy, H), S.address(address[2], iz, D))
                            if None not in k:
                                blocks.add((k[0] // bx, k[1] // by, k[2] // bz))
                if l == 0 and len(taps[0]) * len(taps[1]) * len(taps[2]) == 8:
                    block_counts.add(len(blocks))
                per_level.setdefault(l, set()).update(blocks)
        most = max([most] + [len(b) for b in per_level.values()])
    return outside, zero_axes, block_counts, most, blended, single, invalid
