# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_sample_cube_tensors_device, written from the comment in include/astcenc_amd.h alone: per point
lambda' (tests/sample_lod_model.py), the validity rule of a direction, the face and (sc, tc, ma), the two divisions, per level
the face coordinates x = p h + h and y = q h + h, the taps of NEAREST and BILINEAR with the texel each tap reads -- the "Cube
edges" rule as tests/mip_cube_model.py works it out from the face frames, never the library's byte table -- the sums of the
sample call in tap order, the levels, their weights and the blend of the lod call, then scale, bias, storage and placement of the
tensors call (tests/tensor_model.py).  Every operation is one numpy float64 (or float32) operation.  Nothing here knows how the
library does it."""
import math

import numpy as np

import mip_cube_model as Q
import sample_lod_model as L
import sample_model as S
import tensor_model as M

MIP_NEAREST, MIP_LINEAR = L.MIP_NEAREST, L.MIP_LINEAR
NEAREST, BILINEAR = S.NEAREST, S.BILINEAR
FACES = Q.FACES
MAX_FACE = 65536


def valid(d, lam):
    """dx, dy, dz finite, not all three zero (of either sign), lambda' not a NaN."""
    d = [float(np.float32(c)) for c in d]
    return all(math.isfinite(c) for c in d) and any(c != 0.0 for c in d) and not math.isnan(float(lam))


def face_of(d):
    """(face, sc, tc, ma) of a valid direction: float32 components with a sign, ma = |major|."""
    dx, dy, dz = (np.float32(c) for c in d)
    a, b, c = abs(dx), abs(dy), abs(dz)
    if a >= b and a >= c:
        axis, major = 0, dx
    elif b >= c:
        axis, major = 1, dy
    else:
        axis, major = 2, dz
    f = 2 * axis + (1 if major < 0 else 0)
    # d . S_f and d . T_f: the frames have one non-zero component each, so the dot product is that component with a sign
    sc = [np.float32(sg) * comp for sg, comp in zip(Q.SDIR[f], (dx, dy, dz)) if sg != 0][0]
    tc = [np.float32(sg) * comp for sg, comp in zip(Q.TDIR[f], (dx, dy, dz)) if sg != 0][0]
    return f, np.float32(sc), np.float32(tc), np.float32(abs(major))


def quotients(sc, tc, ma):
    """p = sc / ma, q = tc / ma: one float64 division each."""
    return np.float64(sc) / np.float64(ma), np.float64(tc) / np.float64(ma)


def face_coordinate(p, s):
    """x = p h + h with h = s * 0.5: one product, then one sum."""
    h = np.float64(s) * np.float64(0.5)
    ph = np.float64(p) * h
    return ph + h


def axis_taps(filter, x, s):
    """[(index, weight)] in tap order, zero weights left out: NEAREST min(floor(x), s - 1); BILINEAR the sample call's axis rule."""
    if filter == NEAREST:
        return [(min(int(math.floor(x)), s - 1), np.float64(1.0))]
    return L.axis_taps(filter, x)


def point_taps(filter, f, x, y, s):
    """[(wy, [(wx, (face, tx, ty), (ix, iy)), ...]), ...]: rows in y tap order, each row's x taps in order, with the texel a tap
    reads and its indices before the cube rule."""
    rows = []
    for iy, wy in axis_taps(filter, y, s):
        rows.append((wy, [(wx, Q.source(f, ix, iy, s), (ix, iy)) for ix, wx in axis_taps(filter, x, s)]))
    return rows


def level_point(level, cube, filter, f, p, q):
    """s_l[0 .. 3] (float32) of a valid point in the level [6 n, s, s, 4]."""
    s = level.shape[1]
    assert level.shape[2] == s and level.shape[0] % 6 == 0 and 6 * cube + 5 < level.shape[0] and s <= MAX_FACE
    x, y = face_coordinate(p, s), face_coordinate(q, s)
    with np.errstate(all="ignore"):
        acc = None
        for wy, row in point_taps(filter, f, x, y, s):
            r = None
            for wx, (tf, tx, ty), _ in row:
                prod = wx * level[6 * cube + tf, ty, tx].astype(np.float64)
                r = prod if r is None else r + prod
            prod = wy * r
            acc = prod if acc is None else acc + prod
        return acc.astype(np.float32)


def sample_point(chain, cube, filter, mip_filter, d, lod, lod_bias):
    """s[0 .. 3] (float32) of one point of the chain [level [6 n, s_l, s_l, 4] per level]."""
    lam = L.lambda_prime(lod, lod_bias)
    if not valid(d, lam):
        return np.zeros(4, dtype=np.float32)
    f, sc, tc, ma = face_of(d)
    p, q = quotients(sc, tc, ma)
    pairs = L.levels(mip_filter, len(chain), lam)
    s = [level_point(chain[l], cube, filter, f, p, q) for l, _ in pairs]
    if len(pairs) == 1:
        return s[0]
    with np.errstate(all="ignore"):
        p0 = pairs[0][1] * s[0].astype(np.float64)
        p1 = pairs[1][1] * s[1].astype(np.float64)
        return (p0 + p1).astype(np.float32)


def sample(chain, cube, filter, mip_filter, dirs, lod, lod_bias):
    """dirs [out_y, out_x, 3] float32, lod [out_y, out_x] float32 or None -> s [out_y, out_x, 4] float32."""
    dirs = np.asarray(dirs, dtype=np.float32)
    out = np.empty(dirs.shape[:2] + (4,), dtype=np.float32)
    for j in range(dirs.shape[0]):
        for i in range(dirs.shape[1]):
            out[j, i] = sample_point(chain, cube, filter, mip_filter, dirs[j, i], None if lod is None else lod[j, i], lod_bias)
    return out


def convert(chain, cube, filter, mip_filter, dirs, lod, lod_bias, ttype, channels, scale, bias):
    """-> bits [1, out_y, out_x, channels] (the D, H, W, C of tensor_model.scatter)."""
    return M.convert(sample(chain, cube, filter, mip_filter, dirs, lod, lod_bias)[None], ttype, channels, scale, bias)


def direction(f, x, y, s):
    """The float32 direction s M_f + (2x - s) S_f + (2y - s) T_f through the point (x, y) of face f in texel units (texel (k, l) has
    its centre at (k + 0.5, l + 0.5)): exact for dyadic x and y of few bits."""
    u, v = 2.0 * x - s, 2.0 * y - s
    return np.array([s * Q.MAJOR[f][i] + u * Q.SDIR[f][i] + v * Q.TDIR[f][i] for i in range(3)], dtype=np.float32)


def constructed_directions(sizes=(1, 2, 3, 5, 8, 64)):
    """The directions of the hand checks: through x, y in {0, 0.25, 0.5, 1, s - 0.5, s - 0.25, s} (clipped to [0, s]) of every face
    for every s; the ties a = b, b = c, a = c and a = b = c in all sign combinations (the eight corners among them); the six axes;
    components of +-0.0; subnormal components; components of magnitude 3e38; NaN, +-inf and the zero vector in each position."""
    out = []
    for s in sizes:
        marks = sorted({min(max(v, 0.0), float(s)) for v in (0.0, 0.25, 0.5, 1.0, s - 0.5, s - 0.25, float(s))})
        for f in range(6):
            for y in marks:
                for x in marks:
                    out.append(direction(f, x, y, s))
    signs = (1.0, -1.0)
    for sa in signs:
        for sb in signs:
            for third in (0.0, 0.5, -0.5, 2.0, -2.0):
                out += [(sa, sb, third), (third, sa, sb), (sa, third, sb)]          # a = b, b = c, a = c
            for sc in signs:
                out.append((sa, sb, sc))                                            # a = b = c: the corners
    for axis in range(3):
        for sg in signs:
            for z0 in (0.0, -0.0):
                for z1 in (0.0, -0.0):
                    v = [z0, z1]
                    v.insert(axis, sg)
                    out.append(tuple(v))                                            # the axes, zeros of either sign
    tiny, sub, big = np.float32(1e-45), np.float32(3e-39), np.float32(3e38)
    for axis in range(3):
        for m in (tiny, sub, big):
            for other in (0.0, 0.25, -1.0):
                v = [np.float32(other) * m, np.float32(-0.5) * m]
                v.insert(axis, m)
                out.append(tuple(v))
                v = [np.float32(other) * m, np.float32(0.75) * m]
                v.insert(axis, -m)
                out.append(tuple(v))
    # (a subnormal next to normal components, and alone)
    out += [(tiny, 1.0, -2.0), (1.0, sub, 0.5), (tiny, 0.0, 0.0), (0.0, -sub, -0.0), (sub, tiny, -sub)]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            v = [0.5, -0.25]
            v.insert(axis, bad)
            out.append(tuple(v))
    for z0 in (0.0, -0.0):
        for z1 in (0.0, -0.0):
            for z2 in (0.0, -0.0):
                out.append((z0, z1, z2))
    return np.array(out, dtype=np.float32)


def coverage(dirs, sizes, filter=BILINEAR):
    """What the valid directions reach under `filter` over faces of the sizes `sizes`: the (face, side) pairs of taps with one
    index outside (side 0: x < 0, 1: x >= s, 2: y < 0, 3: y >= s), the (face, quadrant) pairs of taps with both outside
    (quadrant = (x >= s) + 2 (y >= s)), the axes on which a second tap of weight zero was left out, and the tie branches taken:
    ("ab", x wins), ("bc", y wins), ("ac", x wins) and the same ties lost to a larger third component."""
    sides, quadrants, zero_axes, ties = set(), set(), set(), set()
    for d in dirs:
        if not valid(d, 0.0):
            continue
        f, sc, tc, ma = face_of(d)
        a, b, c = (abs(np.float32(v)) for v in d)
        if a == b:
            ties.add(("ab", f // 2 == 0) if a >= c else ("ab>c", f // 2 == 2))
        if b == c:
            ties.add(("bc", f // 2 == 1) if b > a else ("bc<=a", f // 2 == 0))
        if a == c:
            ties.add(("ac", f // 2 == 0) if a >= b else ("ac<b", f // 2 == 1))
        p, q = quotients(sc, tc, ma)
        for s in sizes:
            x, y = face_coordinate(p, s), face_coordinate(q, s)
            if filter == BILINEAR:
                if len(axis_taps(filter, x, s)) == 1:
                    zero_axes.add("x")
                if len(axis_taps(filter, y, s)) == 1:
                    zero_axes.add("y")
            for _, row in point_taps(filter, f, x, y, s):
                for _, _, (ix, iy) in row:
                    in_x, in_y = 0 <= ix < s, 0 <= iy < s
                    if in_x and not in_y:
                        sides.add((f, 2 + (iy >= s)))
                    elif in_y and not in_x:
                        sides.add((f, int(ix >= s)))
                    elif not in_x and not in_y:
                        quadrants.add((f, int(ix >= s) + 2 * int(iy >= s)))
    return sides, quadrants, zero_axes, ties
