# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_decompress_scaled_tensors_device, written from the comment in include/astcenc_amd.h alone: the taps
of every output position from (S, D, position) in Python integers; the window's texels (what the regions call writes) widened to
binary64; per source row the x taps' products summed in tap order, then the y taps' products of those sums, one float64
operation at a time (numpy's float64 multiply and add are IEEE operations and are never fused); one float64 division, one
rounding to float32; then scale, bias, storage and placement of the tensors call (tests/tensor_model.py).  Nothing here knows
how the library does it."""
import numpy as np

import tensor_model as M

BILINEAR, BOX = 0, 1


def taps(filter, S, D, p):
    """([(source index, weight), ...] in tap order without zero weights, den) of output position p along an axis."""
    if filter == BILINEAR:
        n = (2 * p + 1) * S - D
        i0 = n // (2 * D)                      # Python's // is the floor, also for a negative n
        f = n - i0 * 2 * D
        assert 0 <= f < 2 * D
        clamp = lambda v: min(max(v, 0), S - 1)
        t = [(clamp(i0), 2 * D - f), (clamp(i0 + 1), f)]
        den = 2 * D
    else:
        a, b = p * S, (p + 1) * S
        t = [(k, min(b, (k + 1) * D) - max(a, k * D)) for k in range(a // D, (b - 1) // D + 1)]
        assert all(w >= 1 for _, w in t)
        den = S
    assert sum(w for _, w in t) == den
    return [(k, w) for k, w in t if w != 0], den


def resample(texels, filter, out_x, out_y):
    """texels [S_y, S_x, 4] (uint8 / float16 / float32: a window as the regions call writes it) -> s [out_y, out_x, 4] float32."""
    v = np.asarray(texels).astype(np.float64)                  # exact for all three types
    sy, sx = v.shape[:2]
    tx = [taps(filter, sx, out_x, i) for i in range(out_x)]
    ty = [taps(filter, sy, out_y, j) for j in range(out_y)]
    den_x, den_y = tx[0][1], ty[0][1]
    with np.errstate(all="ignore"):
        # r[ky, i]: the x pass of every source row, tap after tap
        r = np.empty((sy, out_x, 4), dtype=np.float64)
        for i, (t, _) in enumerate(tx):
            acc = None
            for k, w in t:
                p = np.float64(w) * v[:, k]
                acc = p if acc is None else acc + p
            r[:, i] = acc
        out = np.empty((out_y, out_x, 4), dtype=np.float64)
        for j, (t, _) in enumerate(ty):
            acc = None
            for k, w in t:
                p = np.float64(w) * r[k]
                acc = p if acc is None else acc + p
            out[j] = acc
        return (out / (np.float64(den_x) * np.float64(den_y))).astype(np.float32)


def convert(texels, filter, out_x, out_y, ttype, channels, scale, bias):
    """A window's texels [S_y, S_x, 4] -> bits [1, out_y, out_x, channels] (the D, H, W, C of tensor_model.scatter)."""
    s = resample(texels, filter, out_x, out_y)[None]
    return M.convert(s, ttype, channels, scale, bias)


def tensor(texels, filter, out_x, out_y, ttype, layout, channels, scale, bias, flags=0):
    """The tight tensor of one region: bits [C, H, W] (planar) or [H, W, C] (interleaved)."""
    t = M.tensor(resample(texels, filter, out_x, out_y)[None], ttype, layout, channels, scale, bias, flags)
    return t[:, 0] if layout == M.PLANAR else t[0]
