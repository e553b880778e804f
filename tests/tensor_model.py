# SPDX-License-Identifier: Apache-2.0
"""numpy model of astcenc_amd_decompress_tensors_device, written from the comment in include/astcenc_amd.h alone: the texels the
regions call writes (the entry's data type) -> binary32 exactly -> * scale -> + bias, each rounded to binary32 -> the bits of the
tensor's type (F32 as it is, F16 / BF16 round to nearest even, NaNs canonical) -> their place, mirrored, planar or interleaved.
Everything is integer views and one float32 operation at a time; nothing here knows how the library does it."""
import numpy as np

F32, F16, BF16 = 0, 1, 2
PLANAR, INTERLEAVED = 0, 1
FLIP_X, FLIP_Y = 1, 2
BITS_DTYPE = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
CANONICAL_NAN = {F32: 0x7FC00000, F16: 0x7E00, BF16: 0x7FC0}


def bf16_bits(u):
    """uint32 bits of finite or infinite binary32 values -> bfloat16 bits, round to nearest even (integer arithmetic)."""
    u = u.astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def store_bits(y, ttype):
    """float32 array -> the bits it is stored as."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    u = y.view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    if ttype == F32:
        bits = u.copy()
    elif ttype == F16:
        with np.errstate(all="ignore"):
            bits = np.where(nan, np.float32(0), y).astype(np.float16).view(np.uint16)     # IEEE: nearest even, overflow to infinity, subnormals
    else:
        bits = bf16_bits(np.where(nan, np.uint32(0), u))
    bits = bits.astype(BITS_DTYPE[ttype])
    bits[nan] = CANONICAL_NAN[ttype]
    return bits


def convert(texels, ttype, channels, scale, bias):
    """texels [..., 4] of uint8 / float16 / float32 (a crop of what the regions call writes) -> bits [..., channels]."""
    s = np.asarray(texels)[..., :channels].astype(np.float32)          # exact for all three types
    with np.errstate(all="ignore"):
        t = s * np.asarray(scale[:channels], dtype=np.float32)         # rounded to float32
        y = t + np.asarray(bias[:channels], dtype=np.float32)          # rounded to float32
    assert t.dtype == np.float32 and y.dtype == np.float32
    return store_bits(y, ttype)


def tight_pitches(size, layout, channels, row_pitch=0, slice_pitch=0, plane_pitch=0):
    sx, sy, sz = size
    row = row_pitch or (sx if layout == PLANAR else sx * channels)
    sl = slice_pitch or row * sy
    plane = plane_pitch or sl * sz
    return row, sl, plane


def scatter(buf, offset, bits, layout, flags=0, row_pitch=0, slice_pitch=0, plane_pitch=0):
    """Writes bits [D, H, W, C] into the flat element array `buf` with element (c, k, j, i) = (0, 0, 0, 0) at `offset`."""
    d, h, w, ch = bits.shape
    row, sl, plane = tight_pitches((w, h, d), layout, ch, row_pitch, slice_pitch, plane_pitch)
    k, j, i, c = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), np.arange(ch), indexing="ij")
    i2 = (w - 1 - i) if flags & FLIP_X else i
    j2 = (h - 1 - j) if flags & FLIP_Y else j
    at = c * plane + k * sl + j2 * row + i2 if layout == PLANAR else k * sl + j2 * row + i2 * ch + c
    buf[offset + at.ravel()] = bits.ravel()


def tensor(texels, ttype, layout, channels, scale, bias, flags=0):
    """The tight tensor of one window: bits [C, D, H, W] (planar) or [D, H, W, C] (interleaved) of texels [D, H, W, 4]."""
    bits = convert(texels, ttype, channels, scale, bias)
    d, h, w, ch = bits.shape
    out = np.zeros(d * h * w * ch, dtype=bits.dtype)
    scatter(out, 0, bits, layout, flags)
    return out.reshape((ch, d, h, w) if layout == PLANAR else (d, h, w, ch))
