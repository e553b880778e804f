# SPDX-License-Identifier: Apache-2.0
"""Shared by tests/test_straight_stages_cpu.py and tests/test_straight_stages.py: one 96x96 image (256 blocks at 6x6) per
branch of the ideal-endpoint and endpoint-format stages that works on registers instead of LDS cells (csrc/wave_ideal.h,
csrc/wave_format.h), and what it takes to show from the reference's own output that the branch was taken.

  component subsets   RGB noise with constant alpha (3 components; the two-plane trials fit 2 + 1), luminance + alpha,
                      full RGBA noise (4 components; the two-plane trials fit 3 + 1)
  partition counts    two-, three- and four-colour patches at 6x6 -thorough: every arm of combine_partitions_for_quant
  HDR                 RGBA16F at 6x6 -medium
  footprints          10x8 (more than 64 texels: the generic build), 5x5 -medium (on the GPU: a run-time build)

Not a conftest and not a test module: a plain module, imported by name."""
import numpy as np

import astcenc_amd as A

SIZE = 96
MIN_BLOCKS = 8          # blocks of the wanted kind the reference's output must hold

PALETTE = np.array([[200, 60, 40, 230], [30, 70, 210, 120], [40, 200, 70, 250], [230, 220, 50, 60]], dtype=np.int64)
HUES = np.array([[255, 60, 40, 255], [40, 80, 255, 255], [50, 255, 70, 255], [250, 240, 50, 255]], dtype=np.int64)


def rgb_noise(seed=21):
    img = np.random.default_rng(seed).integers(0, 256, size=(SIZE, SIZE, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def luminance_alpha(seed=22):
    rng = np.random.default_rng(seed)
    img = np.empty((SIZE, SIZE, 4), dtype=np.uint8)
    img[..., 0] = img[..., 1] = img[..., 2] = rng.integers(0, 256, size=(SIZE, SIZE), dtype=np.uint8)
    img[..., 3] = rng.integers(0, 256, size=(SIZE, SIZE), dtype=np.uint8)
    return img


def rgba_noise(seed=23):
    return np.random.default_rng(seed).integers(0, 256, size=(SIZE, SIZE, 4), dtype=np.uint8)


def _hash52(p):
    """(ASTC specification, partition pattern generation: the 32-bit mixing function)"""
    m = 0xFFFFFFFF
    p ^= p >> 15; p = (p - (p << 17)) & m; p = (p + (p << 7)) & m; p = (p + (p << 4)) & m
    p ^= p >> 5; p = (p + (p << 16)) & m; p ^= p >> 7; p ^= p >> 3
    p = (p ^ (p << 6)) & m; p ^= p >> 17
    return p


def partition_of_texel(seed, x, y, count):
    """The partition of texel (x, y) in pattern `seed` for `count` partitions, 2D blocks of 31 texels or more (ASTC
    specification, partition pattern generation)."""
    seed += (count - 1) * 1024
    rnum = _hash52(seed)
    s = [(rnum >> sh) & 0xF for sh in (0, 4, 8, 12, 16, 20, 24, 28)]
    s = [v * v for v in s]
    if seed & 1:
        sh1, sh2 = (4 if seed & 2 else 5), (6 if count == 3 else 5)
    else:
        sh1, sh2 = (6 if count == 3 else 5), (4 if seed & 2 else 5)
    s = [v >> (sh1 if i % 2 == 0 else sh2) for i, v in enumerate(s)]
    a = (s[0] * x + s[1] * y + (rnum >> 14)) & 0x3F
    b = (s[2] * x + s[3] * y + (rnum >> 10)) & 0x3F
    c = (s[4] * x + s[5] * y + (rnum >> 6)) & 0x3F if count >= 3 else 0
    d = (s[6] * x + s[7] * y + (rnum >> 2)) & 0x3F if count >= 4 else 0
    if a >= b and a >= c and a >= d:
        return 0
    if b >= c and b >= d:
        return 1
    return 2 if c >= d else 3


def patches(colours, seed):
    """Every 6x6 block is cut into `colours` regions along one of the format's own partition patterns (one in which every
    region has at least five texels); a region has a colour of its own and varies along a channel of its own, so that no two
    regions share a line in colour space and the block wants `colours` partitions."""
    rng = np.random.default_rng(seed)
    patterns = []
    for pattern_seed in range(1024):
        cut = np.array([[partition_of_texel(pattern_seed, x, y, colours) for x in range(6)] for y in range(6)])
        if min(int((cut == k).sum()) for k in range(colours)) >= 5:
            patterns.append(cut)
    which = np.empty((SIZE, SIZE), dtype=np.int64)
    for by in range(SIZE // 6):
        for bx in range(SIZE // 6):
            which[by * 6:by * 6 + 6, bx * 6:bx * 6 + 6] = patterns[int(rng.integers(0, len(patterns)))]
    if colours == 4:
        # (four partitions leave four integers per endpoint pair -- 18 in all is the format's limit --: opaque hues that
        #  vary in brightness, which is what the RGB-scale endpoint format stores in four)
        img = (HUES[which] * rng.integers(40, 101, size=(SIZE, SIZE, 1))) // 100
        img[..., 3] = 255
        return img.astype(np.uint8)
    img = PALETTE[which] + rng.integers(-3, 4, size=(SIZE, SIZE, 4))
    swing = rng.integers(-50, 51, size=(SIZE, SIZE))
    for k in range(colours):
        img[..., k] += np.where(which == k, swing, 0)
    return np.clip(img, 0, 255).astype(np.uint8)


def hdr_rgba16f(seed=24):
    return A.synthetic_hdr_image(SIZE, SIZE, seed)


# name -> (image, block, quality, profile, what the reference's output must show: ("partitions", n) / ("dual", None) / None)
def cases():
    return {
        "rgb_const_alpha": (rgb_noise(), (6, 6), A.PRE_MEDIUM, A.PRF_LDR, None),
        "luminance_alpha": (luminance_alpha(), (6, 6), A.PRE_MEDIUM, A.PRF_LDR, None),
        "rgba": (rgba_noise(), (6, 6), A.PRE_MEDIUM, A.PRF_LDR, ("dual", None)),
        "two_colours": (patches(2, 31), (6, 6), A.PRE_THOROUGH, A.PRF_LDR, ("partitions", 2)),
        "three_colours": (patches(3, 32), (6, 6), A.PRE_THOROUGH, A.PRF_LDR, ("partitions", 3)),
        "four_colours": (patches(4, 33), (6, 6), A.PRE_THOROUGH, A.PRF_LDR, ("partitions", 4)),
        "hdr_rgba16f": (hdr_rgba16f(), (6, 6), A.PRE_MEDIUM, A.PRF_HDR, None),
        "footprint_10x8": (rgba_noise(25), (10, 8), A.PRE_MEDIUM, A.PRF_LDR, None),
        "footprint_5x5": (rgba_noise(26), (5, 5), A.PRE_MEDIUM, A.PRF_LDR, None),
    }


NAMES = ["rgb_const_alpha", "luminance_alpha", "rgba", "two_colours", "three_colours", "four_colours", "hdr_rgba16f",
         "footprint_10x8", "footprint_5x5"]


def block_headers(blocks):
    """(partition count, two weight planes) of every block of a 2D ASTC stream; (0, False) for a constant-colour block.
    (ASTC specification, block mode layout: bits 0-10 the mode, bits 11-12 the partition count less one)"""
    out = []
    for b in np.asarray(blocks, dtype=np.uint8).reshape(-1, 16):
        word = int(b[0]) | (int(b[1]) << 8)
        mode = word & 0x7FF
        if (mode & 0x1FF) == 0x1FC:
            out.append((0, False))
            continue
        # (the one layout without a D bit: bits 0-1 zero and bits 7-8 "10")
        no_d_bit = (mode & 0x3) == 0 and ((mode >> 7) & 0x3) == 0x2
        dual = not no_d_bit and bool((mode >> 10) & 1)
        out.append((((word >> 11) & 0x3) + 1, dual))
    return out


def coverage(blocks, what):
    """How many blocks of `blocks` are of the kind `what` asks for."""
    kind, n = what
    headers = block_headers(blocks)
    if kind == "partitions":
        return sum(1 for pc, _ in headers if pc == n)
    return sum(1 for _, dual in headers if dual)


class Reference:
    """The reference's bytes of every case, compressed once per session and never changed."""

    def __init__(self, ref):
        self.ref = ref
        self.cases = cases()
        self.bytes = {}

    def want(self, name):
        if name not in self.bytes:
            img, block, quality, profile, _ = self.cases[name]
            out = self.ref.compress(img, block, quality, profile=profile)
            out.setflags(write=False)
            self.bytes[name] = out
        return self.bytes[name]
