# SPDX-License-Identifier: Apache-2.0
"""Shared by tests/test_encoding_coverage_cpu.py and tests/test_encoding_coverage.py: the coverage matrix -- which encodings
(columns: the features of tests/block_census.py) the reference must emit in which kernel build class (rows: contexts, each
chosen for the build it launches) -- and the small seeded images that fill it.  Every image is at most 10x10 blocks (4x4x4
blocks for a volume) and is generated at test time.

Not a conftest and not a test module: a plain module, imported by name.

Where to add an image: when a search stage gets a build or an arm of its own, find the feature its blocks end with
(python tests/block_census.py cases), and if the class's count is below MIN_BLOCKS add a generator to IMAGES_LDR / IMAGES_HDR /
IMAGES_3D (and a row to ROWS for a new build), then write profiles/encoding_coverage/census_after.txt again;
tests/test_encoding_coverage_cpu.py then holds the cell at MIN_BLOCKS."""
import collections
import os

import numpy as np

import astcenc_amd as A
from straight_stages_cases import HUES, MIN_BLOCKS, PALETTE, _hash52

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS_BEFORE = os.path.join(ROOT, "profiles", "encoding_coverage", "census_before.txt")
CENSUS_AFTER = os.path.join(ROOT, "profiles", "encoding_coverage", "census_after.txt")

BLOCKS = 10             # blocks along an edge of a 2D image
BLOCKS_3D = 4           # ... of a volume

# ---- rows: row -> (profile, block, quality, kernel build, build class) ----------------------------------------------------
K = "astc_compress_blocks_"
ROWS = collections.OrderedDict([
    ("R1", (A.PRF_LDR, (6, 6), A.PRE_MEDIUM, K + "ldr_6x6m", "ldr_6x6m")),
    ("R2", (A.PRF_LDR, (8, 8), A.PRE_THOROUGH, K + "ldr_8x8t", "ldr_8x8t")),
    ("R3", (A.PRF_HDR, (6, 6), A.PRE_MEDIUM, K + "hdr_6x6m", "hdr_6x6m")),
    ("R4", (A.PRF_LDR, (6, 6), A.PRE_THOROUGH, K + "ldr64", "ldr64")),
    ("R5", (A.PRF_LDR, (4, 4), A.PRE_THOROUGH, K + "ldr64", "ldr64")),      # fewer than 31 texels: the small-block partition hash
    ("R6", (A.PRF_LDR, (10, 8), A.PRE_THOROUGH, K + "ldr", "ldr")),
    ("R7", (A.PRF_LDR, (12, 12), A.PRE_THOROUGH, K + "ldr", "ldr")),
    ("R8", (A.PRF_HDR, (6, 6), A.PRE_THOROUGH, K + "hdr64", "hdr64")),
    ("R9", (A.PRF_HDR_RGB_LDR_A, (6, 6), A.PRE_THOROUGH, K + "hdr64", "hdr64")),
    ("R10", (A.PRF_HDR, (10, 8), A.PRE_THOROUGH, K + "hdr", "hdr")),
    ("R13", (A.PRF_HDR_RGB_LDR_A, (10, 8), A.PRE_THOROUGH, K + "hdr", "hdr")),
    ("R11", (A.PRF_LDR, (4, 4, 4), A.PRE_THOROUGH, K + "ldr64", "3d")),     # 64 texels: the build of the small 2D footprints
    ("R12", (A.PRF_LDR, (6, 6, 6), A.PRE_THOROUGH, K + "ldr", "3d")),
])
CLASSES = ["ldr_6x6m", "ldr_8x8t", "hdr_6x6m", "ldr64", "ldr", "hdr64", "hdr", "3d"]
GENERIC_OF_FIXED = {"R1": K + "ldr64", "R2": K + "ldr64", "R3": K + "hdr64"}       # with ASTCENC_AMD_KERNEL=generic
JIT_ROWS = ["R5", "R6", "R9", "R10", "R11"]      # one row per generic class on a run-time build (a fixed-context build has none)


def build_class(profile, block, quality):
    """The build class of a context with default settings (csrc/backend_hip.hip, kernel_variants)."""
    hdr = profile in (A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)
    if len(block) > 2 and block[2] > 1:
        return "3d"
    if tuple(block[:2]) == (6, 6) and quality == A.PRE_MEDIUM and profile in (A.PRF_LDR, A.PRF_HDR):
        return "hdr_6x6m" if hdr else "ldr_6x6m"
    if tuple(block[:2]) == (8, 8) and quality == A.PRE_THOROUGH and profile == A.PRF_LDR:
        return "ldr_8x8t"
    small = block[0] * block[1] <= 64
    return ("hdr" if hdr else "ldr") + ("64" if small else "")


# ---- columns ------------------------------------------------------------------------------------------------------------
LDR_FORMATS = (0, 4, 5, 6, 8, 9, 10, 12, 13)
HDR_FORMATS = (2, 3, 7, 11, 14, 15)


def columns(hdr):
    """Every feature of the matrix for an LDR or an HDR class: the formats its profiles emit (the reference's HDR search
    proposes HDR formats only), blue contraction for the LDR formats that have it, and the profile's constant-colour block."""
    out = ["partitions:%d" % n for n in (1, 2, 3, 4)]
    out += ["partitions:%d:%s" % (n, s) for n in (2, 3, 4) for s in ("same", "mixed")]
    out += ["plane2:%d" % c for c in range(4)]
    out += ["format:%d" % f for f in (HDR_FORMATS if hdr else LDR_FORMATS)]
    if not hdr:
        out += ["blue:%d:%s" % (f, s) for f in (8, 9, 12, 13) for s in ("on", "off")]
    out += ["kind:void_fp16" if hdr else "kind:void_ldr"]
    out += ["wq:%d" % q for q in range(12)]
    out += ["cq:%d" % q for q in range(4, 21)]
    return out


# Cells that must hold MIN_BLOCKS blocks whatever the sweep reached, (class, feature):
MANDATORY = [("ldr64", "partitions:4"), ("ldr", "partitions:4"), ("hdr64", "partitions:4"), ("hdr", "partitions:4"),
             ("hdr64", "kind:void_fp16"), ("hdr", "kind:void_fp16")]


# ... and per row, not per class: the partition hash and the texel loops depend on the footprint (fewer than 31 texels, more
# than 64, a third axis), so every -thorough row by itself holds MIN_BLOCKS blocks of each partition count.
ROW_MANDATORY = ["partitions:2", "partitions:3", "partitions:4"]


def read_census(path):
    """{class: {feature: blocks}} of a file written by block_census.format_census."""
    lines = [ln for ln in open(path).read().split("\n") if ln and not ln.startswith("#")]
    names = lines[0].split()[1:]
    table = {n: {} for n in names}
    for ln in lines[2:]:
        cells = ln.split()
        for n, v in zip(names, cells[1:]):
            table[n][cells[0]] = int(v)
    return table


def mandatory_cells():
    """MANDATORY, and every cell the sweep tools' matrices reached with MIN_BLOCKS blocks in that class
    (profiles/encoding_coverage/census_before.txt: python tests/block_census.py sweep)."""
    cells = list(MANDATORY)
    before = read_census(CENSUS_BEFORE)
    for cls in CLASSES:
        hdr = cls.startswith("hdr")
        for feature in columns(hdr):
            if before[cls].get(feature, 0) >= MIN_BLOCKS and (cls, feature) not in cells:
                cells.append((cls, feature))
    return cells


# Encodings the reference's search cannot produce: feature -> (reference file and lines, why).
BY_CONSTRUCTION = {
    "plane2:partitions:2": ("Source/astcenc_compress_symbolic.cpp:1326-1372",
                            "compress_block tries two weight planes only in its one-partition pass (compress_symbolic_block_for_partition_2planes is called from the loop before the partition-count loop, never inside it)"),
    "plane2:partitions:3": ("Source/astcenc_compress_symbolic.cpp:1326-1372", "as for two partitions"),
    "format:1": ("Source/astcenc_color_quantize.cpp, pack_color_endpoints",
                 "its switch has no case for FMT_LUMINANCE_DELTA, and compute_color_error_for_every_integer_count_and_quant_level never proposes it"),
}

# Cells the reference did not reach after a real attempt: (classes, features, what was tried and what explains it).  No
# mandatory cell may be here, and the CPU test fails when one of these is in fact reached with MIN_BLOCKS blocks.
_NOT_REACHED = [
    (("ldr_6x6m", "hdr_6x6m"), ("partitions:4", "partitions:4:same", "partitions:4:mixed"),
     "four_patches / hdr_four_patches / mixed_patches4 at 6x6 -medium give none: config_init sets tune_partition_count_limit = 3 "
     "for -medium (read back from the reference's config), so the search never tries four partitions in these two builds"),
    (("ldr_6x6m", "hdr_6x6m"), ("wq:9", "wq:10"),
     "gray / rgb / rgba ramps (which give wq:9 to wq:11 at -thorough), noise in one to four channels and the sweep's own six "
     "image classes (2380 + 1200 blocks) give no block with 20 or 24 weight levels at 6x6 -medium; wq:11 is reached"),
    (("ldr_6x6m",), ("cq:17",),
     "2 blocks over all images (rgb_ramps gives 15 at 8x8 -thorough); the sweep's 2380 blocks of this context hold 4"),
    (("hdr_6x6m",), ("format:14",),
     "the class's rows are PRF_HDR, which stores alpha as HDR: pick_best_endpoint_format proposes format 15 for four components "
     "there and format 14 only with PRF_HDR_RGB_LDR_A (Source/astcenc_pick_best_endpoint_format.cpp:522, :542), whose 6x6 -medium "
     "context is not this build"),
    (("hdr_6x6m", "hdr64", "hdr"), ("cq:4", "cq:5", "cq:6", "cq:7"),
     "none over 26 images in five contexts nor in the sweep's 31 160 HDR blocks: the HDR error table is filled from 16 colour "
     "levels up only, every coarser level keeps the default (worst) error (Source/astcenc_pick_best_endpoint_format.cpp:515-520)"),
]
NOT_REACHED = {(cls, feature): tried for classes, features_, tried in _NOT_REACHED for cls in classes for feature in features_}


# ---- images ---------------------------------------------------------------------------------------------------------------


def partition_of_texel(seed, x, y, z, count, small):
    """The partition of texel (x, y, z) in pattern `seed` for `count` partitions (ASTC specification, partition pattern
    generation); small: the block has fewer than 31 texels."""
    if small:
        x, y, z = x << 1, y << 1, z << 1
    seed += (count - 1) * 1024
    rnum = _hash52(seed)
    s = [(rnum >> sh) & 0xF for sh in (0, 4, 8, 12, 16, 20, 24, 28, 18, 22, 26)] + [((rnum >> 30) | (rnum << 2)) & 0xF]
    s = [v * v for v in s]
    if seed & 1:
        sh1, sh2 = (4 if seed & 2 else 5), (6 if count == 3 else 5)
    else:
        sh1, sh2 = (6 if count == 3 else 5), (4 if seed & 2 else 5)
    sh3 = sh1 if seed & 0x10 else sh2
    s = [v >> (sh3 if i >= 8 else (sh1 if i % 2 == 0 else sh2)) for i, v in enumerate(s)]
    a = (s[0] * x + s[1] * y + s[10] * z + (rnum >> 14)) & 0x3F
    b = (s[2] * x + s[3] * y + s[11] * z + (rnum >> 10)) & 0x3F
    c = (s[4] * x + s[5] * y + s[8] * z + (rnum >> 6)) & 0x3F if count >= 3 else 0
    d = (s[6] * x + s[7] * y + s[9] * z + (rnum >> 2)) & 0x3F if count >= 4 else 0
    if a >= b and a >= c and a >= d:
        return 0
    if b >= c and b >= d:
        return 1
    return 2 if c >= d else 3


def _dims(block):
    """(bx, by, bz, image shape without the channel axis) of a footprint."""
    bx, by = block[0], block[1]
    bz = block[2] if len(block) > 2 else 1
    if bz > 1:
        return bx, by, bz, (bz * BLOCKS_3D, by * BLOCKS_3D, bx * BLOCKS_3D)
    return bx, by, 1, (by * BLOCKS, bx * BLOCKS)


_CUTS = {}


def _cuts(block, colours):
    """The format's own `colours`-partition patterns of the footprint in which every region has a fair share of the texels."""
    key = (tuple(block), colours)
    if key not in _CUTS:
        bx, by, bz, _ = _dims(block)
        texels = bx * by * bz
        floor = min(5, texels // (2 * colours))
        found = []
        for seed in range(1024):
            cut = np.array([[[partition_of_texel(seed, x, y, z, colours, texels < 31) for x in range(bx)] for y in range(by)] for z in range(bz)])
            if min(int((cut == k).sum()) for k in range(colours)) >= floor:
                found.append(cut)
            if len(found) == 48:
                break
        _CUTS[key] = found
    return _CUTS[key]


def _which(block, colours, rng):
    """Region index of every texel: each block cut along one of its footprint's own partition patterns."""
    bx, by, bz, shape = _dims(block)
    cuts = _cuts(block, colours)
    full = (shape if bz > 1 else (1,) + shape)
    which = np.empty(full, dtype=np.int64)
    for k in range(full[0] // bz):
        for j in range(full[1] // by):
            for i in range(full[2] // bx):
                which[k * bz:(k + 1) * bz, j * by:(j + 1) * by, i * bx:(i + 1) * bx] = cuts[int(rng.integers(0, len(cuts)))]
    return which if bz > 1 else which[0]


def patches(block, colours, seed):
    """tests/straight_stages_cases.patches for any footprint: every block cut into `colours` regions along one of the format's
    own partition patterns; a region has a colour of its own and varies along a channel of its own (four regions: opaque hues
    that vary in brightness, which is what the RGB-scale endpoint format stores in four integers)."""
    rng = np.random.default_rng(seed)
    which = _which(block, colours, rng)
    if colours == 4:
        img = (HUES[which] * rng.integers(40, 101, size=which.shape + (1,))) // 100
        img[..., 3] = 255
        return img.astype(np.uint8)
    img = PALETTE[which] + rng.integers(-3, 4, size=which.shape + (4,))
    swing = rng.integers(-50, 51, size=which.shape)
    for k in range(colours):
        img[..., k] += np.where(which == k, swing, 0)
    return np.clip(img, 0, 255).astype(np.uint8)


def _block_scale(block, shape, rng, choices):
    """One of `choices` per block, as an array of the image's shape (2D)."""
    by, bx = block[1], block[0]
    per = rng.choice(np.asarray(choices, dtype=np.float64), size=(shape[0] // by, shape[1] // bx))
    return np.repeat(np.repeat(per, by, axis=0), bx, axis=1)


def hdr_patches(block, colours, seed):
    """The four-colour patches as RGBA16F: opaque hues that vary in brightness, each block scaled by one of 0.25, 1, 4, 16."""
    rng = np.random.default_rng(seed)
    which = _which(block, colours, rng)
    img = (HUES[which] / 255.0) * (rng.integers(40, 101, size=which.shape + (1,)) / 100.0)
    img[..., :3] *= _block_scale(block, which.shape, rng, (0.25, 1.0, 4.0, 16.0))[..., None]
    img[..., 3] = 1.0
    return img.astype(np.float16)


GRAY_AND_HUES = np.array([[255, 255, 255, 255], [40, 80, 255, 255], [150, 150, 150, 255], [250, 60, 50, 255]], dtype=np.int64)


def mixed_patches(block, colours, seed, hdr=False):
    """As the four-colour patches, with gray regions next to hued ones, all varying in brightness: a luminance format
    (two integers) next to an RGB-scale one (four), which are of different classes."""
    rng = np.random.default_rng(seed)
    which = _which(block, colours, rng)
    img = (GRAY_AND_HUES[which] * rng.integers(40, 101, size=which.shape + (1,))) // 100
    img[..., 3] = 255
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, which.shape, rng, (0.25, 1.0, 4.0, 16.0))[..., None]
    return out.astype(np.float16)


def alpha_regions(block, colours, seed, hdr=False):
    """`colours` regions per block that differ in what their alpha does -- region 0 opaque, the others with an alpha that
    varies with their colour -- so that the partitions want endpoint formats of different classes (RGB next to RGBA)."""
    rng = np.random.default_rng(seed)
    which = _which(block, colours, rng)
    img = PALETTE[which] + rng.integers(-3, 4, size=which.shape + (4,))
    swing = rng.integers(-50, 51, size=which.shape)
    for k in range(colours):
        img[..., k % 3] += np.where(which == k, swing, 0)
    img[..., 3] = np.where(which == 0, 255, 128 + 2 * swing)
    img = np.clip(img, 0, 255)
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, which.shape, rng, (0.5, 2.0, 8.0))[..., None]
    return out.astype(np.float16)


def gray_regions(block, colours, seed):
    """Gray regions, region 0 opaque and the others with a varying alpha: luminance next to luminance+alpha formats."""
    rng = np.random.default_rng(seed)
    which = _which(block, colours, rng)
    level = np.array([60, 200, 120, 240])[which] + rng.integers(-40, 41, size=which.shape)
    img = np.stack([level, level, level, np.where(which == 0, 255, 100 + rng.integers(-60, 61, size=which.shape))], axis=-1)
    return np.clip(img, 0, 255).astype(np.uint8)


def noise(block, seed, channels="rgba", hdr=False):
    """White noise in the named channels: "rgba", "rgb" (alpha constant), "la" (gray and alpha), "l" (gray, opaque)."""
    rng = np.random.default_rng(seed)
    shape = _dims(block)[3]
    img = rng.integers(0, 256, size=shape + (4,))
    if channels in ("la", "l"):
        img[..., 1] = img[..., 0]
        img[..., 2] = img[..., 0]
    if channels in ("rgb", "l"):
        img[..., 3] = 255
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, shape, rng, (0.25, 1.0, 4.0, 16.0))[..., None]
    return out.astype(np.float16)


def lone_channel(block, component, seed, hdr=False):
    """A smooth field shared by all channels but `component`, which holds a field of its own: the two-plane search puts its
    second plane on that component."""
    rng = np.random.default_rng(seed)
    bx, by, bz, shape = _dims(block)
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    phase = rng.uniform(0, 6.28, size=6)
    shared = sum(np.sin(g * (2.2 / b) + p) for g, b, p in zip(grid, (bz, by, bx)[-len(grid):], phase))
    own = sum(np.cos(g * (3.1 / b) + p) for g, b, p in zip(grid[::-1], (bx, by, bz), phase[3:]))
    shared = 128 + 90 * shared / len(grid) + rng.integers(-4, 5, size=shape)
    own = 128 + 100 * own / len(grid) + rng.integers(-4, 5, size=shape)
    scale = np.array([1.0, 0.8, 0.6, 0.9])
    img = shared[..., None] * scale
    img[..., component] = own
    img = np.clip(img, 0, 255)
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, shape, rng, (0.5, 2.0, 8.0))[..., None]
    return out.astype(np.float16)


def smooth(block, seed, hdr=False):
    """Ramps of several steepnesses with a little noise, opaque in the upper half: coarse colour and fine weight grids."""
    rng = np.random.default_rng(seed)
    shape = _dims(block)[3]
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    x, y = grid[-1], grid[-2]
    z = grid[0] if len(grid) == 3 else 0
    w, h = shape[-1], shape[-2]
    img = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x + y + z) * 7) % 256, 255 - (x * 3 + y * 2 + z * 5) % 256], axis=-1)
    img = img + rng.integers(-2, 3, size=img.shape)
    img[: shape[0] // 2, ..., 3] = 255
    img = np.clip(img, 0, 255)
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, shape, rng, (0.25, 1.0, 4.0, 16.0))[..., None]
    return out.astype(np.float16)


def flat(block, seed, hdr=False):
    """The product's synthetic image with a constant patch of 5x5 blocks (void-extent blocks; FP16 ones in an HDR profile) and
    an opaque quarter."""
    bx, by, bz, shape = _dims(block)
    rng = np.random.default_rng(seed)
    if bz > 1:
        img = rng.integers(0, 256, size=shape + (4,), dtype=np.uint8)
        img[: 2 * bz, : 3 * by, : 3 * bx] = (90, 14, 200, 255)
        return img
    h, w = shape
    if hdr:
        img = A.synthetic_hdr_image(w, h, seed).copy()
        img[: 5 * by, : 5 * bx] = np.array([0.75, 2.5, 11.0, 1.0], dtype=np.float16)
        return img
    img = A.synthetic_image(w, h, seed).copy()
    img[: 5 * by, : 5 * bx] = (17, 99, 201, 255)
    img[5 * by:, : 5 * bx, 3] = 255
    return img


def synthetic(block, seed, hdr=False, variant=None):
    """The product's own synthetic image (what the parity tests and the sweep tools use), and for HDR the variants of
    tests/images.hdr_variants."""
    bx, by, bz, shape = _dims(block)
    if bz > 1:
        return np.ascontiguousarray(A.synthetic_image(shape[2], shape[0] * shape[1], seed).reshape(shape + (4,)))
    h, w = shape
    if not hdr:
        return A.synthetic_image(w, h, seed)
    img = A.synthetic_hdr_image(w, h, seed).astype(np.float32)
    if variant == "opaque":
        img[..., 3] = 1.0
    elif variant == "gray":
        img[..., 1] = img[..., 0]
        img[..., 2] = img[..., 0]
        img[..., 3] = 1.0
    elif variant == "dim":
        img[..., :3] *= 0.02
    elif variant == "bright":
        img[..., :3] *= 400.0
    return img.astype(np.float16)


def ramps(block, seed, channels="l", hdr=False):
    """Every block a smooth, bent ramp between two levels of its own, the same shape in every channel: few weights on a
    coarse grid that want many levels.  channels: "l" gray, "rgb" coloured, "rgba" with an alpha that follows."""
    rng = np.random.default_rng(seed)
    bx, by, bz, shape = _dims(block)
    full = shape if bz > 1 else (1,) + shape
    img = np.empty(full + (4,), dtype=np.float64)
    z, y, x = np.meshgrid(np.arange(bz) / max(bz - 1, 1), np.arange(by) / (by - 1), np.arange(bx) / (bx - 1), indexing="ij")
    for k in range(full[0] // bz):
        for j in range(full[1] // by):
            for i in range(full[2] // bx):
                d = rng.uniform(-1, 1, size=3)
                t = d[0] * x + d[1] * y + d[2] * z
                t = (t - t.min()) / max(t.max() - t.min(), 1e-9)
                t = t ** rng.uniform(0.5, 2.0)
                lo, hi = rng.integers(0, 256, size=4), rng.integers(0, 256, size=4)
                if channels == "l":
                    lo[1:3], hi[1:3] = lo[0], hi[0]
                if channels != "rgba":
                    lo[3] = hi[3] = 255
                img[k * bz:(k + 1) * bz, j * by:(j + 1) * by, i * bx:(i + 1) * bx] = lo + (hi - lo) * t[..., None]
    img = np.clip(np.rint(img), 0, 255)
    img = img if bz > 1 else img[0]
    if not hdr:
        return img.astype(np.uint8)
    out = img / 255.0
    out[..., :3] *= _block_scale(block, shape, rng, (0.25, 1.0, 4.0, 16.0))[..., None]
    return out.astype(np.float16)


def pastel(block, seed):
    """Near-gray blocks: a gray level per block, a faint tint and a short ramp to a neighbouring colour, with an alpha ramp in
    the lower half -- endpoints close together and close to gray, where the delta formats with blue contraction pay."""
    rng = np.random.default_rng(seed)
    bx, by, bz, shape = _dims(block)
    full = shape if bz > 1 else (1,) + shape
    img = np.empty(full + (4,), dtype=np.float64)
    z, y, x = np.meshgrid(np.arange(bz) / max(bz - 1, 1), np.arange(by) / (by - 1), np.arange(bx) / (bx - 1), indexing="ij")
    for k in range(full[0] // bz):
        for j in range(full[1] // by):
            for i in range(full[2] // bx):
                d = rng.uniform(-1, 1, size=3)
                t = d[0] * x + d[1] * y + d[2] * z
                t = (t - t.min()) / max(t.max() - t.min(), 1e-9)
                lo = rng.integers(40, 216) + rng.integers(-12, 13, size=4)
                hi = lo + rng.integers(-24, 25, size=4)
                if 2 * j < full[1] // by:
                    lo[3] = hi[3] = 255
                img[k * bz:(k + 1) * bz, j * by:(j + 1) * by, i * bx:(i + 1) * bx] = lo + (hi - lo) * t[..., None]
    img = np.clip(np.rint(img + rng.integers(-1, 2, size=img.shape)), 0, 255)
    return (img if bz > 1 else img[0]).astype(np.uint8)


def grain(block, seed):
    """Opaque near-gray blocks, every texel at a random place between two close colours of its block: a full weight grid
    leaves few bits for the endpoints, where the RGB delta format with blue contraction pays."""
    rng = np.random.default_rng(seed)
    bx, by, bz, shape = _dims(block)
    full = shape if bz > 1 else (1,) + shape
    img = np.empty(full + (4,), dtype=np.float64)
    for k in range(full[0] // bz):
        for j in range(full[1] // by):
            for i in range(full[2] // bx):
                t = rng.uniform(0, 1, size=(bz, by, bx, 1))
                lo = rng.integers(40, 216) + rng.integers(-12, 13, size=4)
                hi = lo + rng.integers(-24, 25, size=4)
                img[k * bz:(k + 1) * bz, j * by:(j + 1) * by, i * bx:(i + 1) * bx] = lo + (hi - lo) * t
    img[..., 3] = 255
    img = np.clip(np.rint(img), 0, 255)
    return (img if bz > 1 else img[0]).astype(np.uint8)


def synthetic_opaque(block, seed):
    """The synthetic image without its alpha: RGB blocks of every smoothness, where the RGB delta format is common."""
    img = synthetic(block, seed).copy()
    img[..., 3] = 255
    return img


def two_colour(block, seed):
    """tests/images.two_colour at the footprint's size: hard two-region blocks with different alpha."""
    rng = np.random.default_rng(seed)
    shape = _dims(block)[3]
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    mask = ((grid[-1] * 3 + grid[-2] * 5 + (grid[0] * 2 if len(grid) == 3 else 0)) // 7) % 2
    a = np.array([220, 40, 30, 255])
    b = np.array([20, 60, 230, 128])
    img = np.where(mask[..., None] == 1, a, b) + rng.integers(-6, 7, size=shape + (4,))
    return np.clip(img, 0, 255).astype(np.uint8)


def gray(block, seed):
    """tests/images.grayscale at the footprint's size: luminance blocks, opaque in the upper half."""
    img = synthetic(block, seed).copy()
    img[..., 1] = img[..., 0]
    img[..., 2] = img[..., 0]
    img[: img.shape[0] // 2, ..., 3] = 255
    return img


# name -> generator(block); LDR rows take IMAGES_LDR, HDR rows IMAGES_HDR (all RGBA16F), volumes IMAGES_3D
IMAGES_LDR = collections.OrderedDict([
    ("two_patches", lambda b: patches(b, 2, 31)),
    ("three_patches", lambda b: patches(b, 3, 32)),
    ("four_patches", lambda b: patches(b, 4, 33)),
    ("alpha_regions2", lambda b: alpha_regions(b, 2, 34)),
    ("alpha_regions3", lambda b: alpha_regions(b, 3, 35)),
    ("gray_regions2", lambda b: gray_regions(b, 2, 36)),
    ("rgba_noise", lambda b: noise(b, 37, "rgba")),
    ("rgb_noise", lambda b: noise(b, 38, "rgb")),
    ("la_noise", lambda b: noise(b, 39, "la")),
    ("l_noise", lambda b: noise(b, 40, "l")),
    ("lone_r", lambda b: lone_channel(b, 0, 41)),
    ("lone_g", lambda b: lone_channel(b, 1, 42)),
    ("lone_b", lambda b: lone_channel(b, 2, 43)),
    ("lone_a", lambda b: lone_channel(b, 3, 44)),
    ("smooth", lambda b: smooth(b, 45)),
    ("flat", lambda b: flat(b, 46)),
    ("synthetic", lambda b: synthetic(b, 47)),
    ("two_colour", lambda b: two_colour(b, 48)),
    ("gray", lambda b: gray(b, 49)),
    ("gray_ramps", lambda b: ramps(b, 81, "l")),
    ("rgb_ramps", lambda b: ramps(b, 82, "rgb")),
    ("rgba_ramps", lambda b: ramps(b, 83, "rgba")),
    ("pastel", lambda b: pastel(b, 84)),
    ("pastel2", lambda b: pastel(b, 85)),
    ("synthetic2", lambda b: synthetic(b, 86)),
    ("synthetic_opaque", lambda b: synthetic_opaque(b, 87)),
    ("synthetic_opaque2", lambda b: synthetic_opaque(b, 88)),
    ("grain", lambda b: grain(b, 89)),
    ("mixed_patches4", lambda b: mixed_patches(b, 4, 90)),
])
IMAGES_HDR = collections.OrderedDict([
    ("hdr_two_patches", lambda b: hdr_patches(b, 2, 51)),
    ("hdr_three_patches", lambda b: hdr_patches(b, 3, 52)),
    ("hdr_four_patches", lambda b: hdr_patches(b, 4, 53)),
    ("hdr_alpha_regions2", lambda b: alpha_regions(b, 2, 54, hdr=True)),
    ("hdr_alpha_regions3", lambda b: alpha_regions(b, 3, 55, hdr=True)),
    ("hdr_rgba_noise", lambda b: noise(b, 56, "rgba", hdr=True)),
    ("hdr_l_noise", lambda b: noise(b, 57, "l", hdr=True)),
    ("hdr_lone_r", lambda b: lone_channel(b, 0, 58, hdr=True)),
    ("hdr_lone_g", lambda b: lone_channel(b, 1, 59, hdr=True)),
    ("hdr_lone_b", lambda b: lone_channel(b, 2, 60, hdr=True)),
    ("hdr_lone_a", lambda b: lone_channel(b, 3, 61, hdr=True)),
    ("hdr_smooth", lambda b: smooth(b, 62, hdr=True)),
    ("hdr_flat", lambda b: flat(b, 63, hdr=True)),
    ("hdr_synthetic", lambda b: synthetic(b, 64, hdr=True)),
    ("hdr_opaque", lambda b: synthetic(b, 65, hdr=True, variant="opaque")),
    ("hdr_gray", lambda b: synthetic(b, 66, hdr=True, variant="gray")),
    ("hdr_dim", lambda b: synthetic(b, 67, hdr=True, variant="dim")),
    ("hdr_bright", lambda b: synthetic(b, 68, hdr=True, variant="bright")),
    ("hdr_gray_ramps", lambda b: ramps(b, 91, "l", hdr=True)),
    ("hdr_rgb_ramps", lambda b: ramps(b, 92, "rgb", hdr=True)),
    ("hdr_mixed_patches3", lambda b: mixed_patches(b, 3, 93, hdr=True)),
    ("hdr_mixed_patches4", lambda b: mixed_patches(b, 4, 94, hdr=True)),
])
IMAGES_3D = collections.OrderedDict((k, IMAGES_LDR[k]) for k in (
    "two_patches", "three_patches", "four_patches", "alpha_regions2", "gray_regions2", "rgba_noise", "rgb_noise", "la_noise",
    "l_noise", "lone_r", "lone_g", "lone_b", "lone_a", "smooth", "flat", "two_colour", "gray_ramps", "rgb_ramps", "rgba_ramps", "pastel", "pastel2", "synthetic_opaque", "synthetic_opaque2", "grain", "mixed_patches4"))


class Case:
    """One image in one row's context."""

    def __init__(self, row, name, make):
        self.row, self.name, self.make = row, name, make
        self.profile, self.block, self.quality, self.kernel, self.build_class = ROWS[row]
        self.id = "%s-%s" % (row, name)
        self._image = None

    def image(self):
        if self._image is None:
            img = np.ascontiguousarray(self.make(self.block))
            bx, by, bz, _ = _dims(self.block)
            blocks = (img.shape[-2] // bx) * (img.shape[-3] // by) * ((img.shape[0] // bz) if bz > 1 else 1)
            assert blocks <= 100, (self.id, blocks)
            img.setflags(write=False)
            self._image = img
        return self._image


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = []
        for row, (profile, block, _, _, _) in ROWS.items():
            hdr = profile in (A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)
            images = IMAGES_3D if len(block) > 2 else (IMAGES_HDR if hdr else IMAGES_LDR)
            _CASES += [Case(row, name, make) for name, make in images.items()]
    return _CASES


def case_ids():
    return [c.id for c in cases()]


class Reference:
    """The reference's bytes of every case, compressed once per session and never changed."""

    def __init__(self, ref):
        self.ref = ref
        self.by_id = {c.id: c for c in cases()}
        self.bytes = {}

    def want(self, case_id):
        if case_id not in self.bytes:
            c = self.by_id[case_id]
            out = self.ref.compress(c.image(), c.block, c.quality, profile=c.profile)
            out.setflags(write=False)
            self.bytes[case_id] = out
        return self.bytes[case_id]


# ---- float edge values through the block load (load_block, half_to_float, float_to_lns in csrc/wave_*.h) ---------------------

FLOAT_EDGE_QUALITY = A.PRE_MEDIUM
FLOAT_EDGE_VALUES = [np.nan, np.inf, -np.inf, -0.0, 1e-40, 1e-8, 6e-8, 2.0 ** -15, 2.0 ** -14, 0.99999994, 1.0000001, 65504.0]
FLOAT_EDGE_VALUES_F32 = [1e5]


def float_edge_image(dtype):
    """24x24 RGBA of `dtype` (np.float16 / np.float32): values drawn from -0.25 to 1.25, sixty seeded positions overwritten
    with non-finite values, signed zero, denormals, the neighbours of 1 and the largest half (for F32 also 1e5)."""
    rng = np.random.default_rng(71)
    img = rng.uniform(-0.25, 1.25, size=(24, 24, 4)).astype(np.float32)
    values = FLOAT_EDGE_VALUES + (FLOAT_EDGE_VALUES_F32 if dtype == np.float32 else [])
    flat = img.reshape(-1)
    where = rng.choice(flat.size, size=60, replace=False)
    with np.errstate(over="ignore", under="ignore"):
        flat[where] = np.asarray([values[i % len(values)] for i in range(60)], dtype=np.float32)
        return np.ascontiguousarray(img.astype(dtype))


def float_edge_cases():
    """(dtype, profile, block, swizzle): F16 and F32 x the four profiles x 4x4, 6x6, 10x8 x identity and (B, G, R, 1)."""
    return [(dtype, profile, block, swizzle)
            for dtype in (np.float16, np.float32)
            for profile in (A.PRF_LDR, A.PRF_LDR_SRGB, A.PRF_HDR_RGB_LDR_A, A.PRF_HDR)
            for block in ((4, 4), (6, 6), (10, 8))
            for swizzle in (A.SWZ_RGBA, (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_1))]


def float_edge_id(case):
    dtype, profile, block, swizzle = case
    return "%s-%s-%dx%d-%s" % ("f16" if dtype == np.float16 else "f32", ("srgb", "ldr", "hdr_ldr_a", "hdr")[profile], block[0], block[1],
                               "rgba" if swizzle == A.SWZ_RGBA else "bgr1")
