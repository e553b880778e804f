# SPDX-License-Identifier: Apache-2.0
"""What the loader stage of the compressor (csrc/wave_load.h, load_block) is fed by tests/test_input_coverage_cpu.py,
tests/test_input_coverage.py and part (b) of tests/test_jit_matrix.py: texels of every data type that lie outside the range of
the format -- negative, above one, above the largest half, NaN, infinities, -0.0, subnormals -- through every swizzle kind, under
every profile, on every build of the kernel.  A plain module: no fixtures, seeded content, arrays handed out read-only.

The contract (ref: load_image_block, Source/astcenc_image.cpp:162-275; float_to_lns, Source/astcenc_vecmathlib.h) is the
reference's bytes.  `sanitised` states it in numpy: the compressor sees a NaN as zero and every other value clipped to [0, 1]
(an LDR profile) or to [0, 65536] (an HDR profile), and a half as the float of the same value.

Content classes (`image`, `volume`), each as F16 and as F32 over images.noisy / 255 of 41 x 38 texels (no multiple of any
footprint; 4 x 4 blocks of 12 x 12), with up to four constant REGION x REGION squares in the top left corner:
  range      base * 3 - 1: -1 .. 2
  nonfinite  NaN, +Inf, -Inf, 7.5, -3.0 on 3 % of the components each; squares of NaN, of +Inf, of -0.0 and of
             (2, 3, +Inf, 1) -- the last one constant under an LDR profile only once it is clamped
  tiny       a subnormal on 30 % of the components (1e-40; as a half 2^-24); a square of G = B = 0, A = 1 and R a varying
             subnormal: r * 65535 != 0, so the block is neither grayscale nor constant -- unless the device flushes r
  huge       base * 40 with 1e30, 65520, 70000 (as a half: 65504), subnormals, negatives, NaN and infinities scattered; a
             square of (70000, 1e9, +Inf, 1) -- the void-extent block of colour 0x7BFF under HDR -- and one of NaN
  u8         images.noisy itself, for the HDR profiles and the constant swizzles"""
import collections
import functools

import numpy as np

import images

import astcenc_amd as A  # (path set up by conftest.py)

W, H, REGION = 41, 38, 12
VOL_D, VOL_W, VOL_H, VOL_REGION = 7, 23, 19, 8
SEED = 0x51ED

FLOAT_CLASSES = ["range", "nonfinite", "tiny", "huge"]
CLASSES = FLOAT_CLASSES + ["u8"]
DTYPES = {"f16": np.float16, "f32": np.float32, "u8": np.uint8}
SWIZZLES = collections.OrderedDict([
    ("rgba", A.SWZ_RGBA),
    ("ba01", (A.SWZ_B, A.SWZ_A, A.SWZ_0, A.SWZ_1)),
    ("aaar", (A.SWZ_A, A.SWZ_A, A.SWZ_A, A.SWZ_R)),
])
PROFILES = collections.OrderedDict([("srgb", A.PRF_LDR_SRGB), ("ldr", A.PRF_LDR), ("hdr_ldr_a", A.PRF_HDR_RGB_LDR_A), ("hdr", A.PRF_HDR)])
HDR_PROFILES = (A.PRF_HDR_RGB_LDR_A, A.PRF_HDR)

NAN, INF = float("nan"), float("inf")
HALF_MAX, HALF_TINY = 65504.0, 2.0 ** -24


def _subnormal(dtype):
    return 1e-40 if dtype == np.float32 else HALF_TINY


def _regions(img, r):
    """The four r x r squares of the top left corner, as views."""
    return [img[y:y + r, x:x + r] for y, x in ((0, 0), (0, r), (r, 0), (r, r))]


def _scatter(img, u, values, share):
    for i, v in enumerate(values):
        img[(u >= i * share) & (u < (i + 1) * share)] = v


def _build(cls, dtype, w, h, seed, r):
    base = images.noisy(w, h, seed).astype(np.float64) / 255.0
    if cls == "base":
        return base.astype(np.float32)
    u = np.random.default_rng([seed, CLASSES.index(cls)]).random((h, w, 4))
    sub, big = _subnormal(dtype), (1e30 if dtype == np.float32 else HALF_MAX)
    if cls == "range":
        img = base * 3.0 - 1.0
    elif cls == "nonfinite":
        img = base.copy()
        _scatter(img, u, [NAN, INF, -INF, 7.5, -3.0], 0.03)
        nan, inf, negzero, clamped = _regions(img, r)
        nan[...] = NAN
        inf[...] = INF
        negzero[...] = -0.0
        clamped[...] = (2.0, 3.0, INF, 1.0)
    elif cls == "tiny":
        img = base.copy()
        img[u < 0.3] = sub
        y, x = np.meshgrid(np.arange(r), np.arange(r), indexing="ij")
        region = _regions(img, r)[0]
        region[...] = (0.0, 0.0, 0.0, 1.0)
        region[..., 0] = sub * (1 + (x + y) % 7)
    elif cls == "huge":
        img = base * 40.0
        over = [65520.0, 70000.0] if dtype == np.float32 else [HALF_MAX, HALF_MAX]
        _scatter(img, u, [big] + over + [sub, -5.0, -big, NAN, INF, -INF], 0.02)
        bright, nan = _regions(img, r)[:2]
        bright[...] = (70000.0, 1e9, INF, 1.0) if dtype == np.float32 else (HALF_MAX, INF, INF, 1.0)
        nan[...] = NAN
    else:
        raise KeyError(cls)
    with np.errstate(over="raise"):                 # (every value is chosen to be one the type holds)
        return img.astype(dtype)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def image(cls, dtype="f32", w=W, h=H, seed=SEED):
    """[h, w, 4] of class `cls` ("base": the unspoilt F32 image every float class starts from), read-only."""
    if cls == "u8":
        return _frozen(images.noisy(w, h, seed))
    return _frozen(_build(cls, DTYPES[dtype], w, h, seed, REGION))


@functools.lru_cache(maxsize=None)
def volume(cls, dtype="f32"):
    """[7, 19, 23, 4]: seven slices of the class, the constant squares (8 x 8 here) at the same place in each."""
    if cls == "u8":
        return _frozen(np.stack([images.noisy(VOL_W, VOL_H, SEED + z) for z in range(VOL_D)]))
    return _frozen(np.stack([_build(cls, DTYPES[dtype], VOL_W, VOL_H, SEED + z, VOL_REGION) for z in range(VOL_D)]))


def widened(img):
    """(P1) the F32 image of the same values as an F16 one."""
    assert img.dtype == np.float16
    return _frozen(img.astype(np.float32))


def sanitised(img, profile):
    """(P2) the numpy statement of the contract, always F32: what the compressor makes of a float image under `profile`."""
    assert img.dtype in (np.float16, np.float32)
    out = img.astype(np.float32)
    out[np.isnan(out)] = 0.0
    return _frozen(np.clip(out, np.float32(0.0), np.float32(65536.0 if profile in HDR_PROFILES else 1.0)))


# ---- the case table ---------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "cls dtype swizzle")          # swizzle: a key of SWIZZLES
K = "astc_compress_blocks_"
M, F, T = A.PRE_MEDIUM, A.PRE_FAST, A.PRE_THOROUGH
# build of the kernel: the contexts (profile, block, quality) that load every class through it
CONTEXTS = collections.OrderedDict([
    ("ldr_6x6m", [(A.PRF_LDR, (6, 6), M)]),
    ("ldr_8x8t", [(A.PRF_LDR, (8, 8), T)]),
    ("hdr_6x6m", [(A.PRF_HDR, (6, 6), M)]),
    ("ldr64", [(A.PRF_LDR, (4, 4), F), (A.PRF_LDR, (5, 4), M), (A.PRF_LDR_SRGB, (6, 6), M)]),
    ("ldr", [(A.PRF_LDR, (10, 8), M), (A.PRF_LDR, (12, 12), M)]),
    ("hdr64", [(A.PRF_HDR, (8, 8), M), (A.PRF_HDR_RGB_LDR_A, (6, 6), M), (A.PRF_HDR, (4, 4), F)]),
    ("hdr", [(A.PRF_HDR, (10, 10), M), (A.PRF_HDR_RGB_LDR_A, (12, 10), M)]),
    ("3d", [(A.PRF_LDR, (4, 4, 4), M), (A.PRF_HDR, (5, 5, 5), M), (A.PRF_LDR, (3, 3, 3), M)]),
])
BUILDS = list(CONTEXTS)


def kernel_of(build, ctx):
    """The kernel the library launches for context `ctx` of row `build` with run-time builds off (csrc/backend_hip.hip): a
    volume runs the generic build of its profile and texel count."""
    if build != "3d":
        return K + build
    profile, block = ctx[0], ctx[1]
    return K + ("hdr" if profile in HDR_PROFILES else "ldr") + ("64" if block[0] * block[1] * block[2] <= 64 else "")


def cases():
    """The 20 cases every context runs: every class in every type it comes in; `nonfinite` through the three swizzles, the rest
    through the identity and the one with constants."""
    out = []
    for cls in CLASSES:
        for dtype in (("u8",) if cls == "u8" else ("f16", "f32")):
            for swz in list(SWIZZLES)[:3 if cls == "nonfinite" else 2]:
                out.append(Case(cls, dtype, swz))
    return out


def content(case, block):
    """The array of a case for a footprint: the image, or the volume for a 3D footprint."""
    return volume(case.cls, case.dtype) if len(block) == 3 else image(case.cls, case.dtype)


def ctx_id(ctx):
    names = {v: k for k, v in PROFILES.items()}
    return "%s-%s-q%g" % (names[ctx[0]], "x".join(map(str, ctx[1])), ctx[2])


def case_id(case):
    return "%s-%s-%s" % case


def compress(lib, ctx, img, swizzle="rgba", flags=0, tweak=None):
    profile, block, quality = ctx
    return lib.compress(img, block, quality, profile=profile, flags=flags, swizzle=SWIZZLES[swizzle], tweak=tweak).reshape(-1, 16)


def differing(a, b):
    a, b = a.reshape(-1, 16), b.reshape(-1, 16)
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((a != b).any(axis=1).sum())


def void_extent_colours(blocks):
    """The colour fields (8 bytes, as a hex string) of the void-extent blocks of a stream (block mode bits 0x1FC)."""
    b = blocks.reshape(-1, 16)
    void = (b[:, 0] == 0xFC) & ((b[:, 1] & 1) == 1)
    return [bytes(row[8:]).hex() for row in b[void]]


class Outputs:
    """One library's bytes per (context, case), compressed once and never changed."""

    def __init__(self, lib):
        self.lib, self.bytes = lib, {}

    def of(self, ctx, case):
        key = (ctx, case)
        if key not in self.bytes:
            out = compress(self.lib, ctx, content(case, ctx[1]), case.swizzle)
            out.setflags(write=False)
            self.bytes[key] = out
        return self.bytes[key]
