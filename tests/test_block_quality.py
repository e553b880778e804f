# SPDX-License-Identifier: Apache-2.0
"""Compressed blocks scored against the source image in one device pass (astcenc_amd_compare_blocks_device, its _hdr_ form and
astcenc_amd_compare_image_set_device; csrc/kernel_quality.hip, csrc/wave_quality.h).

The yardstick is always the two existing calls on the same stream: astcenc_amd_decompress_image_device into a scratch tensor,
then astcenc_amd_compare_images(_hdr)_device with the original as image 1.  Totals agree within REL = 1e-12 relative (two
summation orders of non-negative terms, neither side chaining more than about a hundred additions before its tree); rgb_peak
and texels are equal.  Per-block sums are checked against a numpy model over the two-call path's decoded image -- float32
terms as in reference_sums of tests/test_metrics.py, float64 sums -- within 1e-12 relative (a block has at most 216
non-negative terms: any order is within 216 * 2^-53 = 2.4e-14 of exact), and a channel's per-block values add up to its total
within the same tolerance.

Streams: what the library compresses from the noisy, flat and two-colour images of tests/images.py at -thorough
(multi-partition and dual-plane blocks, constant blocks), and random bit patterns (error blocks, FP16 constants, HDR endpoint
formats).  Shapes: the smallest that reach a distinct path of the texel phases and of the reduction (SHAPES below).

What each group is there for, and the one-line mistakes it would catch:
  * test_shapes_ldr / test_shapes_other_profiles: every shape, type pair, profile and swizzle against the yardstick.
      - a per-block fold that takes the first trip only, or loses a block that straddles two trips: 134x10 at 4x4 (a 128-column
        run in two trips), 390x13 at 12x12 (six trips, blocks 5 | 6 split by a trip), 100x4x4 at 3x3x3;
      - a run partial indexed by block instead of by run: every shape with more than one block per run;
      - the F16 operand compared before it is rounded to half; the U8 operand taken from floats: the HDR-context cases (the
        host harness of tests/test_block_quality_cpu.py checks the terms bit for bit);
      - the swizzle applied to the original, or not applied: bgra, rrr1, gggr and the z reconstruction;
      - rgb_peak or the alpha scale taken from the decoded image: every case (the original is image 1).
  * test_memory_discipline: guard bytes on both sides of the per-block records, originals and streams bit-unchanged,
    sub-views 4, 8 and 12 bytes past a 16-byte boundary.
  * test_image_set: a chain, a 134x10 entry and a 3-slice entry in one call: every entry's sums and block records bit equal to
    the single-image call (an entry's first run taken from the wrong table slot, partials of neighbouring entries mixed);
    bad entries and a short per-block buffer rejected without a write.
  * test_launch_logic: a one-block call after the 390x13 call on one context (stale partials: a finish pass that adds slots
    past the entry's runs); two runs give the same doubles (atomics, an order that depends on scheduling); a side stream with
    a pending producer (work queued on the wrong stream).
  * test_many_runs: 2100 x 40 at 4x4 is 170 runs: a finish pass that stops at 64 runs, or whose second trip per lane is lost.
  * test_split_launches: ASTCENC_AMD_DECODE_GRID_LIMIT=2 in a fresh process: pieces of two runs, an entry's later pieces added
    on top of its earlier ones, launches that hold the tail of one entry and the head of the next."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import images
from test_metrics import Guarded, load_texels

pytestmark = pytest.mark.gpu
REL = 1e-12

# (block, (w, h, d)): 6x6: one block; partial in x and y; exact; a second block of one column.  4x4 on 134x10: 34 blocks per
# row -- a second run of two blocks, a 128-column run in two lane trips, partial last blocks in x and y.  12x12 on 390x13: a
# 384-column run in six trips, a one-block run with 6 of 12 columns, a one-row second block row.  6x6 on 40x20x3: a 2D footprint
# over slices.  3D: the texel phase of 3D footprints, 34 blocks per row, partial in z.
SHAPES = [((6, 6), (1, 1, 1)), ((6, 6), (5, 7, 1)), ((6, 6), (6, 6, 1)), ((6, 6), (7, 6, 1)), ((4, 4), (134, 10, 1)), ((12, 12), (390, 13, 1)),
          ((6, 6), (40, 20, 3)), ((3, 3, 3), (100, 4, 4)), ((4, 4, 4), (9, 6, 5)), ((6, 6, 6), (7, 7, 7))]
SHAPE_IDS = ["%s-%s" % ("x".join(map(str, b)), "x".join(map(str, d))) for b, d in SHAPES]
SWIZZLES = {"rgba": "SWZ_R SWZ_G SWZ_B SWZ_A", "bgra": "SWZ_B SWZ_G SWZ_R SWZ_A", "rrr1": "SWZ_R SWZ_R SWZ_R SWZ_1", "gggr": "SWZ_G SWZ_G SWZ_G SWZ_R",
            "ra_z1": "SWZ_R SWZ_A SWZ_Z SWZ_1"}
NP_TYPES = {0: np.uint8, 1: np.float16, 2: np.float32}


def swizzle(A, name):
    return tuple(getattr(A, n) for n in SWIZZLES[name].split())


@pytest.fixture(scope="module")
def contexts(product, A):
    """Contexts by (block, profile), made on first use and freed with the module."""
    made = {}

    def get(block, profile=None):
        profile = A.PRF_LDR if profile is None else profile
        key = (tuple(block), profile)
        if key not in made:
            err, cfg = product.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, A.PRE_THOROUGH, 0)
            assert err == 0
            err, ctx = product.context_alloc(cfg, 1)
            assert err == 0, product.error_string(err)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


def block_count(block, dims):
    bz = block[2] if len(block) > 2 else 1
    return -(-dims[0] // block[0]) * -(-dims[1] // block[1]) * -(-dims[2] // bz)


def source_image(kind, dims, seed=5):
    """[D, H, W, 4] RGBA8."""
    w, h, d = dims
    make = {"noisy": lambda z: images.noisy(w, h, seed + z), "flat": lambda z: images.flat_regions(w, h), "two_colour": lambda z: images.two_colour(w, h, seed + z)}[kind]
    return np.stack([make(z) for z in range(d)])


def as_type(img8, t, specials=True):
    """The RGBA8 image in type t (floats: value / 255 * 3, with a NaN, a negative and an infinity when there is room)."""
    if t == 0:
        return img8
    x = (img8.astype(np.float32) / np.float32(255.0) * np.float32(3.0)).astype(NP_TYPES[t])
    flat = x.reshape(-1, 4)
    if specials and flat.shape[0] > 8:
        flat[1, 0] = np.nan; flat[3, 1] = -2.0; flat[5, 2] = np.inf
    return x


def random_stream(block, dims, seed):
    """test_decode_random_bit_patterns' generator: reserved modes, void extents (legal and not), FP16 constants."""
    rng = np.random.default_rng(seed)
    blocks = rng.integers(0, 256, size=(block_count(block, dims), 16), dtype=np.uint8)
    blocks[::7, 0] = 0xFC
    blocks[::7, 1] |= 0x01
    blocks[::14, 1] = 0xFD
    blocks[::14, 2:8] = 0xFF
    blocks[::28, 1] = 0xFF
    blocks[1::5, 1] &= 0xE7
    return blocks.reshape(-1)


def compressed_stream(product, A, kind, block, dims, profile=None):
    img = source_image(kind, dims)
    return product.compress(img if dims[2] > 1 or len(block) > 2 else img[0], block, A.PRE_THOROUGH, A.PRF_LDR if profile is None else profile)


def two_calls(product, A, ctx, t_blocks, t_image, dims, image_type, decode_type, swz, hdr=None, stream=None):
    """The yardstick: decode into a scratch tensor, compare with the original as image 1.  Returns (sums, hdr sums, decoded)."""
    import torch
    w, h, d = dims
    scratch = torch.zeros(w * h * d * 4 * np.dtype(NP_TYPES[decode_type]).itemsize, dtype=torch.uint8, device="cuda")
    s = A.Swizzle(*swz)
    err = product.lib.astcenc_amd_decompress_image_device(ctx, t_blocks.data_ptr(), t_blocks.numel(), scratch.data_ptr(), w, h, d, decode_type, C.byref(s), stream)
    assert err == 0, product.error_string(err)
    sums, hs = A.ErrorSums(), A.HdrErrorSums()
    if hdr is None:
        err = product.lib.astcenc_amd_compare_images_device(ctx, t_image.data_ptr(), image_type, scratch.data_ptr(), decode_type, w, h, d, stream, C.byref(sums))
    else:
        err = product.lib.astcenc_amd_compare_images_hdr_device(ctx, t_image.data_ptr(), image_type, scratch.data_ptr(), decode_type, w, h, d,
                                                                hdr[0], hdr[1], stream, C.byref(sums), C.byref(hs))
    assert err == 0, product.error_string(err)
    return sums, hs, scratch.cpu().numpy().view(NP_TYPES[decode_type]).reshape(d, h, w, 4)


def fused(product, A, ctx, t_blocks, t_image, dims, image_type, decode_type, swz, hdr=None, stream=None, per_block=None):
    """The call under test; per_block: None, or the number of blocks (records are returned as [blocks, 4])."""
    import torch
    w, h, d = dims
    s = A.Swizzle(*swz)
    errors = torch.full((per_block * 4,), -7.0, dtype=torch.float64, device="cuda") if per_block else None
    args = [ctx, t_blocks.data_ptr(), t_blocks.numel(), t_image.data_ptr(), w, h, d, image_type, decode_type, C.byref(s),
            errors.data_ptr() if per_block else None, per_block * 32 if per_block else 0]
    sums, hs = A.ErrorSums(), A.HdrErrorSums()
    if hdr is None:
        err = product.lib.astcenc_amd_compare_blocks_device(*args, stream, C.byref(sums))
    else:
        err = product.lib.astcenc_amd_compare_blocks_hdr_device(*args, hdr[0], hdr[1], stream, C.byref(sums), C.byref(hs))
    assert err == 0, product.error_string(err)
    return sums, hs, errors.cpu().numpy().reshape(-1, 4) if per_block else None


def block_model(original, decoded, block, dims):
    """[blocks, 4] squared-error sums per block: float32 terms (reference_sums of tests/test_metrics.py), float64 sums."""
    w, h, d = dims
    bz = block[2] if len(block) > 2 else 1
    diff = load_texels(original.reshape(d, h, w, 4)) - load_texels(decoded.reshape(d, h, w, 4))
    terms = (diff * diff).astype(np.float64)
    z, y, x = np.meshgrid(np.arange(d) // bz, np.arange(h) // block[1], np.arange(w) // block[0], indexing="ij")
    nbx, nby = -(-w // block[0]), -(-h // block[1])
    index = ((z * nby + y) * nbx + x).reshape(-1)
    n = block_count(block, dims)
    return np.stack([np.bincount(index, weights=terms[..., c].reshape(-1), minlength=n) for c in range(4)], axis=1)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "max relative difference", float(np.max(np.abs(got - want) / np.maximum(np.maximum(np.abs(got), np.abs(want)), 1e-300))))
    assert np.allclose(got, want, rtol=REL, atol=0), (what, got, want)


def check_case(product, A, ctx, block, dims, stream_bytes, original, decode_type, swz_name, hdr=None, what=""):
    import torch
    what = "%s %s %s original %s decode %d %s %s" % (block, dims, what, original.dtype, decode_type, swz_name, hdr)
    image_type = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[original.dtype]
    t_blocks, t_image = torch.from_numpy(stream_bytes).cuda(), torch.from_numpy(np.ascontiguousarray(original)).cuda()
    swz = swizzle(A, swz_name)
    want, want_h, decoded = two_calls(product, A, ctx, t_blocks, t_image, dims, image_type, decode_type, swz, hdr)
    n = block_count(block, dims)
    got, got_h, per_block = fused(product, A, ctx, t_blocks, t_image, dims, image_type, decode_type, swz, hdr, per_block=n)
    close(got.squared_error, want.squared_error, what + " squared error")
    close(got.alpha_scaled_squared_error, want.alpha_scaled_squared_error, what + " alpha-scaled")
    assert got.rgb_peak == want.rgb_peak and got.texels == want.texels == dims[0] * dims[1] * dims[2], what
    if hdr is not None:
        close(got_h.log2_squared_error, want_h.log2_squared_error, what + " log2")
        close(got_h.mpsnr_squared_error, want_h.mpsnr_squared_error, what + " mPSNR")
        assert (got_h.fstop_lo, got_h.fstop_hi) == hdr
    close(per_block, block_model(original, decoded, block, dims), what + " per block")
    close(per_block.sum(axis=0), got.squared_error, what + " blocks against the total")
    # without the per-block output: the same doubles
    again, again_h, _ = fused(product, A, ctx, t_blocks, t_image, dims, image_type, decode_type, swz, hdr)
    assert bytes(again) == bytes(got) and (hdr is None or bytes(again_h) == bytes(got_h)), what
    # nothing but the records is written
    assert np.array_equal(t_blocks.cpu().numpy(), stream_bytes) and t_image.cpu().numpy().tobytes() == np.ascontiguousarray(original).tobytes(), what
    return got


@pytest.mark.parametrize("block,dims", SHAPES, ids=SHAPE_IDS)
def test_shapes_ldr(product, A, contexts, block, dims):
    """U8 against U8 in an LDR context: the library's own -thorough streams and random bit patterns, every swizzle."""
    ctx = contexts(block)
    names = list(SWIZZLES)
    for i, kind in enumerate(("noisy", "flat", "two_colour")):
        original = source_image(kind, dims)
        data = compressed_stream(product, A, kind, block, dims)
        sums = check_case(product, A, ctx, block, dims, data, original, A.TYPE_U8, "rgba", what=kind)
        if kind == "noisy" and dims[0] * dims[1] > 64 and (dims[2] == 1 or len(block) > 2):
            assert 20.0 < sums.psnr() < 70.0, sums.psnr()          # (the comparison is with the right image)
        check_case(product, A, ctx, block, dims, data, original, A.TYPE_U8, names[1 + i], what=kind)
    original = source_image("noisy", dims, seed=9)
    for name in ("rgba", "gggr", "ra_z1"):
        check_case(product, A, ctx, block, dims, random_stream(block, dims, 31 + dims[0]), original, A.TYPE_U8, name, what="random")


@pytest.mark.parametrize("block,dims", [SHAPES[i] for i in (1, 4, 5, 6, 7, 9)], ids=[SHAPE_IDS[i] for i in (1, 4, 5, 6, 7, 9)])
def test_shapes_other_profiles(product, A, contexts, block, dims):
    """LDR_SRGB U8 / U8; an F16 original against F16 and F32 decodes in an HDR context, with the HDR sums over two f-stop
    ranges; an F32 original against a U8 decode in an HDR_RGB_LDR_A context."""
    img8 = source_image("noisy", dims)
    ldr_stream = compressed_stream(product, A, "two_colour", block, dims)
    rnd = random_stream(block, dims, 77 + dims[1])
    srgb = contexts(block, A.PRF_LDR_SRGB)
    check_case(product, A, srgb, block, dims, compressed_stream(product, A, "noisy", block, dims, A.PRF_LDR_SRGB), img8, A.TYPE_U8, "rgba", what="srgb")
    check_case(product, A, srgb, block, dims, rnd, img8, A.TYPE_U8, "bgra", what="srgb random")
    hdr = contexts(block, A.PRF_HDR)
    half = as_type(img8, 1)
    hdr_image = np.stack([images.hdr_f16(dims[0], dims[1], 40 + z) for z in range(dims[2])]).astype(np.float16)
    hdr_stream = product.compress(hdr_image if dims[2] > 1 or len(block) > 2 else hdr_image[0], block, A.PRE_THOROUGH, A.PRF_HDR)
    check_case(product, A, hdr, block, dims, hdr_stream, hdr_image, A.TYPE_F16, "rgba", hdr=(-10, 10), what="hdr image")
    check_case(product, A, hdr, block, dims, hdr_stream, hdr_image, A.TYPE_F32, "rgba", hdr=(-2, 3), what="hdr image")
    for decode_type, name, stops in ((A.TYPE_F16, "rgba", (-10, 10)), (A.TYPE_F16, "gggr", (-2, 3)), (A.TYPE_F32, "bgra", (-2, 3)), (A.TYPE_F32, "ra_z1", None)):
        check_case(product, A, hdr, block, dims, rnd, half, decode_type, name, hdr=stops, what="hdr random")
    check_case(product, A, hdr, block, dims, ldr_stream, half, A.TYPE_F16, "rrr1", hdr=(-2, 3), what="hdr ldr stream")
    mixed = contexts(block, A.PRF_HDR_RGB_LDR_A)
    check_case(product, A, mixed, block, dims, rnd, as_type(img8, 2), A.TYPE_U8, "rgba", what="hdr rgb ldr a random")
    check_case(product, A, mixed, block, dims, ldr_stream, as_type(img8, 2), A.TYPE_U8, "bgra", what="hdr rgb ldr a")


def test_memory_discipline(product, A, contexts):
    import torch
    block, dims = (4, 4), (134, 10, 1)
    ctx = contexts(block)
    n = block_count(block, dims)
    original = source_image("noisy", dims)
    data = compressed_stream(product, A, "noisy", block, dims)
    t_blocks, t_image = torch.from_numpy(data).cuda(), torch.from_numpy(original).cuda()
    want, _, per_block = fused(product, A, ctx, t_blocks, t_image, dims, 0, 0, A.SWZ_RGBA, per_block=n)
    # guard bytes on both sides of the records
    records = Guarded(product, np.full(n * 32, 0xCD, dtype=np.uint8))
    swz, sums = A.Swizzle(*A.SWZ_RGBA), A.ErrorSums()
    err = product.lib.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 134, 10, 1, 0, 0, C.byref(swz),
                                                        records.ptr, n * 32, None, C.byref(sums))
    assert err == 0 and bytes(sums) == bytes(want)
    assert np.array_equal(records.payload("block records").view(np.float64).reshape(-1, 4), per_block)
    # a longer buffer than needed: the rest is not touched
    records = Guarded(product, np.full(n * 32 + 64, 0xCD, dtype=np.uint8))
    err = product.lib.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 134, 10, 1, 0, 0, C.byref(swz),
                                                        records.ptr, n * 32 + 64, None, C.byref(sums))
    assert err == 0 and (records.payload("long block records")[n * 32:] == 0xCD).all()
    # sub-views of an allocation: the original of every type at 4, 8 and 12 bytes past a 16-byte boundary, the records at 8 (doubles)
    for t, image in ((0, original), (1, as_type(original, 1)), (2, as_type(original, 2))):
        flat = np.ascontiguousarray(image).view(np.uint8).reshape(-1)
        base = fused(product, A, ctx, t_blocks, torch.from_numpy(flat).cuda(), dims, t, 0, A.SWZ_RGBA, per_block=n)
        for offset in (4, 8, 12):
            whole_i = torch.full((flat.size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            whole_r = torch.full((n * 32 + 64,), 0xEE, dtype=torch.uint8, device="cuda")
            assert whole_i.data_ptr() % 16 == 0 and whole_r.data_ptr() % 16 == 0
            whole_i[offset:offset + flat.size] = torch.from_numpy(flat).cuda()
            err = product.lib.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, whole_i.data_ptr() + offset, 134, 10, 1, t, 0,
                                                                C.byref(swz), whole_r.data_ptr() + 8, n * 32, None, C.byref(sums))
            assert err == 0, (t, offset)
            assert bytes(sums) == bytes(base[0]), (t, offset)
            r = whole_r.cpu().numpy()
            assert np.array_equal(r[8:8 + n * 32].view(np.float64).reshape(-1, 4), base[2]) and (r[:8] == 0xEE).all() and (r[8 + n * 32:] == 0xEE).all()
            i = whole_i.cpu().numpy()
            assert np.array_equal(i[offset:offset + flat.size], flat) and (i[:offset] == 0xEE).all() and (i[offset + flat.size:] == 0xEE).all()
    # the argument checks: nothing is written
    sums.texels = -1.0
    records = Guarded(product, np.full(n * 32, 0xCD, dtype=np.uint8))
    L = product.lib
    common = (134, 10, 1, 0, 0, C.byref(swz))
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), *common, records.ptr, n * 32 - 1, None, C.byref(sums)) == A.ERR_OUT_OF_MEM
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes - 1, t_image.data_ptr(), *common, records.ptr, n * 32, None, C.byref(sums)) == A.ERR_OUT_OF_MEM
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, None, *common, records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_device(ctx, None, data.nbytes, t_image.data_ptr(), *common, records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 0, 10, 1, 0, 0, C.byref(swz), records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 134, 10, 1, 3, 0, C.byref(swz), records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 134, 10, 1, 0, 5, C.byref(swz), records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_PARAM
    bad = A.Swizzle(A.SWZ_R, A.SWZ_G, A.SWZ_B, 9)
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), 134, 10, 1, 0, 0, C.byref(bad), records.ptr, n * 32, None, C.byref(sums)) == A.ERR_BAD_SWIZZLE
    assert L.astcenc_amd_compare_blocks_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), *common, records.ptr, n * 32, None, None) == A.ERR_BAD_PARAM
    hs = A.HdrErrorSums()
    for lo, hi in ((-126, 0), (0, 126), (3, 2)):
        assert L.astcenc_amd_compare_blocks_hdr_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), *common, records.ptr, n * 32, lo, hi, None,
                                                       C.byref(sums), C.byref(hs)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_hdr_device(ctx, t_blocks.data_ptr(), data.nbytes, t_image.data_ptr(), *common, records.ptr, n * 32, -1, 1, None,
                                                   C.byref(sums), None) == A.ERR_BAD_PARAM
    assert sums.texels == -1.0 and (records.payload("rejected calls") == 0xCD).all()


SET_DIMS = [(20, 12, 1), (10, 6, 1), (5, 3, 1), (2, 1, 1), (1, 1, 1), (134, 10, 1), (40, 20, 3)]


def test_image_set(product, A, contexts):
    import torch
    block = (6, 6)
    ctx = contexts(block)
    originals = [source_image("noisy", d, seed=60 + i) for i, d in enumerate(SET_DIMS)]
    streams = [compressed_stream(product, A, "noisy", block, d) if i % 2 == 0 else random_stream(block, d, 90 + i) for i, d in enumerate(SET_DIMS)]
    t_images = [torch.from_numpy(o if d[2] > 1 else o[0]).cuda() for o, d in zip(originals, SET_DIMS)]
    t_blocks = [torch.from_numpy(s).cuda() for s in streams]
    counts = [block_count(block, d) for d in SET_DIMS]
    total = sum(counts)
    records = Guarded(product, np.full(total * 32, 0xCD, dtype=np.uint8))
    entries = [A.image_set_entry(i, b) for i, b in zip(t_images, t_blocks)]
    arr = (A.ImageSetEntry * len(entries))(*entries)
    sums = (A.ErrorSums * len(entries))()
    err = product.lib.astcenc_amd_compare_image_set_device(ctx, arr, len(entries), records.ptr, total * 32, None, sums)
    assert err == 0, product.error_string(err)
    got = records.payload("set records").view(np.float64).reshape(-1, 4)
    at = 0
    for i, d in enumerate(SET_DIMS):
        alone, _, per_block = fused(product, A, ctx, t_blocks[i], t_images[i], d, 0, 0, A.SWZ_RGBA, per_block=counts[i])
        assert bytes(sums[i]) == bytes(alone), (i, d)
        assert np.array_equal(got[at:at + counts[i]], per_block), (i, d)
        at += counts[i]
        want, _, decoded = two_calls(product, A, ctx, t_blocks[i], t_images[i], d, 0, 0, A.SWZ_RGBA)
        close(sums[i].squared_error, want.squared_error, "entry %d" % i)
        assert sums[i].rgb_peak == want.rgb_peak and sums[i].texels == want.texels
    # the binding, without records
    err, listed = product.compare_image_set_device(ctx, list(zip(t_images, t_blocks)))
    assert err == 0 and [bytes(s) for s in listed] == [bytes(s) for s in sums]
    # rejected without a write: a bad entry (named in the log), a short records buffer, entries without sums
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        records = Guarded(product, np.full(total * 32, 0xCD, dtype=np.uint8))
        fresh = (A.ErrorSums * len(entries))()
        for s in fresh:
            s.texels = -1.0
        for index, change, code in ((2, dict(dim_x=0), A.ERR_BAD_PARAM), (5, dict(blocks_len=16), A.ERR_OUT_OF_MEM), (6, dict(image=None), A.ERR_BAD_PARAM),
                                    (3, dict(swizzle=A.Swizzle(0, 1, 2, 9)), A.ERR_BAD_SWIZZLE), (4, dict(data_type=3), A.ERR_BAD_PARAM)):
            bad = (A.ImageSetEntry * len(entries))(*[A.image_set_entry(i, b) for i, b in zip(t_images, t_blocks)])
            for field, value in change.items():
                setattr(bad[index], field, value)
            del logged[:]
            assert product.lib.astcenc_amd_compare_image_set_device(ctx, bad, len(entries), records.ptr, total * 32, None, fresh) == code, (index, change)
            assert any("entry %d of %d" % (index, len(entries)) in line for line in logged), (index, logged)
        assert product.lib.astcenc_amd_compare_image_set_device(ctx, arr, len(entries), records.ptr, total * 32 - 1, None, fresh) == A.ERR_OUT_OF_MEM
        assert product.lib.astcenc_amd_compare_image_set_device(ctx, arr, len(entries), records.ptr, total * 32, None, None) == A.ERR_BAD_PARAM
        assert product.lib.astcenc_amd_compare_image_set_device(ctx, None, 2, records.ptr, total * 32, None, fresh) == A.ERR_BAD_PARAM
        assert product.lib.astcenc_amd_compare_image_set_device(ctx, arr, 0, records.ptr, total * 32, None, fresh) == A.SUCCESS
        assert all(s.texels == -1.0 for s in fresh) and (records.payload("rejected sets") == 0xCD).all()
    finally:
        product.lib.astcenc_amd_set_log_callback(None)


def test_launch_logic(product, A, contexts):
    import torch
    block, dims = (12, 12), (390, 13, 1)
    ctx = contexts(block)
    original = source_image("noisy", dims)
    data = compressed_stream(product, A, "noisy", block, dims)
    t_blocks, t_image = torch.from_numpy(data).cuda(), torch.from_numpy(original).cuda()
    n = block_count(block, dims)
    runs = [fused(product, A, ctx, t_blocks, t_image, dims, 0, 0, A.SWZ_RGBA, per_block=n) for _ in range(3)]
    assert bytes(runs[0][0]) == bytes(runs[1][0]) == bytes(runs[2][0])
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][2], runs[2][2])
    # one block after the large call on the same context: the partials of the earlier runs are stale, not part of the sums
    one = source_image("noisy", (1, 1, 1), seed=3)
    one_blocks = random_stream(block, (1, 1, 1), 4)
    check_case(product, A, ctx, block, (1, 1, 1), one_blocks, one, A.TYPE_U8, "rgba", what="one block after large")
    check_case(product, A, ctx, block, dims, data, original, A.TYPE_U8, "rgba", what="large again")
    # a side stream with a pending producer: blocks and original arrive by copies queued behind a long kernel
    rng = np.random.default_rng(6)
    side = torch.cuda.Stream()
    h_blocks, h_img = torch.from_numpy(data).pin_memory(), torch.from_numpy(original).pin_memory()
    d_blocks = torch.from_numpy(rng.integers(0, 256, data.shape, dtype=np.uint8)).cuda()
    d_img = torch.from_numpy(rng.integers(0, 256, original.shape, dtype=np.uint8)).cuda()
    errors = torch.full((n * 4,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    swz, sums = A.Swizzle(*A.SWZ_RGBA), A.ErrorSums()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        d_blocks.copy_(h_blocks, non_blocking=True)
        d_img.copy_(h_img, non_blocking=True)
        err = product.lib.astcenc_amd_compare_blocks_device(ctx, d_blocks.data_ptr(), data.nbytes, d_img.data_ptr(), 390, 13, 1, 0, 0, C.byref(swz),
                                                            errors.data_ptr(), n * 32, A.torch_stream(side), C.byref(sums))
    assert err == 0
    side.synchronize()
    assert bytes(sums) == bytes(runs[0][0]) and np.array_equal(errors.cpu().numpy().reshape(-1, 4), runs[0][2])


def test_many_runs(product, A, contexts):
    """170 runs in one entry: lanes of the finish pass with two and with three partials, more than 64 runs."""
    block, dims = (4, 4), (2100, 40, 1)
    original = source_image("noisy", dims)
    check_case(product, A, contexts(block), block, dims, random_stream(block, dims, 12), original, A.TYPE_U8, "rgba", what="170 runs")


SPLIT_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import astcenc_amd as A
import test_block_quality as T
product = A.Library(A.LIB_PRODUCT)
torch.zeros(1, device="cuda:0")
made = {}
def contexts(block, profile=None):
    profile = A.PRF_LDR if profile is None else profile
    if (block, profile) not in made:
        err, cfg = product.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, A.PRE_MEDIUM, 0)
        err, ctx = product.context_alloc(cfg, 1)
        assert err == 0
        made[(block, profile)] = ctx
    return made[(block, profile)]
for block, dims in (((4, 4), (134, 10, 1)), ((12, 12), (390, 13, 1)), ((6, 6), (40, 20, 3)), ((3, 3, 3), (100, 4, 4)), ((4, 4), (700, 9, 1))):
    original = T.source_image("noisy", dims)
    T.check_case(product, A, contexts(block), block, dims, T.random_stream(block, dims, 5), original, A.TYPE_U8, "rgba", what="split")
half = T.as_type(T.source_image("noisy", (134, 10, 1)), 1)
T.check_case(product, A, contexts((4, 4), A.PRF_HDR), (4, 4), (134, 10, 1), T.random_stream((4, 4), (134, 10, 1), 8), half, A.TYPE_F16, "rgba", hdr=(-2, 3), what="split hdr")
T.test_image_set(product, A, contexts)
print("split launches ok")
"""


def test_split_launches(product, A):
    """Pieces of two runs (the limit is read once per process: a fresh one): every entry above two runs is finished in several
    passes, and launches hold the tail of one entry with the head of the next."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ASTCENC_AMD_DECODE_GRID_LIMIT="2")
    script = SPLIT_SCRIPT % (os.path.join(root, "astc-encoder_amd", "python"), os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "split launches ok" in out.stdout, out.stdout[-2000:]
