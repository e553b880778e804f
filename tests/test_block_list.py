# SPDX-License-Identifier: Apache-2.0
"""The block-list launch of the compression kernel (astcenc_amd_compress_block_list_device; csrc/kernel_device.h,
csrc/astcenc_adaptive.cpp).

The yardstick is astcenc_amd_compress_volume_device on the same context and arguments.  The output buffer is filled with 0xA5
and has 64 guard bytes on both sides; after a list call the listed in-range blocks equal the full call's and every other byte is
still 0xA5.

One case per build of the kernel and per input path (CASES): the generic builds for small and large footprints, LDR and HDR, the
fixed-context builds, a 3D footprint, a 2D footprint over slices, the alpha-scale pre-pass, a run-time build, and the generic
build of a context that has a fixed one (a fresh process with ASTCENC_AMD_KERNEL=generic).

Lists (lists_for): empty, one block, all ascending, all reversed, every third, [5, 5, 5], the first 7, 8 and 9 blocks (the XCD
remap changes at a multiple of 8), and a list with `blocks` and 0xFFFFFFFF mixed in.

One-line mistakes these catch: the output indexed by list position instead of block index (reversed, every third); `first` added
before the lookup instead of after, or the remap applied to the index instead of the position (8 and 9 blocks, reversed); a
pre-pass skipped (the alpha-scale case, whose image has a transparent patch that only the pre-pass turns into constant
blocks); an out-of-range index written (guards, the stale list); list_count == 0 launching a zero grid (an error code)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import images

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA5


def alpha_image():
    """flat_regions with a fully transparent patch of varying colour: constant-zero blocks only with the pre-pass."""
    img = images.flat_regions(50, 45)
    img[24:45, 26:50, 3] = 0
    return img


# name: (profile, block, quality, flags, tweak, image maker, kernel name or prefix expected)
CASES = {
    "4x4_fast_ldr64": ("PRF_LDR", (4, 4), "PRE_FAST", 0, None, lambda: images.flat_regions(50, 45), "astc_compress_blocks_ldr64"),
    "6x6_medium_fixed": ("PRF_LDR", (6, 6), "PRE_MEDIUM", 0, None, lambda: images.flat_regions(50, 45), "astc_compress_blocks_ldr_6x6m"),
    "12x12_fast_ldr": ("PRF_LDR", (12, 12), "PRE_FAST", 0, None, lambda: images.noisy(134, 50), "astc_compress_blocks_ldr"),
    "6x6_medium_hdr_fixed": ("PRF_HDR", (6, 6), "PRE_MEDIUM", 0, None, lambda: images.hdr_f16(50, 45).astype(np.float16), "astc_compress_blocks_hdr_6x6m"),
    "5x5_fast_hdr64": ("PRF_HDR", (5, 5), "PRE_FAST", 0, None, lambda: images.hdr_f16(50, 45).astype(np.float16), "astc_compress_blocks_hdr64"),
    "3x3x3_fast": ("PRF_LDR", (3, 3, 3), "PRE_FAST", 0, None, lambda: images.volume("grad", 5, 7, 10), "astc_compress_blocks_ldr64"),
    "6x6_slices": ("PRF_LDR", (6, 6), "PRE_MEDIUM", 0, None, lambda: np.stack([images.noisy(40, 20, 5 + z) for z in range(3)]), "astc_compress_blocks_ldr_6x6m"),
    "alpha_scale": ("PRF_LDR", (6, 6), "PRE_FAST", "FLG_USE_ALPHA_WEIGHT", {"a_scale_radius": 2}, lambda: images.flat_regions(50, 45), "astc_compress_blocks_ldr64"),
    "alpha_scale_patch": ("PRF_LDR", (6, 6), "PRE_FAST", "FLG_USE_ALPHA_WEIGHT", {"a_scale_radius": 2}, alpha_image, "astc_compress_blocks_ldr64"),
}


def make_context(product, A, profile, block, quality, flags, tweak):
    err, cfg = product.config_init(getattr(A, profile), block[0], block[1], block[2] if len(block) > 2 else 1, getattr(A, quality),
                                   getattr(A, flags) if flags else 0)
    assert err == 0
    for field, value in (tweak or {}).items():
        setattr(cfg, field, value)
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0, product.error_string(err)
    return ctx


def block_count(block, shape):
    d = shape[0] if len(shape) == 4 else 1
    bz = block[2] if len(block) > 2 else 1
    return -(-shape[-2] // block[0]) * -(-shape[-3] // block[1]) * -(-d // bz)


def full_stream(product, A, ctx, t_image, n):
    """The yardstick: the whole image through astcenc_amd_compress_volume_device."""
    import torch
    out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    args, s = product._image_args(t_image, None)
    err = product.lib.astcenc_amd_compress_volume_device(ctx, *args, C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(), s, None)
    assert err == 0, product.error_string(err)
    return out.cpu().numpy().reshape(n, 16)


def lists_for(n):
    every = np.arange(n, dtype=np.uint32)
    stale = np.array([1 % n, n, 0xFFFFFFFF, 0, n + 1, 0x80000000, n - 1], dtype=np.uint32)
    return {"empty": every[:0], "one": every[n // 2:n // 2 + 1], "ascending": every, "reversed": every[::-1].copy(), "every third": every[::3].copy(),
            "repeated": np.array([5 % n] * 3, dtype=np.uint32), "first 7": every[:7], "first 8": every[:8], "first 9": every[:9], "stale": stale}


def run_list(product, ctx, t_image, n, block_list):
    """One list call into a guarded 0xA5 buffer; returns (error, the whole buffer on the host)."""
    import torch
    whole = torch.full((GUARD + n * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    t_list = torch.from_numpy(block_list.view(np.int32)).cuda() if block_list.size else None
    err = product.compress_block_list_device(ctx, t_image, t_list, whole[GUARD:GUARD + n * 16])
    return err, whole.cpu().numpy()


def check_lists(product, A, ctx, image, block, what):
    import torch
    t_image = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    n = block_count(block, image.shape)
    want = full_stream(product, A, ctx, t_image, n)
    assert n > 9, what
    for name, block_list in lists_for(n).items():
        err, got = run_list(product, ctx, t_image, n, block_list)
        assert err == 0, (what, name, product.error_string(err))
        expect = np.full((n, 16), FILL, dtype=np.uint8)
        listed = np.unique(block_list[block_list < n]).astype(np.int64)
        expect[listed] = want[listed]
        assert (got[:GUARD] == FILL).all() and (got[GUARD + n * 16:] == FILL).all(), (what, name, "guards")
        bad = np.flatnonzero((got[GUARD:GUARD + n * 16].reshape(n, 16) != expect).any(axis=1))
        assert bad.size == 0, (what, name, "blocks that differ", bad[:16], "listed", listed[:16])
    return want


@pytest.fixture(scope="module")
def case_context(product, A):
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_context(product, A, *CASES[name][:5])
        return made[name]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


@pytest.mark.parametrize("name", list(CASES))
def test_lists(product, A, case_context, name):
    ctx = case_context(name)
    assert product.lib.astcenc_amd_context_kernel_name(ctx).decode() == CASES[name][6]
    want = check_lists(product, A, ctx, CASES[name][5](), CASES[name][1], name)
    if name == "alpha_scale_patch":
        # (the case is about the pre-pass: without it the transparent patch is not made of constant blocks)
        plain = make_context(product, A, "PRF_LDR", (6, 6), "PRE_FAST", "FLG_USE_ALPHA_WEIGHT", None)
        try:
            import torch
            image = alpha_image()
            other = full_stream(product, A, plain, torch.from_numpy(image).cuda(), want.shape[0])
        finally:
            product.context_free(plain)
        assert (other != want).any(axis=1).sum() > 0


def test_run_time_build(product, A, tmp_path, monkeypatch):
    from jit_builds import is_jit, prewarm
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", str(tmp_path / "cache"))
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    prewarm(str(tmp_path / "cache"), [(A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0)])       # (compiled on the CPU, found in the cache)
    ctx = make_context(product, A, "PRF_LDR", (6, 6), "PRE_THOROUGH", 0, None)
    try:
        assert is_jit(product.lib.astcenc_amd_context_kernel_name(ctx).decode())
        check_lists(product, A, ctx, images.flat_regions(50, 45), (6, 6), "run-time build")
    finally:
        product.context_free(ctx)


GENERIC_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import torch
import astcenc_amd as A
import test_block_list as T
product = A.Library(A.LIB_PRODUCT)
torch.zeros(1, device="cuda:0")
ctx = T.make_context(product, A, *T.CASES["6x6_medium_fixed"][:5])
assert product.lib.astcenc_amd_context_kernel_name(ctx).decode() == "astc_compress_blocks_ldr64"
T.check_lists(product, A, ctx, T.CASES["6x6_medium_fixed"][5](), (6, 6), "generic build")
print("generic build ok")
"""


def test_generic_build_of_a_fixed_context(product, A):
    """(the choice of the build is made once per context from the environment: a fresh process)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ASTCENC_AMD_KERNEL="generic")
    script = GENERIC_SCRIPT % (os.path.join(root, "astc-encoder_amd", "python"), os.path.join(root, "tests"), os.path.join(root, "oracle"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "generic build ok" in out.stdout, out.stdout[-2000:]


def test_errors_write_nothing(product, A, case_context):
    import torch
    ctx = case_context("6x6_medium_fixed")
    image = images.flat_regions(50, 45)
    t_image = torch.from_numpy(image).cuda()
    n = block_count((6, 6), image.shape)
    whole = torch.full((GUARD + n * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = whole[GUARD:GUARD + n * 16]
    t_list = torch.arange(n, dtype=torch.int32, device="cuda")
    # a null list with a non-zero count; a short data_len; a null image; a bad swizzle; a zero dimension
    assert product.compress_block_list_device(ctx, t_image, None, out, list_count=3) == A.ERR_BAD_CONTEXT
    assert product.compress_block_list_device(ctx, t_image, t_list, out, data_len=n * 16 - 1) == A.ERR_OUT_OF_MEM
    L, swz = product.lib, A.Swizzle(*A.SWZ_RGBA)
    assert L.astcenc_amd_compress_block_list_device(ctx, None, 50, 45, 1, 0, C.byref(swz), t_list.data_ptr(), n, out.data_ptr(), n * 16, None, None) == A.ERR_BAD_CONTEXT
    assert L.astcenc_amd_compress_block_list_device(ctx, t_image.data_ptr(), 50, 45, 1, 0, C.byref(A.Swizzle(0, 1, 2, 9)), t_list.data_ptr(), n, out.data_ptr(), n * 16,
                                                    None, None) == A.ERR_BAD_SWIZZLE
    assert L.astcenc_amd_compress_block_list_device(ctx, t_image.data_ptr(), 0, 45, 1, 0, C.byref(swz), t_list.data_ptr(), n, out.data_ptr(), n * 16, None, None) == A.ERR_BAD_PARAM
    # a decompress-only context
    err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, dctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        assert product.compress_block_list_device(dctx, t_image, t_list, out) == A.ERR_BAD_CONTEXT
    finally:
        product.context_free(dctx)
    # an empty list succeeds with a kernel time of zero, and a null list is then legal
    assert product.compress_block_list_device(ctx, t_image, None, out) == A.SUCCESS and product.last_kernel_ms == 0.0
    assert (whole.cpu().numpy() == FILL).all()
    # kernel_ms of a real launch is positive
    assert product.compress_block_list_device(ctx, t_image, t_list, out) == A.SUCCESS and product.last_kernel_ms > 0.0
