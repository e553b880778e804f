# SPDX-License-Identifier: Apache-2.0
"""The block-list launch over an image set (astcenc_amd_compress_block_list_set_device; csrc/kernel_device.h: the list names global
block indices, which go through the set's lookup; csrc/backend_hip.hip: compress_set_on_slot).

The set is the chain of images.flat_regions(50, 45) made with the numpy mip model: at 6x6 its levels hold 72 + 20 + 4 + 1 + 1 + 1
= 99 blocks in 6 entries.  The expected bytes are those astcenc_amd_compress_images_device writes for the same entries.  Every
entry's buffer is prefilled with 0xA5 between guards; after a list call the listed blocks (those below the set's total) hold the
expected bytes and every other byte, the guards included, is still 0xA5.

Cases (CASES): 6x6 and 4x4 at -fastest; a U8 set whose second entry is F16; and a context with a_scale_radius != 0, whose
pre-pass runs per entry over the whole entry.  Lists (lists_of): every block, every third, the first and last block of each
entry, reversed, with duplicates, with stale indices (total, total + 1, 2^32 - 1), empty.

The same cases run in child processes with ASTCENC_AMD_COMPRESS_GRID = 8 (every launch draws its blocks from tickets) and = 0
(one workgroup per block), the mechanism of tests/test_persistent_grid.py: the variable is read once per process, so fresh
children, started here and never replaced."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import images
import mip_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GUARD = 64


def chain_u8():
    return [np.ascontiguousarray(level) for level in mip_model.chain(images.flat_regions(50, 45))]


def chain_mixed():
    levels = chain_u8()
    levels[1] = (levels[1].astype(np.float32) / 255.0).astype(np.float16)
    return levels


def chain_transparent():
    """Two fully transparent patches in level 0, wide enough for blocks whose whole neighbourhood is transparent."""
    img = images.flat_regions(50, 45).copy()
    img[4:30, 24:50, 3] = 0
    return [np.ascontiguousarray(level) for level in mip_model.chain(img)]


def set_radius(cfg):
    cfg.a_scale_radius = 2


# name -> (footprint, flags name or None, config tweak, the set's images)
CASES = {
    "6x6": ((6, 6), None, None, chain_u8),
    "4x4": ((4, 4), None, None, chain_u8),
    "mixed_types": ((6, 6), None, None, chain_mixed),
    "alpha_scale": ((6, 6), "FLG_USE_ALPHA_WEIGHT", set_radius, chain_transparent),
}


def entry_blocks(block, levels):
    return [-(-l.shape[1] // block[0]) * -(-l.shape[0] // block[1]) for l in levels]


def lists_of(counts):
    total = sum(counts)
    first = np.cumsum([0] + counts[:-1])
    ends = sorted(set(int(f) for f in first) | set(int(f + c - 1) for f, c in zip(first, counts)))
    every = np.arange(total, dtype=np.uint32)
    return {
        "all": every,
        "every_third": every[::3],
        "entry_ends": np.array(ends, dtype=np.uint32),
        "reversed": every[::-1].copy(),
        "duplicates": np.array([5, 5, total - 1, 0, 5, total - 1, counts[0], counts[0]], dtype=np.uint32),
        "stale": np.array([3, total, total + 1, 0xFFFFFFFF, counts[0] + 1, 0x80000000, total - 1], dtype=np.uint32),
        "empty": np.zeros(0, dtype=np.uint32),
    }


def run_case(product, A, name):
    """{"want": the set call's bytes, entry after entry; <list name>: every entry's guarded buffer after the list call, entry
    after entry}."""
    import torch
    block, flags, tweak, make = CASES[name]
    err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], 1, A.PRE_FASTEST, getattr(A, flags) if flags else 0)
    assert err == 0
    if tweak:
        tweak(cfg)
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0, product.error_string(err)
    try:
        levels = make()
        counts = entry_blocks(block, levels)
        t_images = [torch.from_numpy(l).cuda() for l in levels]
        full = [torch.zeros(c * 16, dtype=torch.uint8, device="cuda") for c in counts]
        err = product.compress_images_device(ctx, list(zip(t_images, full)))
        assert err == 0, product.error_string(err)
        result = {"want": np.concatenate([f.cpu().numpy() for f in full])}
        for list_name, indices in lists_of(counts).items():
            whole = [torch.full((GUARD + c * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda") for c in counts]
            entries = [(t, w[GUARD:GUARD + c * 16]) for t, w, c in zip(t_images, whole, counts)]
            t_list = torch.from_numpy(indices.view(np.int32)).cuda() if indices.size else None
            err = product.compress_block_list_set_device(ctx, entries, t_list)
            assert err == 0, (name, list_name, product.error_string(err))
            assert (product.last_kernel_ms > 0.0) == (indices.size > 0), (name, list_name)
            result[list_name] = np.concatenate([w.cpu().numpy() for w in whole])
        return result
    finally:
        product.context_free(ctx)


def check_case(name, result, what):
    block, _, _, make = CASES[name]
    counts = entry_blocks(block, make())
    total = sum(counts)
    want = result["want"].reshape(total, 16)
    assert (want != FILL).any(axis=1).all()                   # (no expected block looks like the prefill)
    for list_name, indices in lists_of(counts).items():
        listed = np.zeros(total, dtype=bool)
        listed[indices[indices < total]] = True
        whole = result[list_name]
        assert whole.size == total * 16 + 2 * GUARD * len(counts)
        at = g = 0
        for c in counts:
            part = whole[at:at + GUARD + c * 16 + GUARD]
            assert (part[:GUARD] == FILL).all() and (part[GUARD + c * 16:] == FILL).all(), (what, name, list_name, "guards")
            got = part[GUARD:GUARD + c * 16].reshape(c, 16)
            expect = np.where(listed[g:g + c, None], want[g:g + c], np.uint8(FILL))
            bad = np.flatnonzero((got != expect).any(axis=1))
            assert bad.size == 0, (what, name, list_name, "global blocks that differ", (bad + g)[:16])
            at += GUARD + c * 16 + GUARD
            g += c
        if list_name == "empty":
            assert (whole == FILL).all()


def test_the_set_and_its_lists():
    counts = entry_blocks((6, 6), chain_u8())
    assert counts == [72, 20, 4, 1, 1, 1]
    lists = lists_of(counts)
    assert lists["entry_ends"].tolist() == [0, 71, 72, 91, 92, 95, 96, 97, 98]
    assert set(lists["stale"].tolist()) >= {99, 100, 0xFFFFFFFF}
    assert chain_mixed()[1].dtype == np.float16 and chain_mixed()[0].dtype == np.uint8


@pytest.mark.parametrize("name", list(CASES))
def test_lists_in_this_process(product, A, name):
    check_case(name, run_case(product, A, name), "default launch path")


def child_main(path):
    """(child process) every case through the product library, the results into the .npz at `path`."""
    import torch
    import astcenc_amd as A
    torch.zeros(1, device="cuda:0")
    product = A.Library(A.LIB_PRODUCT)
    out = {}
    for name in CASES:
        for key, value in run_case(product, A, name).items():
            out[name + "/" + key] = value
    np.savez(path, **out)


@pytest.mark.parametrize("grid", ["8", "0"])
def test_lists_on_both_launch_paths(grid, tmp_path):
    path = str(tmp_path / "lists.npz")
    script = "import sys; sys.path[:0] = %r; import test_block_list_set as T; T.child_main(%r)" % (
        [os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")], path)
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, ASTCENC_AMD_COMPRESS_GRID=grid), timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    loaded = dict(np.load(path))
    for name in CASES:
        check_case(name, {key.split("/", 1)[1]: value for key, value in loaded.items() if key.startswith(name + "/")}, "ASTCENC_AMD_COMPRESS_GRID=" + grid)


def test_errors_write_nothing(product, A):
    import torch
    levels = chain_u8()
    counts = entry_blocks((6, 6), levels)
    err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, 0)
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        t_images = [torch.from_numpy(l).cuda() for l in levels]
        whole = [torch.full((GUARD + c * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda") for c in counts]
        t_list = torch.arange(99, dtype=torch.int32, device="cuda")
        L = product.lib

        def entries_of(change=None):
            e = [A.image_set_entry(t, w[GUARD:GUARD + c * 16]) for t, w, c in zip(t_images, whole, counts)]
            if change:
                change(e)
            return (A.ImageSetEntry * len(e))(*e)

        def call(ctx=ctx, entries=entries_of(), n=len(counts), lst=t_list.data_ptr(), count=99):
            return L.astcenc_amd_compress_block_list_set_device(ctx, entries, n, lst, count, None, None)

        def short(e):
            e[1].blocks_len = counts[1] * 16 - 1

        def null_image(e):
            e[2].image = None

        def zero_dim(e):
            e[3].dim_x = 0

        def bad_swizzle(e):
            e[0].swizzle = A.Swizzle(0, 1, 2, 9)

        assert call(ctx=None) == A.ERR_BAD_PARAM and call(entries=None) == A.ERR_BAD_PARAM
        assert call(entries=entries_of(short)) == A.ERR_OUT_OF_MEM
        assert call(entries=entries_of(null_image)) == A.ERR_BAD_CONTEXT
        assert call(entries=entries_of(zero_dim)) == A.ERR_BAD_PARAM
        assert call(entries=entries_of(bad_swizzle)) == A.ERR_BAD_SWIZZLE
        assert call(lst=None) == A.ERR_BAD_CONTEXT
        # (an empty list and an empty set succeed and launch nothing)
        assert call(count=0) == A.SUCCESS and call(lst=None, count=0) == A.SUCCESS and call(entries=None, n=0) == A.SUCCESS
        torch.cuda.synchronize()
        assert all((w.cpu().numpy() == FILL).all() for w in whole)
    finally:
        product.context_free(ctx)
