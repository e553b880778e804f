# SPDX-License-Identifier: Apache-2.0
"""The ticket path of the compression kernel (csrc/block_tickets.h, csrc/kernel_device.h): a launch of fewer workgroups than
blocks, every workgroup compressing block after block.

ASTCENC_AMD_COMPRESS_GRID=N forces it with min(N, blocks) workgroups, =0 switches it off; the variable is read once per
process, so every case that sets it runs in a child process (one child per value, shared by the cases: CHILDREN).  The expected
bytes are those of the same library in a launch of one workgroup per block -- this process, without the variable, for the
launches of fewer blocks than the device holds workgroups (the 204-block images, the block list), the child with =0 for the
larger ones (the image set, 1024^2) -- and, where the reference can compress the image, the reference library's.

The main image is 100x70 at 6x6: 17 x 12 = 204 blocks with a partial last column and row, 204 = 25 * 8 + 4, so four blocks
take the identity tail of the XCD remap.  Its content is block-sized tiles of the nine classes of the library's self-check of
run-time builds (constant, two-colour, noise of several amplitudes, grey, smooth), so a workgroup meets blocks of every kind
after every other: a constant block leaves the previous block's search state behind, a noisy one runs every trial.  Caps 24, 8
and 1: with one workgroup the blocks run strictly one after the other, all eight heads drained by the same wave, and every
block has another predecessor than under cap 24."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import images

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5


def tiles(w, h, block=(6, 6), seed=5):
    """Block-sized tiles of nine content classes (the classes of jit_self_check, csrc/backend_hip.hip)."""
    bsx, bsy = block
    y, x = np.mgrid[0:h, 0:w]
    tile = (x // bsx + 3 * (y // bsy) + y // (3 * bsy)) % 9
    noise = np.random.default_rng(seed).integers(0, 256, size=(h, w, 4))

    def tri(v):
        m = v & 511
        return np.where(m < 256, m, 511 - m)
    grey = (3 * tri(x + 2 * y) + tri((3 * x + 512 - y) >> 1)) // 4 + noise[..., 0] % 21 - 10
    img = np.zeros((h, w, 4), dtype=np.int64)
    for ch in range(4):
        n = noise[..., ch]
        v = (x * (3 + ch) + y * (7 - ch)) & 255                                                          # 0: ramps
        v = np.where(tile == 1, v + (n & 15) - 6, v)                                                     # light noise
        v = np.where(tile == 2, v + (n & 63) - 24, v)                                                    # noise, alpha too
        v = np.where(tile == 3, n, v)                                                                    # pure noise
        v = np.where(tile == 4, np.where(((x + ch) ^ (y >> 1)) & 2, 220 - 20 * ch, 30 + 25 * ch), v)     # two colours
        v = np.where(tile == 5, 40 + 50 * ch, v)                                                         # constant
        v = np.where((tile == 6) | (tile == 7), grey if ch < 3 else 192 + tri((x >> 1) + (y >> 2)) // 4 + n % 7 - 3, v)
        v = np.where(tile == 8, tri(x * (2 + ch) + y * (5 - ch)), v)                                     # smooth
        if ch == 3:
            v = np.where((tile != 3) & (tile != 2) & (tile != 7), 255, v)
        img[..., ch] = np.clip(v, 0, 255)
    return img.astype(np.uint8)


def transparent_tiles():
    """The main image with two fully transparent patches of 3 x 3 tiles: with an alpha-scale radius their inner blocks are out of
    reach of visible content and become constant zero without being read (load_transparent_block), between searched blocks."""
    img = tiles(100, 70)
    img[18:36, 12:30, 3] = 0
    img[42:60, 54:72, 3] = 0
    return img


def hdr_tiles():
    return (tiles(100, 70).astype(np.float32) * (4.0 / 255.0)).astype(np.float16)


def set_radius(cfg):
    cfg.a_scale_radius = 2


def make_context(product, A, profile, block, quality, flags=0):
    err, cfg = product.config_init(profile, block[0], block[1], 1, quality, flags)
    assert err == 0
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0, product.error_string(err)
    return ctx


def device_stream(product, A, ctx, image, block):
    """The whole image through astcenc_amd_compress_image_device (one launch over all blocks)."""
    import torch
    h, w = image.shape[:2]
    n = -(-w // block[0]) * -(-h // block[1])
    t_image = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    out = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    err = product.lib.astcenc_amd_compress_image_device(ctx, t_image.data_ptr(), w, h, 0, C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                        A.torch_stream(), None)
    assert err == 0, product.error_string(err)
    return out.cpu().numpy()


STALE_LIST = np.array([3, 200, 204, 0xFFFFFFFF, 17, 5, 5, 0x80000000] + list(range(100, 141)), dtype=np.uint32)     # 204 = the image's blocks
SET_SIZES = [(544, 544), (100, 70), (12, 12)]      # 8281 + 204 + 4 blocks: one full group of 8 x 1024 runs and a tail


def job_list(product, A):
    import torch
    ctx = make_context(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        whole = torch.full((64 + 204 * 16 + 64,), FILL, dtype=torch.uint8, device="cuda")
        t_image = torch.from_numpy(tiles(100, 70)).cuda()
        t_list = torch.from_numpy(STALE_LIST.view(np.int32)).cuda()
        err = product.compress_block_list_device(ctx, t_image, t_list, whole[64:64 + 204 * 16])
        assert err == 0, product.error_string(err)
        return whole.cpu().numpy()
    finally:
        product.context_free(ctx)


def job_set(product, A):
    import torch
    ctx = make_context(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        entries = []
        for i, (w, h) in enumerate(SET_SIZES):
            t_image = torch.from_numpy(tiles(w, h, seed=5 + i)).cuda()
            entries.append((t_image, torch.zeros(-(-w // 6) * -(-h // 6) * 16, dtype=torch.uint8, device="cuda")))
        err = product.compress_images_device(ctx, entries)
        assert err == 0, product.error_string(err)
        torch.cuda.synchronize()
        return np.concatenate([blocks.cpu().numpy() for _, blocks in entries])
    finally:
        product.context_free(ctx)


def job_big(product, A):
    ctx = make_context(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        return device_stream(product, A, ctx, A.synthetic_image(1024, 1024), (6, 6))
    finally:
        product.context_free(ctx)


def job_twice(product, A):
    """Two ticket launches of one context, so of one set of heads: the second one's stream (the heads are zeroed per launch)."""
    ctx = make_context(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    try:
        device_stream(product, A, ctx, tiles(100, 70, seed=9), (6, 6))
        return device_stream(product, A, ctx, tiles(100, 70), (6, 6))
    finally:
        product.context_free(ctx)


class Log:
    """The library's diagnostics lines while the block runs."""
    def __init__(self, product):
        self.product, self.lines = product, []
        self.cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: self.lines.append(m.decode()))

    def __enter__(self):
        self.product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
        self.product.lib.astcenc_amd_set_log_callback(C.cast(self.cb, C.c_void_p))
        return self

    def __exit__(self, *exc):
        self.product.lib.astcenc_amd_set_log_callback(None)

    def resident(self):
        """The resident grids the library reported: a launch of more blocks than that draws them from tickets."""
        found = [re.search(r"(\d+) workgroups resident", line) for line in self.lines]
        return [int(m.group(1)) for m in found if m]


def job_jit(product, A):
    got = product.compress(tiles(100, 70), (6, 6), A.PRE_THOROUGH, specialize=True)
    from jit_builds import is_jit
    assert is_jit(product.last_kernel), product.last_kernel
    return got


def job_kernel(kernel, *args, **kwargs):
    """product.compress(*args) with the build that ran asserted by name."""
    def run(product, A):
        got = product.compress(*[a(A) if callable(a) else a for a in args], **{k: v(A) if callable(v) and k != "tweak" else v for k, v in kwargs.items()})
        assert product.last_kernel == kernel, product.last_kernel
        return got
    return run


JOBS = {
    "main": job_kernel("astc_compress_blocks_ldr_6x6m", tiles(100, 70), (6, 6), lambda A: A.PRE_MEDIUM),
    "generic": job_kernel("astc_compress_blocks_ldr64", tiles(100, 70), (6, 6), lambda A: A.PRE_MEDIUM),
    "tiny": job_kernel("astc_compress_blocks_ldr_6x6m", tiles(12, 12), (6, 6), lambda A: A.PRE_MEDIUM),
    "8x8_thorough": job_kernel("astc_compress_blocks_ldr_8x8t", tiles(100, 70, (8, 8)), (8, 8), lambda A: A.PRE_THOROUGH),
    "hdr_6x6_medium": job_kernel("astc_compress_blocks_hdr_6x6m", hdr_tiles(), (6, 6), lambda A: A.PRE_MEDIUM, profile=lambda A: A.PRF_HDR),
    "10x10": job_kernel("astc_compress_blocks_ldr", tiles(100, 70, (10, 10)), (10, 10), lambda A: A.PRE_MEDIUM),
    "alpha_scale": job_kernel("astc_compress_blocks_ldr64", transparent_tiles(), (6, 6), lambda A: A.PRE_MEDIUM, flags=lambda A: A.FLG_USE_ALPHA_WEIGHT,
                              tweak=set_radius),
    "jit": job_jit,
    "list": job_list,
    "set": job_set,
    "big": job_big,
    "twice": job_twice,
}

# child name: (environment, jobs)
CHILDREN = {
    "cap24": ({"ASTCENC_AMD_COMPRESS_GRID": "24"}, ["main", "tiny", "8x8_thorough", "hdr_6x6_medium", "10x10", "alpha_scale"]),
    "cap8": ({"ASTCENC_AMD_COMPRESS_GRID": "8"}, ["main", "list", "twice"]),
    "cap1": ({"ASTCENC_AMD_COMPRESS_GRID": "1"}, ["main"]),
    "cap204": ({"ASTCENC_AMD_COMPRESS_GRID": "204"}, ["main"]),                      # n == N
    "cap64": ({"ASTCENC_AMD_COMPRESS_GRID": "64"}, ["set"]),
    "cap24_generic": ({"ASTCENC_AMD_COMPRESS_GRID": "24", "ASTCENC_AMD_KERNEL": "generic"}, ["generic"]),
    "cap24_jit": ({"ASTCENC_AMD_COMPRESS_GRID": "24", "ASTCENC_AMD_JIT": "sync"}, ["jit"]),
    "off": ({"ASTCENC_AMD_COMPRESS_GRID": "0"}, ["big", "set"]),
}


def child_main(names, path):
    """(child process) the jobs `names` through the product library, their streams into the .npz at `path`."""
    import torch
    import astcenc_amd as A
    torch.zeros(1, device="cuda:0")
    product = A.Library(A.LIB_PRODUCT)
    np.savez(path, **{name: JOBS[name](product, A) for name in names})


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """child(name): the streams of CHILDREN[name], the process run on first use."""
    done = {}
    tmp = tmp_path_factory.mktemp("persistent_grid")

    def get(name, more_env=None):
        if name not in done:
            env, names = CHILDREN[name]
            path = str(tmp / (name + ".npz"))
            script = "import sys; sys.path[:0] = %r; import test_persistent_grid as T; T.child_main(%r, %r)" % (
                [os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")], names, path)
            out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=dict(os.environ, **env, **(more_env or {})), timeout=600)
            assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
            done[name] = dict(np.load(path))
        return done[name]
    return get


@pytest.fixture(scope="module")
def here(product, A):
    """here(job): the job's stream in this process, computed once.  No variable is set: a launch of no more blocks than the device
    holds workgroups (every job but "set" and "big") is one workgroup per block, a larger one draws from tickets."""
    done = {}

    def get(name):
        if name not in done:
            done[name] = JOBS[name](product, A)
        return done[name]
    return get


def same(got, want, what):
    bad = images.mismatches(want, got)
    assert len(bad) == 0, (what, "%d blocks differ" % len(bad), bad[:8])


@pytest.mark.parametrize("cap", ["cap24", "cap8", "cap1", "cap204"])
def test_main_image(child, here, ref, A, cap):
    want = here("main")
    same(ref.compress(tiles(100, 70), (6, 6), A.PRE_MEDIUM), want, "this process against the reference")
    same(child(cap)["main"], want, cap)


def test_fewer_blocks_than_heads(child, here, ref, A):
    want = here("tiny")
    assert want.size == 4 * 16
    same(ref.compress(tiles(12, 12), (6, 6), A.PRE_MEDIUM), want, "this process against the reference")
    same(child("cap24")["tiny"], want, "2 x 2 blocks")


def reference_stream(ref, A, name):
    if name == "8x8_thorough":
        return ref.compress(tiles(100, 70, (8, 8)), (8, 8), A.PRE_THOROUGH)
    if name == "hdr_6x6_medium":
        return ref.compress(hdr_tiles(), (6, 6), A.PRE_MEDIUM, profile=A.PRF_HDR)
    if name == "10x10":
        return ref.compress(tiles(100, 70, (10, 10)), (10, 10), A.PRE_MEDIUM)
    return ref.compress(transparent_tiles(), (6, 6), A.PRE_MEDIUM, flags=A.FLG_USE_ALPHA_WEIGHT, tweak=set_radius)


@pytest.mark.parametrize("name", ["8x8_thorough", "hdr_6x6_medium", "10x10", "alpha_scale"])
def test_other_builds(child, here, ref, A, name):
    want = here(name)
    same(reference_stream(ref, A, name), want, "this process against the reference")
    same(child("cap24")[name], want, name)
    if name == "alpha_scale":
        # (the case is about load_transparent_block: the inner blocks of the patches are the constant zero block)
        zero = ref.compress(np.zeros((6, 6, 4), dtype=np.uint8), (6, 6), A.PRE_MEDIUM)
        blocks = want.reshape(-1, 16)
        assert (blocks == zero.reshape(1, 16)).all(axis=1).sum() >= 2
        assert (blocks[4 * 17 + 3] == zero).all() and (blocks[8 * 17 + 10] == zero).all()


def test_generic_build(child, here):
    same(child("cap24_generic")["generic"], here("main"), "ASTCENC_AMD_KERNEL=generic")


def test_run_time_build(child, ref, A, tmp_path):
    from jit_builds import prewarm
    cache = str(tmp_path / "cache")
    prewarm(cache, [(A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0)])          # (compiled on the CPU, found in the cache)
    got = child("cap24_jit", {"ASTCENC_AMD_CACHE_DIR": cache})["jit"]      # (the child asserts the kernel's name)
    same(got, ref.compress(tiles(100, 70), (6, 6), A.PRE_THOROUGH), "run-time build")


def test_block_list_with_a_stale_index(child, here):
    want = here("list")
    listed = np.unique(STALE_LIST[STALE_LIST < 204]).astype(np.int64)
    blocks = want[64:64 + 204 * 16].reshape(204, 16)
    expect = np.full((204, 16), FILL, dtype=np.uint8)
    expect[listed] = here("main").reshape(204, 16)[listed]
    assert (blocks == expect).all() and (want[:64] == FILL).all() and (want[-64:] == FILL).all()
    assert np.array_equal(child("cap8")["list"], want)


def test_image_set(child, here, ref, A):
    """8489 blocks in one launch: the expected bytes are those of one workgroup per block (=0), every entry of them checked
    against the reference; 64 workgroups, and this process with the device's resident grid, draw the same."""
    want = child("off")["set"]
    assert want.size == (8281 + 204 + 4) * 16
    at = 0
    for i, (w, h) in enumerate(SET_SIZES):
        n = -(-w // 6) * -(-h // 6) * 16
        same(want[at:at + n], ref.compress(tiles(w, h, seed=5 + i), (6, 6), A.PRE_MEDIUM), "entry %d without tickets against the reference" % i)
        at += n
    same(child("cap64")["set"], want, "image set, 64 workgroups")
    same(here("set"), want, "image set, default grid")


def test_heads_are_zeroed_per_launch(child, here):
    same(child("cap8")["twice"], here("main"), "second ticket launch of a context")


def test_default_path_takes_tickets(child, here, product, A):
    """1024^2 at 6x6 is 29 241 blocks, more than the device holds workgroups: this process draws them from tickets, the child
    (=0) does not, and the bytes are the same.  The library reports the resident grid it found to the diagnostics callback."""
    with Log(product) as log:
        got = job_big(product, A)
    print("resident grids reported:", log.resident(), log.lines)
    assert len(log.resident()) == 1 and 0 < log.resident()[0] < 29241, log.lines
    same(got, child("off")["big"], "1024^2, default against ASTCENC_AMD_COMPRESS_GRID=0")


def test_chunked_host_path(product, A):
    """A smooth 3080^2 host image through astcenc_compress_image is 264 196 blocks, two launches of the chunk loop (510 block
    rows of 514, then the last four); the device path compresses it in one.  Both report a resident grid smaller than their
    first launch."""
    img = images.smooth(3080, 3080)
    ctx = make_context(product, A, A.PRF_LDR, (6, 6), A.PRE_MEDIUM)
    with Log(product) as log:
        try:
            want = device_stream(product, A, ctx, img, (6, 6))
        finally:
            product.context_free(ctx)
        assert want.size == 264196 * 16
        got = product.compress(img, (6, 6), A.PRE_MEDIUM)
    print("resident grids reported:", log.resident())
    assert len(log.resident()) >= 2 and all(0 < r < 510 * 514 for r in log.resident()), log.lines
    same(got, want, "host path against device path")
