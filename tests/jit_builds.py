# SPDX-License-Identifier: Apache-2.0
"""Shared by the tests that launch run-time builds of the compression kernel (csrc/kernel_jit.cpp): tests/test_jit.py,
tests/test_jit_matrix.py, tests/test_image_set*.py.  Not a conftest: a plain module, imported by name.

The builds of a test are compiled side by side on the CPUs through the sequential library -- same source, same records,
same hash; the workers never open the GPU -- and the GPU process then finds them in the disk cache.

A context is (profile, block, quality, flags) or (profile, block, quality, flags, tweak); a tweak is a dict of hand-edited
astcenc_config fields, {"tune_partition_count_limit": 2} (a dict, not a function: it travels to a worker process)."""
import concurrent.futures
import multiprocessing
import os
import sys

import oracle_libs as O  # (path set up by conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JIT_PREFIX = "astc_compress_blocks_jit_"
MAX_WORKERS = 16


def apply_tweak(tweak):
    """The function Library.compress(tweak=...) wants, of a tweak dict (None: none)."""
    if not tweak:
        return None

    def edit(cfg):
        for field, value in tweak.items():
            assert hasattr(cfg, field), field
            setattr(cfg, field, value)
    return edit


def is_jit(name):
    return bool(name) and name.startswith(JIT_PREFIX)


def specialize_on_cpu(args):
    """Worker process: compile the context's run-time build through the sequential library into the shared cache."""
    cache, profile, block, quality, flags = args[:5]
    tweak = args[5] if len(args) > 5 else None
    os.environ["ASTCENC_AMD_CACHE_DIR"] = cache
    sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
    import astcenc_amd as A
    lib = A.Library(O.LIB_EMU)
    bz = block[2] if len(block) > 2 else 1
    err, cfg = lib.config_init(profile, block[0], block[1], bz, quality, flags)
    assert err == 0
    if tweak:
        apply_tweak(tweak)(cfg)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    rc = lib.lib.astcenc_amd_context_specialize(ctx)
    name = lib.lib.astcenc_amd_context_kernel_name(ctx).decode()
    lib.context_free(ctx)
    return rc, name


def pool_size(jobs):
    """Processes for `jobs` compiles: the affinity mask of a shared machine may show far more CPUs than a command may use."""
    return max(1, min(jobs, MAX_WORKERS, len(os.sched_getaffinity(0))))


def prewarm(cache, contexts, strict=True):
    """Compiles the run-time builds of `contexts` into `cache`; the kernel names, None for a build the library refuses
    (strict: none may be refused)."""
    # (fresh interpreters: the parent may hold a HIP runtime, which does not survive a fork)
    with concurrent.futures.ProcessPoolExecutor(max_workers=pool_size(len(contexts)), mp_context=multiprocessing.get_context("spawn")) as pool:
        results = list(pool.map(specialize_on_cpu, [(cache,) + tuple(c) for c in contexts]))
    if strict:
        assert all(rc == 0 and is_jit(name) for rc, name in results), list(zip(contexts, results))
    return [name if rc == 0 else None for rc, name in results]


def compress_both(product, ref, A, img, block, quality, profile, flags=0, tweak=None, specialize=True, swizzle=None):
    """(blocks that differ from the reference's, the kernel that ran) of one image through the product's context.  tweak: a
    function of the config (as Library.compress takes it) or a tweak dict."""
    if isinstance(tweak, dict):
        tweak = apply_tweak(tweak)
    swizzle = A.SWZ_RGBA if swizzle is None else swizzle
    want = ref.compress(img, block, quality, profile=profile, flags=flags, tweak=tweak, swizzle=swizzle).reshape(-1, 16)
    got = product.compress(img, block, quality, profile=profile, flags=flags, tweak=tweak, swizzle=swizzle, specialize=specialize).reshape(-1, 16)
    return int((want != got).any(axis=1).sum()), product.last_kernel
