# SPDX-License-Identifier: Apache-2.0
"""Run-time specialised builds of the compression kernel (csrc/kernel_jit.cpp): a context none of
the library's three fixed-context builds serves gets a build of its own -- the library's embedded device source compiled by
hipRTC with the context's LdsLayout / DeviceConfig / TableRoot as constants, cached on disk.

CPU: the embedded source compiles for a context's records (hipRTC needs no device; the sequential build of the library
     drives the same kernel_jit.cpp), the code object has no scratch frame, the disk cache is hit the second time.
GPU: contexts of other presets / footprints / profiles / flags launch "astc_compress_blocks_jit_<hash>" and produce the
     reference's bytes; the default (lazy) mode starts on the generic build and switches; a sweep of footprints x presets x
     profiles through the run-time builds matches the reference.  (The builds of the sweep are compiled side by side on the
     box's CPUs through the sequential library -- same source, same records, same hash -- and found in the cache.)"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from jit_builds import compress_both as _compress_both, prewarm as _prewarm, specialize_on_cpu as _specialize_on_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_embedded_source_compiles_and_is_cached(built, emu, A, tmp_path, monkeypatch):
    if not os.path.exists("/opt/rocm/lib/libhiprtc.so"):
        pytest.skip("no hipRTC on this box")
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    t0 = time.time()
    (name,) = _prewarm(cache, [(A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0)])
    first = time.time() - t0
    files = os.listdir(cache)
    assert files == [name[len("astc_compress_blocks_jit_"):] + ".hsaco"], files
    if os.path.exists(READELF):
        notes = subprocess.run([READELF, "--notes", os.path.join(cache, files[0])], capture_output=True, text=True).stdout
        assert ".name:           astc_compress_blocks_jit" in notes
        assert ".private_segment_fixed_size: 0" in notes and ".vgpr_spill_count: 0" in notes, notes[-1500:]
    # the second context with the same records: from the disk, same name; another flag: another build
    t0 = time.time()
    rc, again = _specialize_on_cpu((cache, A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0))
    assert rc == 0 and again == name and time.time() - t0 < max(2.0, first / 3)
    rc, other = _specialize_on_cpu((cache, A.PRF_LDR, (6, 6), A.PRE_THOROUGH, A.FLG_USE_PERCEPTUAL))
    assert rc == 0 and other != name and len(os.listdir(cache)) == 2


@pytest.mark.gpu
def test_other_contexts_get_a_run_time_build(product, ref, A, tmp_path, monkeypatch):
    """The four contexts VERDICT r05 names, a hand-edited tuning field, an HDR one: specialised, and the reference's bytes."""
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    img = A.synthetic_image(250, 190, 3)

    two_partitions = {"tune_partition_count_limit": 2}
    cases = [(A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0, None), (A.PRF_LDR, (4, 4), A.PRE_MEDIUM, 0, None), (A.PRF_LDR_SRGB, (6, 6), A.PRE_MEDIUM, 0, None),
             (A.PRF_LDR, (6, 6), A.PRE_MEDIUM, A.FLG_USE_PERCEPTUAL, None), (A.PRF_LDR, (6, 6), A.PRE_MEDIUM, 0, two_partitions)]
    _prewarm(cache, [c if c[4] else c[:4] for c in cases])
    names = set()
    for profile, block, quality, flags, tweak in cases:
        bad, name = _compress_both(product, ref, A, img, block, quality, profile, flags, tweak)
        assert name.startswith("astc_compress_blocks_jit_"), name
        assert bad == 0, (profile, block, quality, flags, bad)
        names.add(name)
    assert len(names) == len(cases)
    hdr = A.synthetic_hdr_image(120, 90, 3)
    bad, name = _compress_both(product, ref, A, hdr, (8, 8), A.PRE_MEDIUM, A.PRF_HDR)
    assert name.startswith("astc_compress_blocks_jit_") and bad == 0
    # the BASELINE contexts keep the builds the library ships
    bad, name = _compress_both(product, ref, A, img, (6, 6), A.PRE_MEDIUM, A.PRF_LDR)
    assert name == "astc_compress_blocks_ldr_6x6m" and bad == 0


@pytest.mark.gpu
def test_lazy_mode_starts_generic_and_switches(product, ref, A, tmp_path, monkeypatch):
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "lazy")
    img = np.ascontiguousarray(A.synthetic_image(250, 190, 5))
    err, cfg = product.config_init(A.PRF_LDR, 5, 5, 1, A.PRE_FAST, 0)
    assert err == 0
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        name = lambda: product.lib.astcenc_amd_context_kernel_name(ctx).decode()
        assert name() == "astc_compress_blocks_ldr64" and not os.path.exists(cache)      # nothing compiled for a thumbnail
        out0 = np.zeros(50 * 38 * 16, dtype=np.uint8)
        assert product.compress_raw(ctx, img, out0) == 0 and name() == "astc_compress_blocks_ldr64"
        assert product.lib.astcenc_amd_context_specialize(ctx) == 0
        assert name().startswith("astc_compress_blocks_jit_") and len(os.listdir(cache)) == 1
        out1 = np.zeros_like(out0)
        assert product.lib.astcenc_compress_reset(ctx) == 0
        assert product.compress_raw(ctx, img, out1) == 0
        assert np.array_equal(out0, out1)
    finally:
        product.context_free(ctx)
    # a second context with the same records finds the build on disk: specialised from its first launch
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        assert product.lib.astcenc_amd_context_kernel_name(ctx).decode().startswith("astc_compress_blocks_jit_")
    finally:
        product.context_free(ctx)
    want = ref.compress(img, (5, 5), A.PRE_FAST)
    assert np.array_equal(want, out1)
    # ... and "off" keeps the generic build whatever the cache holds
    monkeypatch.setenv("ASTCENC_AMD_JIT", "off")
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        assert product.lib.astcenc_amd_context_kernel_name(ctx).decode() == "astc_compress_blocks_ldr64"
        assert product.lib.astcenc_amd_context_specialize(ctx) == A.ERR_NOT_IMPLEMENTED
    finally:
        product.context_free(ctx)


@pytest.mark.gpu
def test_sweep_through_run_time_builds(product, ref, A, tmp_path, monkeypatch):
    """Footprints (2D up to 12x12, 3D) x presets x profiles: every context on its own run-time build, bytes = the reference's."""
    import images
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    contexts = []
    for block in ((4, 4), (5, 5), (6, 6), (8, 6), (8, 8), (10, 10), (12, 12)):
        for quality in (A.PRE_FASTEST, A.PRE_FAST, A.PRE_MEDIUM, A.PRE_THOROUGH):
            for profile in (A.PRF_LDR, A.PRF_LDR_SRGB):
                if (profile, block, quality) not in ((A.PRF_LDR, (6, 6), A.PRE_MEDIUM), (A.PRF_LDR, (8, 8), A.PRE_THOROUGH)):
                    contexts.append((profile, block, quality, 0))
        contexts.append((A.PRF_HDR_RGB_LDR_A, block, A.PRE_MEDIUM, 0))
    contexts += [(A.PRF_LDR, (3, 3, 3), A.PRE_MEDIUM, 0), (A.PRF_LDR, (4, 4, 4), A.PRE_FAST, 0), (A.PRF_HDR, (6, 6, 6), A.PRE_FAST, 0)]
    # (a build the library refuses -- more than 128 VGPRs, a scratch frame beyond a few bytes: kernel_jit.cpp -- leaves its
    #  context on the generic kernel; that is allowed to happen to a few contexts, not to most)
    names = _prewarm(cache, contexts, strict=False)
    built = [n for n in names if n]
    assert len(set(built)) == len(built) and len(built) >= 0.8 * len(contexts), names
    noisy, rnd = images.noisy(120, 113, 21), images.random_u8(115, 120, 22)
    hdr = list(images.hdr_variants(96, 90).values())[0].astype(np.float16)
    vol = np.stack([images.noisy(40, 36, 40 + z) for z in range(12)])
    vol_hdr = np.stack([hdr[:36, :40] for _ in range(12)])
    bad = []
    for (profile, block, quality, flags), name in zip(contexts, names):
        if len(block) == 3:
            imgs = [vol_hdr if profile == A.PRF_HDR else vol]
        else:
            imgs = [hdr] if profile == A.PRF_HDR_RGB_LDR_A else [noisy, rnd]
        for img in imgs:
            n, used = _compress_both(product, ref, A, img, block, quality, profile, flags, specialize="try")
            assert used == name or (name is None and not used.startswith("astc_compress_blocks_jit_")), (used, name)
            if n:
                bad.append((profile, block, quality, n))
    assert not bad, bad


@pytest.mark.gpu
def test_background_compile_takes_over_by_itself(product, ref, A, tmp_path, monkeypatch):
    """The default mode end to end: the context starts on the generic build, queues its compile once it has compressed enough
    (the count lowered for the test), keeps compressing on the generic build while the compiler process works, and a later
    call finds the build, verifies it and launches it -- same bytes before and after."""
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    monkeypatch.setenv("ASTCENC_AMD_JIT", "lazy")
    monkeypatch.setenv("ASTCENC_AMD_JIT_LAZY_BLOCKS", "3000")
    img = np.ascontiguousarray(A.synthetic_image(250, 190, 8))
    err, cfg = product.config_init(A.PRF_LDR, 8, 6, 1, A.PRE_FAST, 0)
    assert err == 0
    err, ctx = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        name = lambda: product.lib.astcenc_amd_context_kernel_name(ctx).decode()
        first = np.zeros(32 * 32 * 16, dtype=np.uint8)
        assert product.compress_raw(ctx, img, first) == 0 and name() == "astc_compress_blocks_ldr64"
        deadline = time.time() + 120
        calls = 1
        out = np.zeros_like(first)
        while not name().startswith("astc_compress_blocks_jit_") and time.time() < deadline:
            assert product.lib.astcenc_compress_reset(ctx) == 0
            assert product.compress_raw(ctx, img, out) == 0
            assert np.array_equal(first, out)
            calls += 1
            time.sleep(0.05)
        assert name().startswith("astc_compress_blocks_jit_"), "no run-time build after %d calls" % calls
        assert calls >= 3                                   # (1024 blocks per call: the compile was not even queued before the third)
        assert product.lib.astcenc_compress_reset(ctx) == 0
        assert product.compress_raw(ctx, img, out) == 0 and np.array_equal(first, out)
    finally:
        product.context_free(ctx)
    assert np.array_equal(ref.compress(img, (8, 6), A.PRE_FAST), first)


ORPHAN_SCRIPT = r"""
import sys, os, time, threading
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_libs as O, astcenc_amd as A
lib = A.Library(O.LIB_EMU)
err, cfg = lib.config_init(A.PRF_LDR, 5, 4, 1, A.PRE_FAST, 0); assert err == 0
err, ctx = lib.context_alloc(cfg, 1); assert err == 0
threading.Thread(target=lambda: lib.lib.astcenc_amd_context_specialize(ctx), daemon=True).start()
cache = os.environ["ASTCENC_AMD_CACHE_DIR"]
deadline = time.time() + 30
while time.time() < deadline and not (os.path.isdir(cache) and any(f.startswith("jit") for f in os.listdir(cache))):
    time.sleep(0.05)                  # (until the compiler process has its scratch directory: it is at work now)
time.sleep(0.3)
print("leaving", sorted(os.listdir(cache)))
sys.exit(0)
"""


def test_a_host_that_exits_does_not_wait_and_the_build_is_there_next_time(built, emu, A, tmp_path):
    """A compile in flight when the host process exits: the process leaves at once (it neither waits for the compiler
    process nor kills it), the compiler process finishes on its own, writes the build into the disk cache and removes its
    scratch directory -- the next run of the host finds the build."""
    if not os.path.exists("/opt/rocm/lib/libhiprtc.so"):
        pytest.skip("no hipRTC on this box")
    cache = tmp_path / "cache"
    env = dict(os.environ, ASTCENC_AMD_CACHE_DIR=str(cache), ASTCENC_AMD_JIT="lazy")
    script = ORPHAN_SCRIPT % (os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "leaving ['jit" in r.stdout and ".hsaco" not in r.stdout, r.stdout        # only the scratch directory so far
    # the host is gone (and its pipes are closed: subprocess.run has returned) while the compile is still running
    assert not [f for f in os.listdir(cache) if f.endswith(".hsaco")], "the host waited for its compile"
    deadline = time.time() + 60
    while time.time() < deadline and not [f for f in os.listdir(cache) if f.endswith(".hsaco")]:
        time.sleep(0.5)
    time.sleep(0.5)
    assert [f for f in os.listdir(cache) if f.endswith(".hsaco")], os.listdir(cache)
    assert not [f for f in os.listdir(cache) if f.startswith("jit")], os.listdir(cache)   # the scratch directory is gone
    rc, name = _specialize_on_cpu((str(cache), A.PRF_LDR, (5, 4), A.PRE_FAST, 0))       # ... and the next run starts with the build
    assert rc == 0 and name[len("astc_compress_blocks_jit_"):] + ".hsaco" in os.listdir(cache)
