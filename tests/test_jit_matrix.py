# SPDX-License-Identifier: Apache-2.0
"""Run-time kernel builds (csrc/kernel_jit.cpp) on everything the generic builds are tested on.

The rest of the GPU suite runs with ASTCENC_AMD_JIT=off (tests/conftest.py), i.e. on the library's generic builds; by default
a user's context runs a build compiled for it, with its records as constants.  This module puts those builds through
  (a) every footprint (14 2D, 10 3D) x preset x profile,
  (b) the per-call input paths the records do not hold (swizzles, f16 / f32 input, texels outside the format's range under LDR
      and HDR -- tests/input_cases.py --, tiny and partial images, thin volumes),
  (c) the records that turn into literals (channel weights, flags, alpha-scale radius, hand-edited search limits),
  (d) several device slots,
  (e) a deliberately wrong build against the self-check that gates every adoption,
byte for byte against the reference (oracle/_ref), and asserts for every case WHICH kernel ran: a case that fell back to the
generic build proves nothing.  When a stream differs, the same context's generic build (ASTCENC_AMD_JIT=off) is run too, to
say whether the difference is the run-time build's or the source's.

The builds are compiled once per session, side by side on the CPUs (tests/jit_builds.py), and found in the cache.

GENERIC_BY_DESIGN lists the contexts the library keeps on the generic build on purpose (none today).  A build the library
refuses (more than 128 VGPRs, a scratch frame) also leaves its context on the generic kernel: allowed for at most a fifth of
the contexts of (a), for none of the -medium contexts of TAIL_FOOTPRINTS in (a), for none of (b), (c), (d)."""
import contextlib
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import images
import input_cases
from jit_builds import apply_tweak, is_jit, prewarm
from test_gpu_parity import FLAGS_AND_SWIZZLES, LIVE, low_m_image
from test_multi_device import _Devices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import astcenc_amd as A  # noqa: E402  (path set up by conftest.py)

FOOTPRINTS_2D = [(4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12)]
FOOTPRINTS_3D = [(3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4), (5, 4, 4), (5, 5, 4), (5, 5, 5), (6, 5, 5), (6, 6, 5), (6, 6, 6)]
PRESETS = [A.PRE_FASTEST, A.PRE_FAST, A.PRE_MEDIUM, A.PRE_THOROUGH]
# the contexts the library ships fixed-context builds for: they keep those
BASELINE = {(A.PRF_LDR, (6, 6), A.PRE_MEDIUM), (A.PRF_LDR, (8, 8), A.PRE_THOROUGH), (A.PRF_HDR, (6, 6), A.PRE_MEDIUM)}
# Contexts kept on the generic build on purpose, as (profile, block, quality, flags): each with its DESIGN.md reference.
GENERIC_BY_DESIGN = set()
# texel counts whose 64-lane texel loops end in a 16-lane trip (80, 144) or whose count is odd / 2 mod 4 above 64 (125, 150)
TAIL_FOOTPRINTS = [(10, 8), (12, 12), (5, 4, 4), (5, 5, 5), (6, 5, 5)]
# one footprint per tail class, for the per-call paths of (b): 20, 30, 64, 50, 80, 144, 80 (3D), 125 texels
PATH_FOOTPRINTS = [(5, 4), (6, 5), (8, 8), (10, 5), (10, 8), (12, 12), (5, 4, 4), (5, 5, 5)]
RECORD_FOOTPRINTS = [(6, 6), (6, 5), (10, 8)]
# ... of which these take the out-of-range content of tests/input_cases.py under the HDR profile as well
HDR_PATH_FOOTPRINTS = [(5, 4), (8, 8), (10, 8)]


def _matrix_contexts():
    out = []
    for block in FOOTPRINTS_2D + FOOTPRINTS_3D:
        for quality in PRESETS:
            out.append((A.PRF_LDR, block, quality, 0))
        out.append((A.PRF_LDR_SRGB, block, A.PRE_MEDIUM, 0))
        if len(block) == 2 or block in ((3, 3, 3), (5, 4, 4), (6, 6, 6)):
            out += [(A.PRF_HDR, block, A.PRE_MEDIUM, 0), (A.PRF_HDR_RGB_LDR_A, block, A.PRE_MEDIUM, 0)]
    return [c for c in out if c[:3] not in BASELINE]


def _record_cases():
    """(c): (context with tweak, swizzle, image name) -- the flag / swizzle list of tests/test_gpu_parity.py, channel weights,
    the alpha-scale radius, search limits, on three footprints at -medium."""
    cases = []
    for block in RECORD_FOOTPRINTS:
        def ctx(flags=0, tweak=None, block=block):
            return (A.PRF_LDR, block, A.PRE_MEDIUM, flags, tweak)
        cases += [(ctx(tweak={"cw_r_weight": 1.0, "cw_g_weight": 0.5, "cw_b_weight": 0.25, "cw_a_weight": 0.0}), A.SWZ_RGBA, "noisy"),
                  (ctx(tweak={"cw_r_weight": 0.3, "cw_g_weight": 1.0, "cw_b_weight": 0.0, "cw_a_weight": 1.0}), A.SWZ_RGBA, "noisy")]
        for flags, swz in FLAGS_AND_SWIZZLES:
            name = {A.FLG_USE_ALPHA_WEIGHT: "alpha", A.FLG_MAP_RGBM: "low_m"}.get(flags, "noisy")
            cases.append((ctx(flags), swz, name))
        for radius in (1, 4):
            cases.append((ctx(A.FLG_USE_ALPHA_WEIGHT, {"a_scale_radius": radius}), A.SWZ_RGBA, "transparent"))
        for field, value in (("tune_partition_count_limit", 2), ("tune_candidate_limit", 1), ("tune_refinement_limit", 1)):
            cases.append((ctx(tweak={field: value}), A.SWZ_RGBA, "two_colour" if "partition" in field else "noisy"))
    # the live cases of tests/test_gpu_parity.py (content classes x footprints x presets, one with a partition limit)
    for block, quality, name, size, plimit in LIVE:
        cases.append(((A.PRF_LDR, block, quality, 0, {"tune_partition_count_limit": plimit} if plimit else None), A.SWZ_RGBA, (name, size)))
    return [c for c in cases if not (c[0][:3] in BASELINE and c[0][3] == 0 and not c[0][4])]


def _key(c):
    tweak = c[4] if len(c) > 4 else None
    return (c[0], tuple(c[1]), float(c[2]), c[3], tuple(sorted(tweak.items())) if tweak else ())


MUTANT_OPTIONS = "-ffp-contract=fast"
MUTANTS = [(A.PRF_LDR, (6, 6), A.PRE_FAST, 0), (A.PRF_LDR, (10, 8), A.PRE_MEDIUM, 0), (A.PRF_LDR, (5, 5, 5), A.PRE_FAST, 0)]


@pytest.fixture(scope="module")
def builds(built, tmp_path_factory):
    """Every build the module launches, compiled into one cache: {key: kernel name or None (refused)}, and the cache."""
    cache = str(tmp_path_factory.mktemp("jit_cache"))
    contexts = {}
    for c in _matrix_contexts() + [case[0] for case in _record_cases()]:
        contexts.setdefault(_key(c), c if len(c) > 4 and c[4] else c[:4])
    t0 = time.time()
    names = prewarm(cache, list(contexts.values()), strict=False)
    # ... and the wrong builds of (e): another option, another cache key
    old = os.environ.get("ASTCENC_AMD_JIT_OPTIONS")
    os.environ["ASTCENC_AMD_JIT_OPTIONS"] = MUTANT_OPTIONS
    try:
        mutants = prewarm(cache, MUTANTS, strict=False)
    finally:
        if old is None:
            del os.environ["ASTCENC_AMD_JIT_OPTIONS"]
        else:
            os.environ["ASTCENC_AMD_JIT_OPTIONS"] = old
    print("prewarm: %d builds (+ %d of (e)) in %.1f s" % (len(contexts), len(MUTANTS), time.time() - t0))
    table = dict(zip(contexts.keys(), names))
    return {"cache": cache, "names": table, "mutants": mutants, "prewarm_s": time.time() - t0}


@pytest.fixture
def jit_sync(builds, monkeypatch):
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", builds["cache"])
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    monkeypatch.delenv("ASTCENC_AMD_JIT_OPTIONS", raising=False)
    monkeypatch.delenv("ASTCENC_AMD_JIT_SELF_CHECK", raising=False)
    return builds


@contextlib.contextmanager
def _jit_off():
    """Contexts allocated inside run the generic build (the mode is read per astcenc_context_alloc)."""
    old = os.environ.get("ASTCENC_AMD_JIT")
    os.environ["ASTCENC_AMD_JIT"] = "off"
    try:
        yield
    finally:
        if old is None:
            del os.environ["ASTCENC_AMD_JIT"]
        else:
            os.environ["ASTCENC_AMD_JIT"] = old


def _differing(a, b):
    return int((a.reshape(-1, 16) != b.reshape(-1, 16)).any(axis=1).sum())


def _run(product, ref, ctx, img, swizzle=A.SWZ_RGBA, specialize=True):
    """One image through the context's run-time build: (blocks differing from the reference, of those: blocks where the generic
    build differs from the reference too, kernel that ran)."""
    profile, block, quality, flags = ctx[:4]
    tweak = apply_tweak(ctx[4] if len(ctx) > 4 else None)
    kw = dict(profile=profile, flags=flags, tweak=tweak, swizzle=swizzle)
    want = ref.compress(img, block, quality, **kw)
    got = product.compress(img, block, quality, specialize=specialize, **kw)
    used = product.last_kernel
    bad, generic_bad = _differing(want, got), 0
    if bad:
        with _jit_off():
            generic_bad = _differing(want, product.compress(img, block, quality, **kw))
    return bad, generic_bad, used


def _matrix_content():
    noisy, rnd = images.noisy(121, 113, 21), images.random_u8(118, 119, 22)            # (no side a multiple of a footprint's)
    hdr = list(images.hdr_variants(97, 89).values())[0].astype(np.float16)
    vol = np.stack([images.noisy(41, 37, 40 + z) for z in range(11)])
    vol_hdr = np.stack([hdr[:37, :41] for _ in range(11)])
    return {"ldr": [noisy, rnd], "hdr": [hdr], "vol": [vol], "vol_hdr": [vol_hdr]}


def _content_of(content, ctx):
    hdr = ctx[0] in (A.PRF_HDR, A.PRF_HDR_RGB_LDR_A)
    if len(ctx[1]) == 3:
        return content["vol_hdr" if hdr else "vol"]
    return content["hdr" if hdr else "ldr"]


def test_every_footprint_preset_and_profile(product, ref, jit_sync):
    """(a) 24 footprints x {fastest, fast, medium, thorough} LDR, sRGB / HDR / HDR-RGB-LDR-A at medium."""
    contexts = _matrix_contexts()
    names = [jit_sync["names"][_key(c)] for c in contexts]
    content = _matrix_content()
    t0 = time.time()
    bad, generic = [], []
    for ctx, name in zip(contexts, names):
        for img in _content_of(content, ctx):
            n, n_generic, used = _run(product, ref, ctx, img, specialize="try")
            print("%-44s %s" % (ctx, used))
            # what the CPU compile delivered is what runs: a build the self-check turns away shows here
            assert used == name or (name is None and not is_jit(used)), (ctx, used, name)
            if n:
                bad.append((ctx, n, "of which the generic build differs too: %d" % n_generic))
        if not is_jit(name):
            generic.append(ctx)
    print("(a): %d contexts, %d on the generic build: %s; %.1f s after the prewarm of %.1f s" %
          (len(contexts), len(generic), generic, time.time() - t0, jit_sync["prewarm_s"]))
    assert not bad, bad
    must = [c for c in contexts if c[1] in TAIL_FOOTPRINTS and c[2] == A.PRE_MEDIUM and c not in GENERIC_BY_DESIGN]
    assert len(must) >= 2 * len(TAIL_FOOTPRINTS)
    assert not [c for c in must if c in generic], [c for c in must if c in generic]
    assert len(generic) <= 0.2 * len(contexts), generic


def _path_images(block):
    """(b): (name, image, swizzle) of the per-call properties the records do not hold."""
    bgr1, rrrg = (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_1), (A.SWZ_R, A.SWZ_R, A.SWZ_R, A.SWZ_G)
    if len(block) == 2:
        u8 = images.noisy(61, 47, 9)
        tiny = [np.ascontiguousarray(u8[:1, :1]), np.ascontiguousarray(u8[:2, :3])]
        partial = np.ascontiguousarray(u8[:2 * block[1] + 1, :3 * block[0] + 1])
        thin = []
    else:
        u8 = np.stack([images.noisy(23, 19, 60 + z) for z in range(9)])
        tiny = [np.ascontiguousarray(u8[:1, :1, :1]), np.ascontiguousarray(u8[:1, :2, :3])]
        partial = np.ascontiguousarray(u8[:block[2] + 1, :2 * block[1] + 1, :3 * block[0] + 1])
        thin = [("fewer slices than the block is deep", np.ascontiguousarray(u8[:block[2] - 2]), A.SWZ_RGBA)]
    wide = u8.astype(np.float32) / np.float32(255.0) * np.float32(1.5) - np.float32(0.25)         # -0.25 .. 1.25
    ba01 = input_cases.SWIZZLES["ba01"]
    spoilt = [("%s %s B,A,0,1" % (cls, dtype), input_cases.content(input_cases.Case(cls, dtype, "ba01"), block), ba01)
              for cls in ("nonfinite", "tiny") for dtype in ("f16", "f32")]                       # (tests/input_cases.py)
    return [("B,G,R,1", u8, bgr1), ("R,R,R,G", u8, rrrg), ("f16", wide.astype(np.float16), A.SWZ_RGBA), ("f32", wide, A.SWZ_RGBA),
            ("f16 swizzled", wide.astype(np.float16), bgr1), ("1x1", tiny[0], A.SWZ_RGBA), ("3x2", tiny[1], A.SWZ_RGBA),
            ("one partial block column and row", partial, A.SWZ_RGBA)] + spoilt + thin


@pytest.mark.parametrize("block", PATH_FOOTPRINTS, ids=lambda b: "x".join(map(str, b)))
def test_per_call_input_paths(product, ref, jit_sync, block):
    """(b) swizzled RGBA8, f16 / f32 with values outside [0, 1], non-finite and subnormal texels, images smaller than a block, a
    partial last column and row, a volume thinner than the block: properties of the call, not of the records -- the self-check
    never sees them."""
    ctx = (A.PRF_LDR, block, A.PRE_MEDIUM, 0)
    assert is_jit(jit_sync["names"][_key(ctx)]), ("refused", ctx)
    bad = []
    for name, img, swz in _path_images(block):
        n, n_generic, used = _run(product, ref, ctx, img, swz)
        print("%-30s %-34s %s" % (ctx, name, used))
        assert is_jit(used), (ctx, name, used)
        if n:
            bad.append((name, n, "generic build: %d" % n_generic))
    assert not bad, (ctx, bad)
    if block in HDR_PATH_FOOTPRINTS:
        _hdr_input_paths(product, ref, jit_sync, block)


def _hdr_input_paths(product, ref, jit_sync, block):
    """... and under the HDR profile, where the loader converts to LNS: values above the largest half, negatives, subnormals,
    NaN and infinities (tests/input_cases.py), as F16 and F32, through the identity and a swizzle with constants."""
    ctx = (A.PRF_HDR, block, A.PRE_MEDIUM, 0)
    assert is_jit(jit_sync["names"][_key(ctx)]), ("refused", ctx)
    bad = []
    for cls in ("huge", "nonfinite"):
        for dtype in ("f16", "f32"):
            for swz in ("rgba", "ba01"):
                name = "%s %s %s" % (cls, dtype, swz)
                n, n_generic, used = _run(product, ref, ctx, input_cases.image(cls, dtype), input_cases.SWIZZLES[swz])
                print("%-30s %-34s %s" % (ctx, name, used))
                assert is_jit(used), (ctx, name, used)
                if n:
                    bad.append((name, n, "generic build: %d" % n_generic))
    assert not bad, (ctx, bad)


def _record_image(name, block):
    if isinstance(name, tuple):
        return images.ALL[name[0]](*name[1])
    w, h = 9 * block[0] + 3, 7 * block[1] + 2
    if name == "low_m":
        return low_m_image(np.random.default_rng(17), (w, h))
    img = images.two_colour(w, h) if name == "two_colour" else images.noisy(w, h, 5)
    if name == "alpha":
        img[..., 3] = np.random.default_rng(3).integers(0, 256, size=img.shape[:2], dtype=np.uint8)
        img[:, : w // 3, 3] = (np.arange(h) * 255 // (h - 1)).astype(np.uint8)[:, None]
    if name == "transparent":
        img[..., 3] = 255
        img[h // 5: h // 5 + block[1] + 2, :, 3] = 0
        img[h // 2: h // 2 + 3 * block[1], : w // 2, 3] = 0
    return img


def test_records_that_turn_into_literals(product, ref, jit_sync):
    """(c) channel weights other than one (cw_of / cw4_of take literals), USE_ALPHA_WEIGHT (where they must not), MAP_NORMAL's
    tiny weights, PERCEPTUAL, RGBM with M near zero, DECODE_UNORM8, the alpha-scale pre-pass, hand-edited search limits."""
    bad = []
    for ctx, swz, name in _record_cases():
        built = jit_sync["names"][_key(ctx)]
        assert is_jit(built), ("refused", ctx)
        n, n_generic, used = _run(product, ref, ctx, _record_image(name, ctx[1]), swz)
        print("%-100s %-12s %s" % (ctx, name if isinstance(name, str) else name[0], used))
        assert used == built, (ctx, used, built)
        if n:
            bad.append((ctx, name, n, "generic build: %d" % n_generic))
    assert not bad, bad


def _reference_threads(ref, img, block, quality, threads):
    """The reference through `threads` host threads of one context (its own API: one call per thread index)."""
    err, cfg = ref.config_init(A.PRF_LDR, block[0], block[1], 1, quality, 0)
    assert err == 0
    err, ctx = ref.context_alloc(cfg, threads)
    assert err == 0
    try:
        h, w = img.shape[:2]
        out = np.zeros(-(-w // block[0]) * -(-h // block[1]) * 16, dtype=np.uint8)
        rcs = [None] * threads
        def work(i):
            rcs[i] = ref.compress_raw(ctx, img, out, thread_index=i)
        ts = [threading.Thread(target=work, args=(i,)) for i in range(threads)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert rcs == [0] * threads, rcs
        return out
    finally:
        ref.context_free(ctx)


def test_every_device_slot_adopts_the_build(product, ref, jit_sync, monkeypatch):
    """(d) three slots on one GPU: slot_adopt_jit loads and self-checks the build per slot; the dealt portions give the one-slot
    stream and the reference's."""
    monkeypatch.setenv("ASTCENC_AMD_DEAL_MIN_BLOCKS", "4096")
    block, quality = (10, 8), A.PRE_MEDIUM
    w, h = 2243, 1805                               # 225 x 226 blocks: three slots need 3 x 16 384
    img = np.ascontiguousarray(A.synthetic_image(w, h, 31))
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        streams = {}
        for devices, slots in (("0", 1), ("0,0,0", 3)):
            with _Devices(devices):
                err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], 1, quality, 0)
                assert err == 0
                err, ctx = product.context_alloc(cfg, 1)
                assert err == 0
            try:
                assert product.lib.astcenc_amd_context_device_count(ctx) == slots
                assert product.lib.astcenc_amd_context_specialize(ctx) == 0
                name = product.lib.astcenc_amd_context_kernel_name(ctx).decode()
                print("%-10s %s" % (devices, name))
                assert name == jit_sync["names"][_key((A.PRF_LDR, block, quality, 0))], name
                out = np.zeros(-(-w // block[0]) * -(-h // block[1]) * 16, dtype=np.uint8)
                assert product.compress_raw(ctx, img, out) == 0
                streams[devices] = out
            finally:
                product.context_free(ctx)
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
    # a slot that cannot load the build, or whose self-check turns it away, says so -- and stays on the generic build
    assert not [line for line in logged if "generic build stays" in line], logged
    assert np.array_equal(streams["0"], streams["0,0,0"]), _differing(streams["0"], streams["0,0,0"])
    want = _reference_threads(ref, img, block, quality, min(16, len(os.sched_getaffinity(0))))
    assert np.array_equal(want, streams["0,0,0"]), _differing(want, streams["0,0,0"])


MUTANT_SCRIPT = r"""
import json, os, sys
sys.path[:0] = [%(tests)r, %(python)r, %(oracle)r]
import numpy as np
import torch
import astcenc_amd as A, oracle_libs as O
import test_jit_matrix as M
ctx = tuple(json.loads(sys.argv[1])); ctx = (ctx[0], tuple(ctx[1]), ctx[2], ctx[3])
torch.zeros(1, device="cuda:0")
product, ref = A.Library(A.LIB_PRODUCT), A.Library(O.LIB_REF_NONE)
content = M._content_of(M._matrix_content(), ctx)
profile, block, quality, flags = ctx
def run(specialize):
    outs = [product.compress(img, block, quality, profile=profile, flags=flags, specialize=specialize) for img in content]
    return outs, product.last_kernel
os.environ["ASTCENC_AMD_JIT"] = "off"
generic, name = run(False)
assert not M.is_jit(name), name
want = [ref.compress(img, block, quality, profile=profile, flags=flags) for img in content]
os.environ["ASTCENC_AMD_JIT"] = "sync"
os.environ["ASTCENC_AMD_JIT_OPTIONS"] = M.MUTANT_OPTIONS
os.environ["ASTCENC_AMD_JIT_SELF_CHECK"] = "0"
unchecked, name_unchecked = run(True)
del os.environ["ASTCENC_AMD_JIT_SELF_CHECK"]
checked, name_checked = run("try")
d = lambda xs, ys: sum(M._differing(x, y) for x, y in zip(xs, ys))
print("RESULT " + json.dumps({"blocks": sum(x.size // 16 for x in want), "generic_vs_reference": d(generic, want),
                              "unchecked_kernel": name_unchecked, "unchecked_vs_generic": d(unchecked, generic),
                              "checked_kernel": name_checked, "checked_vs_reference": d(checked, want)}))
"""


def test_a_wrong_build_is_turned_away_or_harmless(product, ref, jit_sync):
    """(e) the gate: the three contexts compiled with -ffp-contract=fast (a debugging switch; the contract is
    -ffp-contract=off, wave.h).  With the self-check off the build is launched and its blocks are counted against the
    generic build's -- that it IS wrong somewhere is the premise, asserted.  With the self-check on, the build is either
    turned away (the context stays generic) or, if adopted, gives the reference's bytes on the content of (a).  A byte
    mismatch experiment: each context in a process of its own, the smallest first, stopped at the first process that does
    not end normally.  (A process takes 2.5 s on an MI355X box with torch in the page cache, most of it start-up.)"""
    assert all(is_jit(n) for n in jit_sync["mutants"]), jit_sync["mutants"]
    script = MUTANT_SCRIPT % {"tests": os.path.join(ROOT, "tests"), "python": os.path.join(ROOT, "astc-encoder_amd", "python"),
                              "oracle": os.path.join(ROOT, "oracle")}
    env = dict(os.environ, ASTCENC_AMD_CACHE_DIR=jit_sync["cache"])
    results = []
    for ctx, name in zip(MUTANTS, jit_sync["mutants"]):
        t0 = time.time()
        r = subprocess.run([sys.executable, "-c", script, json.dumps(ctx)], env=env, capture_output=True, text=True, timeout=30)
        assert r.returncode == 0, (ctx, r.returncode, r.stderr[-3000:])
        res = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
        print("%-40s %s (%.1f s)" % (ctx, res, time.time() - t0))
        results.append((ctx, name, res))
    for ctx, name, res in results:
        assert res["generic_vs_reference"] == 0, (ctx, res)
        assert res["unchecked_kernel"] == name, (ctx, res, name)                    # (the wrong build did run)
        if is_jit(res["checked_kernel"]):
            assert res["checked_vs_reference"] == 0, ("adopted by the self-check, and wrong", ctx, res)
        else:
            assert res["checked_vs_reference"] == 0, ("turned away, and the generic build is wrong", ctx, res)
    results = [res for _, _, res in results]
    assert sum(r["unchecked_vs_generic"] for r in results) > 0, ("none of the wrong builds differs anywhere: the test cannot fail", results)
