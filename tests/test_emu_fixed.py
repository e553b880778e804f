# SPDX-License-Identifier: Apache-2.0
"""The kernel source compiled for ONE context on the CPU (oracle/emu/Makefile `fixed`): what a fixed-context
build of the library and every run-time build (csrc/kernel_jit.cpp) are on the device -- LdsLayout, DeviceConfig and TableRoot
as compile-time constants, the ASTC_FIXED-only code paths (the unrolled mode scoring, for_texels_of_quarter, the literal
channel weights) compiled in -- as a sequential build, against the reference's bytes.  The records are the ones the plain
sequential build writes for the context (ASTC_EMU_DUMP_RECORDS: the text a run-time build is compiled with).

One footprint of at most 64 texels (the BASELINE headline context) and one above (10x8: the footprint whose run-time build
on the device needs the texel count kept out of the constants, wave_ctx.h), then one case per class the ASTC_FIXED-only source
branches on (CLASSES below).

What this module cannot see: the WV_DEVICE-only callers of the fixed paths (wv_sum4_texels, wave_weights.h), the 64-lane
texel loops with a 16-lane last trip (80, 144 texels), ASTC_FIXED_OPAQUE_TEXEL_COUNT (never defined by g++) and anything
the device compiler does with the constants.  Those are what tests/test_jit_matrix.py runs on the GPU."""
import concurrent.futures
import os
import subprocess

import numpy as np
import pytest

import images
import oracle_libs as O  # (path set up by conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "oracle", "emu")


@pytest.mark.parametrize("block,quality,profile_name", [((6, 6), 60.0, "PRF_LDR"), ((10, 8), 10.0, "PRF_LDR_SRGB")])
def test_sequential_build_compiled_for_one_context(built, emu, ref, A, tmp_path, monkeypatch, block, quality, profile_name):
    profile = getattr(A, profile_name)
    name = "%dx%d_%d_%s" % (block[0], block[1], int(quality), profile_name.lower())
    records = str(tmp_path / (name + ".inc"))
    monkeypatch.setenv("ASTC_EMU_DUMP_RECORDS", records)
    img = images.noisy(66, 50, 21)
    plain = emu.compress(img, block, quality, profile=profile)
    monkeypatch.delenv("ASTC_EMU_DUMP_RECORDS")
    text = open(records).read()
    assert "constexpr LdsLayout kFixedLayout" in text and "constexpr TableRoot kFixedRoot" in text
    r = subprocess.run(["make", "-s", "fixed", "NAME=" + name, "RECORDS=" + records], cwd=EMU_DIR, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lib_path = os.path.join(EMU_DIR, "_build", "libastcenc_emu_fixed_%s.so" % name)
    try:
        fixed = A.Library(lib_path)
        want = ref.compress(img, block, quality, profile=profile)
        got = fixed.compress(img, block, quality, profile=profile)
        assert np.array_equal(want, plain)
        assert np.array_equal(want, got), int((want.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1).sum())
        # ... and like a fixed-context kernel build it turns every other context away
        err, cfg = fixed.config_init(profile, block[0], block[1], 1, A.PRE_THOROUGH, 0)
        assert err == 0
        err, ctx = fixed.context_alloc(cfg, 1)
        assert err != 0
    finally:
        os.remove(lib_path)


# One case per class of footprint / record the ASTC_FIXED-only source branches on:
#   (name, block, quality, profile, flags, swizzle, tweak, content)
# T % 4 = 1, 2, 0 below and above 64 texels, odd counts above 64 (for_texels_of_quarter's masked tail, wave_ctx.h; the kLast
# clamp of the unrolled mode scoring, wave_block.h), 40 texels (two planes: the last count with kTrips <= 9, unrolled by
# two -- 36, the case above, is the neighbour on the same side, 48 the first on the other), literal channel weights that are
# not all one (cw_of / cw4_of), a volume through the HDR coders.  The content is chosen so that blocks reach those paths --
# for_texels_of_quarter runs for blocks of two to four partitions (wave_ideal.h) and the one-plane fast path of
# wave_batch.h, which plain noise rarely takes on the larger footprints: regions of two and three colours with noise.
_NORMAL = ("SWZ_R", "SWZ_R", "SWZ_R", "SWZ_G")
CLASSES = [
    ("5x5_m", (5, 5), 60.0, "PRF_LDR", 0, None, None, "regions"),                                    # 25 texels, T % 4 = 1
    ("6x5_m_cw", (6, 5), 60.0, "PRF_LDR", 0, None, {"cw_g_weight": 0.5, "cw_b_weight": 0.25, "cw_a_weight": 0.0}, "regions"),   # 30, T % 4 = 2
    ("8x5_t", (8, 5), 98.0, "PRF_LDR", 0, None, None, "regions"),                                    # 40: kTrips = 10 | two planes
    ("10x5_m_normal", (10, 5), 60.0, "PRF_LDR", "FLG_MAP_NORMAL", _NORMAL, None, "regions"),         # 50, T % 4 = 2
    ("12x12_f", (12, 12), 10.0, "PRF_LDR", 0, None, None, "regions"),                                # 144
    ("5x4x4_m_hdr", (5, 4, 4), 60.0, "PRF_HDR", 0, None, None, "regions_hdr_3d"),                    # 80, 3D, HDR coders
    ("5x5x5_m", (5, 5, 5), 60.0, "PRF_LDR", 0, None, None, "regions_3d"),                            # 125, T % 4 = 1
    ("6x5x5_m", (6, 5, 5), 60.0, "PRF_LDR", 0, None, None, "regions_3d"),                            # 150, T % 4 = 2
]


# SENSITIVITY -- measured on a scratch copy of the source with one defect planted in ASTC_FIXED-only code (CPU only, never
# committed): blocks that change, noise image + regions image, of the blocks of each.
#   A  for_texels_of_quarter: tail mask weakened to `i > kT`        B  mode scoring: kLast one too small
#   C  for_texels_of_quarter: tail mask one too strong (`i >= kT - 1`)   D  for_texels_of_quarter: tail mask removed
#   case (blocks per image)    A          B        C          D
#   5x5_m          (140)    139 + 140   9 + 3   53 + 50   139 + 140
#   6x5_m_cw       (110)      1 + 0     2 + 0   37 + 40     1 + 0
#   8x5_t           (90)      -         5 + 0     -          -        (- : T % 4 = 0, the tail mask is compiled out)
#   10x5_m_normal   (70)     70 + 63    0 + 0   19 + 8     70 + 63
#   12x12_f         (30)      -         0 + 1     -          -
#   5x4x4_m_hdr     (75)      -         2 + 2     -          -
#   5x5x5_m         (60)      0 + 0     4 + 0   13 + 3      0 + 0
#   6x5x5_m         (48)      0 + 0     4 + 0    5 + 2      0 + 0
# A and D make the sums read one to three values past the texel arrays; at 30, 125 and 150 texels that moved (next to) nothing
# on any content tried -- what lies there evidently adds nothing -- so those cases rest on B and C.  Every case is moved by at
# least one planted defect.


def regions(w, h, seed=5):
    """Two- and three-colour regions with noise of a few levels, their borders at angles to the block grid: blocks that pick
    two to four partitions, next to single-partition noisy ones (the right-hand quarter is images.noisy)."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    which = ((x * 2 + y * 3) // 11 + (x - y) // 9) % 3
    palette = np.array([[225, 35, 30, 255], [25, 60, 235, 120], [40, 215, 90, 255]])
    img = palette[which] + rng.integers(-7, 8, size=(h, w, 4))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[:, w - w // 4:] = images.noisy(w, h, 21)[:, w - w // 4:]
    return img


def regions_3d(w, h, d, seed=5):
    """The same as a volume: the region borders move from slice to slice, so a block's partitions cut it in all three axes."""
    return np.stack([np.roll(regions(w, h, seed + (z & 1)), 2 * z, axis=1) for z in range(d)])


def content(kind):
    """The images of a case: noise (single-partition blocks of every mode) and regions (blocks of two to four partitions)."""
    if kind == "regions":
        return [images.noisy(66, 50, 21), regions(66, 50)]
    if kind == "regions_3d":
        return [np.stack([images.noisy(22, 18, 40 + z) for z in range(11)]), regions_3d(22, 18, 11)]
    if kind == "regions_hdr_3d":
        hdr = list(images.hdr_variants(22, 18).values())[0].astype(np.float16)
        vol = regions_3d(22, 18, 11).astype(np.float32) / np.float32(255.0)
        vol[..., :3] *= np.where(vol[..., 3:] < 0.75, np.float32(6.0), np.float32(0.5))      # one colour of the three well above 1.0
        return [np.stack([np.roll(hdr, 3 * z, axis=0) for z in range(11)]), vol.astype(np.float16)]
    raise KeyError(kind)


def case_args(A, case):
    """The keyword arguments of Library.compress for a case of CLASSES."""
    from jit_builds import apply_tweak
    _, block, quality, profile, flags, swizzle, tweak, _ = case
    return dict(block=block, quality=quality, profile=getattr(A, profile), flags=getattr(A, flags) if flags else 0,
                swizzle=tuple(getattr(A, s) for s in swizzle) if swizzle else A.SWZ_RGBA, tweak=apply_tweak(tweak))


def build_fixed(emu, A, cases, records_dir, emu_dir=EMU_DIR, jobs=16):
    """The sequential build compiled for each of `cases`: records dumped by the plain build one after the other (the switch
    is an environment variable), then the compiles side by side.  Returns {name: library path}; raises on a failed compile."""
    old = os.environ.get("ASTC_EMU_DUMP_RECORDS")
    recs = {}
    try:
        for case in cases:
            recs[case[0]] = os.path.join(str(records_dir), case[0] + ".inc")
            os.environ["ASTC_EMU_DUMP_RECORDS"] = recs[case[0]]
            kw = case_args(A, case)
            tiny = np.zeros((1, 1, 1, 4) if len(case[1]) > 2 else (1, 1, 4), dtype=np.float16 if case[3] == "PRF_HDR" else np.uint8)
            emu.compress(tiny, **kw)
    finally:
        if old is None:
            os.environ.pop("ASTC_EMU_DUMP_RECORDS", None)
        else:
            os.environ["ASTC_EMU_DUMP_RECORDS"] = old

    def make(name):
        return subprocess.run(["make", "-s", "fixed", "NAME=cls_" + name, "RECORDS=" + recs[name]], cwd=emu_dir, capture_output=True, text=True, timeout=900)
    workers = max(1, min(jobs, len(cases), len(os.sched_getaffinity(0))))
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        results = list(pool.map(make, [c[0] for c in cases]))
    for case, r in zip(cases, results):
        assert r.returncode == 0, (case[0], r.stderr[-3000:])
    return {c[0]: os.path.join(emu_dir, "_build", "libastcenc_emu_fixed_cls_%s.so" % c[0]) for c in cases}


@pytest.fixture(scope="module")
def class_builds(built, emu, A, tmp_path_factory):
    libs = build_fixed(emu, A, CLASSES, tmp_path_factory.mktemp("records"))
    yield libs
    for path in libs.values():
        if os.path.exists(path):
            os.remove(path)


@pytest.mark.parametrize("case", CLASSES, ids=[c[0] for c in CLASSES])
def test_sequential_build_of_each_fixed_only_class(class_builds, emu, ref, A, case):
    """g++ never defines ASTC_FIXED_OPAQUE_TEXEL_COUNT, so these builds have the literal texel count everywhere -- also above
    64 texels, where a run-time build on the device reads it through a register: what is checked
    here is the source for the class, not what the device compiler makes of it.

    How many blocks of this content a defect planted in the ASTC_FIXED-only code changes: SENSITIVITY above."""
    kw = case_args(A, case)
    fixed = A.Library(class_builds[case[0]])
    for img in content(case[7]):
        want = ref.compress(img, **kw)
        plain = emu.compress(img, **kw)
        got = fixed.compress(img, **kw)
        assert np.array_equal(want, plain), int((want.reshape(-1, 16) != plain.reshape(-1, 16)).any(axis=1).sum())
        assert np.array_equal(want, got), int((want.reshape(-1, 16) != got.reshape(-1, 16)).any(axis=1).sum())
