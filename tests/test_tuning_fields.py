# SPDX-License-Identifier: Apache-2.0
"""Hand-set tuning fields (tests/tuning_cases.py) on the HIP builds of the compression kernel, byte for byte against the
reference (oracle/_ref).  tests/test_tuning_fields_cpu.py shows from reference bytes that the cases bite.

(a) the generic builds (the session's ASTCENC_AMD_JIT=off): every case and combination, with the kernel that ran asserted per
    case -- ldr64, ldr, hdr64, hdr and the 3D footprints are all among them.
(b) the three fixed-context builds (csrc/fixed_contexts.inc) step aside: each of their contexts with one field changed reports
    the generic kernel and gives the reference's bytes.  (The sequential library names no builds, so this is checked here only.)
(c) run-time builds: sixteen contexts compiled side by side on the CPUs as tests/test_jit_matrix.py does; each runs its own
    build, gives the reference's bytes, and no two of them share a kernel name -- the cache key sees every field.
(d) the other entry points of a context -- host pointer, device pointer, image set, block list -- give the same bytes."""
import ctypes as C
import time

import numpy as np
import pytest

import tuning_cases as T
from jit_builds import apply_tweak, compress_both, is_jit, prewarm

pytestmark = pytest.mark.gpu

import astcenc_amd as A  # noqa: E402  (path set up by conftest.py)

FIXED = T.FIXED_KERNELS


@pytest.fixture(scope="module")
def want(ref):
    return T.Outputs(ref)


def _run(product, want, ctx, image_name):
    """(blocks that differ from the reference's, the kernel that ran) of one 36-block image on the context's generic build."""
    got = T.compress(product, ctx, T.image(image_name, ctx[1]))
    return T.differing(want.want(ctx, image_name), got), product.last_kernel


# ---- (a) ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field", T.FIELDS)
def test_generic_builds_match_the_reference(product, want, field):
    bad = []
    for c in T.cases_of(field):
        ctx = T.context_of(c)
        n, used = _run(product, want, ctx, c.image)
        assert used == T.expected_kernel(c), (T.case_id(c), used)
        if n:
            bad.append((T.case_id(c), n))
    assert not bad, bad


def _groups():
    return [(profile, block, q) for profile, block, _ in T.COMBO_FOOTPRINTS for q in T.COMBO_PRESETS]


def _group_id(g):
    return "%s%s-q%g" % ("hdr" if g[0] == A.PRF_HDR else "ldr", "x".join(map(str, g[1])), g[2])


@pytest.mark.parametrize("group", _groups(), ids=_group_id)
def test_generic_builds_match_the_reference_on_combinations(product, want, group):
    bad = []
    for c in [c for c in T.combos() if (c.profile, c.block, c.quality) == group]:
        n, used = _run(product, want, c[:5], c.image)
        assert used == T.generic_kernel(c.profile, c.block), (T.combo_id(c), used)
        assert T.build_class(c.profile, c.block, c.quality, c.tweak) == c.build_class, T.combo_id(c)
        if n:
            bad.append((T.combo_id(c), n))
    assert not bad, bad


def test_every_generic_class_is_among_the_contexts():
    """What (a) asserts per case, summed up: the four generic builds and the 3D footprints on both of theirs."""
    seen = set()
    for ctx in [T.context_of(c) for c in T.cases() if c.kind != "inert"] + [c[:5] for c in T.combos()]:
        seen.add((T.build_class(ctx[0], ctx[1], ctx[2], ctx[4]), T.generic_kernel(ctx[0], ctx[1])))
    assert seen == {("ldr64", T.K + "ldr64"), ("ldr", T.K + "ldr"), ("hdr64", T.K + "hdr64"), ("hdr", T.K + "hdr"), ("3d", T.K + "ldr")}, seen


# ---- (b) ------------------------------------------------------------------------------------------------------------------

def _kernel_name(lib, ctx):
    profile, block, quality, flags, tweak = ctx
    err, cfg = lib.config_init(profile, block[0], block[1], 1, quality, flags)
    assert err == 0
    preset = cfg.as_dict()
    for f, v in tweak.items():
        setattr(cfg, f, v)
    err, handle = lib.context_alloc(cfg, 1)
    assert err == 0
    try:
        return lib.lib.astcenc_amd_context_kernel_name(handle).decode(), preset, cfg.as_dict()
    finally:
        lib.context_free(handle)


def other_value(field, preset_value):
    """An in-range value of the table that is not the preset's: the lower end of the range unless the preset holds it."""
    values = [v for v, k in T.VALUES[field] if k in ("lo", "side", "hi", "mid") and np.float32(v) != np.float32(preset_value)]
    return values[0]


@pytest.mark.parametrize("field", T.FIELDS)
def test_fixed_builds_step_aside_for_a_changed_field(product, want, field):
    for base, fixed in FIXED.items():
        profile, block, quality, flags = T.BASES[base]
        name, preset, _ = _kernel_name(product, (profile, block, quality, flags, {}))
        assert name == fixed, (base, name)
        if T.inert(field, base):
            continue          # (context_alloc overwrites it: no record changes, the fixed build is the right one)
        # (validate_config raises the preset's rgbm_m_scale of 0 to 1: a 1 there would be no change)
        value = other_value(field, max(preset[field], 1.0) if field == "rgbm_m_scale" else preset[field])
        ctx = (profile, block, quality, flags, {field: value})
        name, _, _ = _kernel_name(product, ctx)
        assert name == T.generic_kernel(profile, block), (field, value, base, name)
        image_name = T.image_of(field, "hdr6x6" if base == "hdr6x6" else "ldr6x6", value)
        n, used = _run(product, want, ctx, image_name)
        assert used == name and n == 0, (field, value, base, used, n)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
JIT_6X6 = [(A.PRF_LDR, (6, 6), A.PRE_MEDIUM, 0, T.corner_tweak(cand, parts, 1024, modes))
           for cand in (1, 8) for parts in (1, 4) for modes in (1, 100)]
JIT_10X8_CASES = [("tune_refinement_limit", 9), ("tune_2partitioning_candidate_limit", 8), ("tune_db_limit", 0.0), ("tune_mse_overshoot", 1.0),
                  ("tune_2partition_early_out_limit_factor", 0.0), ("tune_3partition_early_out_limit_factor", T.INF),
                  ("tune_2plane_early_out_limit_correlation", 0.0), ("tune_search_mode0_enable", 0.84)]


def _jit_cases():
    out = []
    for field, value in JIT_10X8_CASES:
        out += [c for c in T.cases_of(field) if c.base == "ldr10x8" and c.value == value]
    assert len(out) == len(JIT_10X8_CASES)
    return out


@pytest.fixture(scope="module")
def builds(built, tmp_path_factory):
    cache = str(tmp_path_factory.mktemp("jit_cache_tuning"))
    contexts = JIT_6X6 + [T.context_of(c) for c in _jit_cases()]
    assert len(contexts) <= 16
    t0 = time.time()
    names = prewarm(cache, contexts, strict=False)
    print("prewarm: %d builds in %.1f s" % (len(contexts), time.time() - t0))
    return {"cache": cache, "names": names, "contexts": contexts, "prewarm_s": time.time() - t0}


def test_run_time_builds_match_the_reference(product, ref, builds, monkeypatch):
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", builds["cache"])
    monkeypatch.setenv("ASTCENC_AMD_JIT", "sync")
    monkeypatch.delenv("ASTCENC_AMD_JIT_OPTIONS", raising=False)
    monkeypatch.delenv("ASTCENC_AMD_JIT_SELF_CHECK", raising=False)
    contexts, names = builds["contexts"], builds["names"]
    # (GENERIC_BY_DESIGN of tests/test_jit_matrix.py is empty: the library documents no refusal)
    refused = [ctx for ctx, name in zip(contexts, names) if not is_jit(name)]
    assert not refused, ("builds the library refused", refused)
    assert len(set(names)) == len(names), ("two contexts share a build", sorted(names))
    # corners that differ in one field only: candidates, partitions or the mode limit
    for i, a in enumerate(JIT_6X6):
        for j, b in enumerate(JIT_6X6[:i]):
            if sum(1 for f in a[4] if a[4][f] != b[4][f]) == 1:
                assert names[i] != names[j], (a[4], b[4], names[i])
    image_names = ["patches4"] * len(JIT_6X6) + [c.image for c in _jit_cases()]
    t0 = time.time()
    bad = []
    for ctx, name, image_name in zip(contexts, names, image_names):
        profile, block, quality, flags, tweak = ctx
        n, used = compress_both(product, ref, A, T.image(image_name, block), block, quality, profile, flags=flags, tweak=apply_tweak(tweak),
                                specialize=True)
        print("%-150s %s" % (ctx, used))
        assert is_jit(used) and used == name, (ctx, used, name)
        if n:
            bad.append((ctx, n))
    print("(c): %d contexts in %.1f s after the prewarm of %.1f s" % (len(contexts), time.time() - t0, builds["prewarm_s"]))
    assert not bad, bad


# ---- (d) ------------------------------------------------------------------------------------------------------------------
ENTRY_CONTEXTS = [(A.PRF_LDR, block, A.PRE_THOROUGH, 0, T.corner_tweak(*corner))
                  for block in ((6, 6), (12, 12)) for corner in ((8, 4, 1024, 100), (1, 1, 1, 1))]


@pytest.mark.parametrize("ctx", ENTRY_CONTEXTS, ids=lambda c: "%dx%d-c%d" % (c[1][0], c[1][1], c[4]["tune_candidate_limit"]))
def test_every_entry_point_of_a_context(product, want, ctx):
    import torch
    profile, block, quality, flags, tweak = ctx
    img = T.image("patches4", block)
    expect = want.want(ctx, "patches4")
    err, cfg = product.config_init(profile, block[0], block[1], 1, quality, flags)
    assert err == 0
    T.apply(tweak)(cfg)
    err, handle = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        assert product.lib.astcenc_amd_context_kernel_name(handle).decode() == T.generic_kernel(profile, block)
        outs = {}
        host = np.zeros(36 * 16, dtype=np.uint8)
        assert product.compress_raw(handle, np.ascontiguousarray(img), host) == 0
        outs["host pointer"] = host
        t_img = torch.from_numpy(np.array(img)).cuda()
        swz = A.Swizzle(*A.SWZ_RGBA)

        def fresh():
            return torch.full((36 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
        out = fresh()
        err = product.lib.astcenc_amd_compress_image_device(handle, t_img.data_ptr(), img.shape[1], img.shape[0], A.TYPE_U8, C.byref(swz),
                                                            out.data_ptr(), out.numel(), A.torch_stream(), None)
        assert err == 0, product.error_string(err)
        outs["device pointer"] = out.cpu().numpy()
        out = fresh()
        err = product.compress_images_device(handle, [(t_img, out)])
        assert err == 0, product.error_string(err)
        outs["image set"] = out.cpu().numpy()
        out = fresh()
        every = torch.arange(36, dtype=torch.int32, device="cuda")
        err = product.compress_block_list_device(handle, t_img, every, out)
        assert err == 0, product.error_string(err)
        outs["block list"] = out.cpu().numpy()
    finally:
        product.context_free(handle)
    bad = {name: T.differing(expect, got) for name, got in outs.items() if T.differing(expect, got)}
    assert not bad, bad
