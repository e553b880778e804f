# SPDX-License-Identifier: Apache-2.0
"""The adaptive driver over an image set with a block budget (astcenc_amd_compress_images_adaptive_device;
csrc/astcenc_adaptive.cpp, backend_adaptive_set_refine).

Expected bytes and records are composed in numpy, as in tests/test_adaptive.py, from the set calls that already exist: B0 / B1 =
astcenc_amd_compress_images_device with the base / strong context, E0 / E1 = the records astcenc_amd_compare_image_set_device
gives for them (entry swizzle = the decode swizzle), S = the selection model of tests/test_block_select_set.py on E0.  Block g
of the output is B1[g] if g is in S and e(E1[g]) < e(E0[g]), else B0[g]; the record is the matching one.  Everything is compared
for equality: the bytes of every entry, the bits of the records, the four counts.  The threshold is the median of the positive
e(E0) / n over the set.  Outputs and records lie between guard bytes filled with 0xA5."""
import ctypes as C

import numpy as np
import pytest

import images
import mip_model
from test_adaptive import OTHER, weighted
from test_adaptive import adaptive as adaptive_single
from test_block_select import texels
from test_block_select_set import NONE, model

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA5
RGBA_W = (1.0, 1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def contexts(product, A):
    made = {}

    def get(block, quality, profile=None, flags=0):
        profile = A.PRF_LDR if profile is None else profile
        key = (tuple(block), quality, profile, flags)
        if key not in made:
            err, cfg = product.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, quality, flags)
            assert err == 0
            err, ctx = product.context_alloc(cfg, 1)
            assert err == 0, product.error_string(err)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


def dims_of(image):
    return (image.shape[-2], image.shape[-3], image.shape[0] if image.ndim == 4 else 1)


def guarded(counts, per_block):
    import torch
    return [torch.full((GUARD + c * per_block + GUARD,), FILL, dtype=torch.uint8, device="cuda") for c in counts]


class SetComposition:
    """B0, B1, E0, E1 of a set and two contexts, and what the driver must make of them for a criterion and a budget."""

    def __init__(self, product, A, base, strong, imgs, block, swz=None, decode_swz=None):
        import torch
        self.product, self.A, self.base, self.strong = product, A, base, strong
        self.swz = A.SWZ_RGBA if swz is None else swz
        self.decode_swz = A.SWZ_RGBA if decode_swz is None else decode_swz
        self.t_images = [torch.from_numpy(np.ascontiguousarray(i)).cuda() for i in imgs]
        bl = tuple(block) + (1,) * (3 - len(block))
        per_entry = [texels(bl, dims_of(i)) for i in imgs]
        self.counts = [p.size for p in per_entry]
        self.n = np.concatenate(per_entry)
        self.blocks = self.n.size
        self.b0, self.e0 = self.stream_and_records(base)
        self.b1, self.e1 = self.stream_and_records(strong)

    def records_of(self, ctx, streams):
        import torch
        records = torch.zeros(self.blocks * 4, dtype=torch.float64, device="cuda")
        err, _ = self.product.compare_image_set_device(ctx, [(t, s, self.decode_swz) for t, s in zip(self.t_images, streams)], block_errors=records)
        assert err == 0, self.product.error_string(err)
        return records.cpu().numpy().reshape(self.blocks, 4)

    def stream_and_records(self, ctx):
        import torch
        outs = [torch.zeros(c * 16, dtype=torch.uint8, device="cuda") for c in self.counts]
        err = self.product.compress_images_device(ctx, [(t, o, self.swz) for t, o in zip(self.t_images, outs)])
        assert err == 0, self.product.error_string(err)
        return np.concatenate([o.cpu().numpy() for o in outs]).reshape(self.blocks, 16), self.records_of(ctx, outs)

    def median_threshold(self, weight=RGBA_W):
        per_texel = weighted(self.e0, weight) / self.n
        return float(np.median(per_texel[per_texel > 0]))

    def expect(self, weight, threshold, max_blocks):
        chosen, candidates = model(self.e0, self.n, weight, threshold, max_blocks)
        selected = np.zeros(self.blocks, dtype=bool)
        selected[chosen] = True
        with np.errstate(all="ignore"):
            replaced = selected & (weighted(self.e1, weight) < weighted(self.e0, weight))
        return candidates, selected, replaced, np.where(replaced[:, None], self.b1, self.b0), np.where(replaced[:, None], self.e1, self.e0)

    def run(self, weight, threshold, max_blocks, with_records=True, stream=None, t_images=None):
        """The call under test into guarded buffers: (error, stats, bytes [blocks, 16], records or None, guards intact)."""
        import torch
        whole = guarded(self.counts, 16)
        whole_r = torch.full((GUARD + self.blocks * 32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        records = whole_r[GUARD:GUARD + self.blocks * 32].view(torch.float64) if with_records else None
        entries = [(t, w[GUARD:GUARD + c * 16], self.swz) for t, w, c in zip(t_images or self.t_images, whole, self.counts)]
        err, stats = self.product.compress_images_adaptive_device(self.base, self.strong, entries, self.A.block_criterion(threshold, weight), max_blocks,
                                                                  self.decode_swz, records, stream)
        if stream is not None:
            stream.synchronize()
        hs, r = [w.cpu().numpy() for w in whole], whole_r.cpu().numpy()
        intact = all((h[:GUARD] == FILL).all() and (h[GUARD + c * 16:] == FILL).all() for h, c in zip(hs, self.counts))
        intact = intact and (r[:GUARD] == FILL).all() and (r[GUARD + self.blocks * 32:] == FILL).all() and (with_records or (r == FILL).all())
        got = np.concatenate([h[GUARD:GUARD + c * 16] for h, c in zip(hs, self.counts)]).reshape(self.blocks, 16)
        return err, stats, got, r[GUARD:GUARD + self.blocks * 32].view(np.float64).reshape(self.blocks, 4) if with_records else None, intact

    def check(self, weight=RGBA_W, threshold=None, max_blocks=NONE, what="", stream=None):
        import torch
        threshold = self.median_threshold(weight) if threshold is None else threshold
        candidates, selected, replaced, want_bytes, want_records = self.expect(weight, threshold, max_blocks)
        print(what, "blocks", self.blocks, "candidates", candidates, "budget", max_blocks, "selected", int(selected.sum()), "replaced", int(replaced.sum()))
        for with_records in (True, False):
            err, stats, got, records, intact = self.run(weight, threshold, max_blocks, with_records, stream)
            assert err == 0, (what, self.product.error_string(err))
            assert intact, (what, "guards")
            assert (stats.blocks, stats.candidates, stats.selected, stats.replaced) == (self.blocks, candidates, int(selected.sum()), int(replaced.sum())), (what, with_records)
            bad = np.flatnonzero((got != want_bytes).any(axis=1))
            assert bad.size == 0, (what, "global blocks that differ", bad[:16])
            if with_records:
                assert np.array_equal(records.view(np.uint64), want_records.view(np.uint64)), (what, "records")
                # ... which are bit for bit those of the set scoring call on the final streams
                first = np.cumsum([0] + self.counts)
                finals = [torch.from_numpy(got[first[i]:first[i + 1]].reshape(-1).copy()).cuda() for i in range(len(self.counts))]
                assert np.array_equal(self.records_of(self.strong, finals).view(np.uint64), records.view(np.uint64)), (what, "records of the final streams")
            assert stats.kernel_ms_base > 0.0 and stats.kernel_ms_other > 0.0 and (stats.kernel_ms_strong > 0.0) == (stats.selected > 0), (what, "times")
        return candidates, selected, replaced


def chain_levels():
    return [np.ascontiguousarray(level) for level in mip_model.chain(images.flat_regions(50, 45))]


@pytest.fixture(scope="module")
def chain_6x6(product, A, contexts):
    """6x6 on the chain of the 50x45 flat_regions image, base -fastest, strong -thorough: computed once, read by several tests."""
    return SetComposition(product, A, contexts((6, 6), A.PRE_FASTEST), contexts((6, 6), A.PRE_THOROUGH), chain_levels(), (6, 6))


def test_chain_with_budgets(chain_6x6):
    c = chain_6x6
    assert c.counts == [72, 20, 4, 1, 1, 1]
    candidates, selected, replaced = c.check(what="chain, no budget")
    # (not vacuous: these depend on what the two presets do to this image)
    assert candidates >= 4 and replaced.sum() >= 1 and selected.sum() == candidates
    for budget in (candidates // 2, 1, 0):
        cand, selected, replaced = c.check(max_blocks=budget, what="chain, budget %d" % budget)
        assert cand == candidates and selected.sum() == budget
    # at least one candidate stays outside the budget of c // 2, and some block of the budgeted run is replaced
    _, selected, replaced = c.check(max_blocks=candidates // 2, what="chain, half")
    assert selected.sum() < candidates and replaced.sum() >= 1


def test_threshold_inf_launches_no_strong_pass(chain_6x6):
    candidates, selected, replaced = chain_6x6.check(threshold=float("inf"), what="threshold +inf")
    assert candidates == 0 and selected.sum() == 0


def test_channel_weights_with_a_budget(chain_6x6):
    chain_6x6.check(weight=(0.0, 0.0, 0.0, 1.0), max_blocks=7, what="alpha only, 7")
    chain_6x6.check(weight=(2.0, 0.5, 0.25, 0.0), max_blocks=7, what="rgb uneven, 7")


def test_unrelated_images_and_slices(product, A, contexts):
    imgs = [images.noisy(31, 17), OTHER["6x6_slices"][2](), images.grayscale(13, 40), images.smooth(6, 6)]
    c = SetComposition(product, A, contexts((6, 6), A.PRE_FASTEST), contexts((6, 6), A.PRE_THOROUGH), imgs, (6, 6))
    candidates, selected, _ = c.check(what="unrelated")
    assert candidates >= 4
    c.check(max_blocks=candidates // 3, what="unrelated, a third")


def test_hdr_f16_set(product, A, contexts):
    imgs = [images.hdr_f16(50, 45).astype(np.float16), images.hdr_f16(20, 9, 3).astype(np.float16)]
    c = SetComposition(product, A, contexts((6, 6), A.PRE_FASTEST, A.PRF_HDR), contexts((6, 6), A.PRE_THOROUGH, A.PRF_HDR), imgs, (6, 6))
    candidates, _, _ = c.check(what="hdr f16")
    c.check(max_blocks=max(candidates // 2, 1), what="hdr f16, half")


def test_bgra_swizzle(product, A, contexts):
    swz = (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A)
    c = SetComposition(product, A, contexts((6, 6), A.PRE_FASTEST), contexts((6, 6), A.PRE_THOROUGH), chain_levels()[:3], (6, 6), swz, swz)
    candidates, _, _ = c.check(what="bgra")
    c.check(max_blocks=candidates // 2, what="bgra, half")


def test_one_entry_without_a_budget_is_the_single_image_driver(product, A, contexts):
    image = images.flat_regions(50, 45)
    c = SetComposition(product, A, contexts((6, 6), A.PRE_FASTEST), contexts((6, 6), A.PRE_THOROUGH), [image], (6, 6))
    threshold = c.median_threshold()
    err, stats, got, records, intact = c.run(RGBA_W, threshold, NONE)
    err1, stats1, got1, records1, intact1 = adaptive_single(product, A, c.base, c.strong, c.t_images[0], c.blocks, RGBA_W, threshold, A.SWZ_RGBA, A.SWZ_RGBA)
    assert err == 0 and err1 == 0 and intact and intact1
    assert np.array_equal(got, got1) and np.array_equal(records.view(np.uint64), records1.view(np.uint64))
    assert (stats.blocks, stats.selected, stats.replaced) == (stats1.blocks, stats1.selected, stats1.replaced) and stats.candidates == stats.selected
    assert stats.replaced >= 1


def test_the_same_context_twice(product, A, contexts):
    ctx = contexts((6, 6), A.PRE_FAST)
    c = SetComposition(product, A, ctx, ctx, chain_levels(), (6, 6))
    candidates, selected, replaced = c.check(max_blocks=9, what="the same context twice")
    assert selected.sum() >= 1 and replaced.sum() == 0
    err, stats, got, _, _ = c.run(RGBA_W, c.median_threshold(), NONE)
    assert err == 0 and stats.replaced == 0 and np.array_equal(got, c.b0)


def test_the_mip_chain_helper(product, A, chain_6x6):
    """compress_mip_chain_adaptive of the binding: generate, one entry per level, the set driver."""
    import torch
    c = chain_6x6
    t_image = torch.from_numpy(images.flat_regions(50, 45)).cuda()
    levels = product.generate_mip_chain_weighted_device(c.base, t_image[None])
    threshold, budget = c.median_threshold(), 11
    records = torch.zeros(c.blocks * 4, dtype=torch.float64, device="cuda")
    tensors, blocks, stats = product.compress_mip_chain_adaptive(c.base, c.strong, t_image[None], A.block_criterion(threshold), budget, block_errors=records)
    assert [tuple(t.shape) for t in tensors] == [tuple(l.shape) for l in levels] and all(torch.equal(a, b) for a, b in zip(tensors, levels))
    outs = [torch.zeros(n * 16, dtype=torch.uint8, device="cuda") for n in c.counts]
    records2 = torch.zeros(c.blocks * 4, dtype=torch.float64, device="cuda")
    err, stats2 = product.compress_images_adaptive_device(c.base, c.strong, list(zip(levels, outs)), A.block_criterion(threshold), budget, block_errors=records2)
    assert err == 0
    assert all(torch.equal(a, b) for a, b in zip(blocks, outs)) and torch.equal(records.view(torch.int64), records2.view(torch.int64))
    assert (stats.blocks, stats.candidates, stats.selected, stats.replaced) == (stats2.blocks, stats2.candidates, stats2.selected, stats2.replaced)
    assert stats.blocks == 99 and stats.selected == budget
    # (the device's levels are the model's, so the composition of the fixture applies too)
    _, _, _, want_bytes, _ = c.expect(RGBA_W, threshold, budget)
    assert np.array_equal(np.concatenate([b.cpu().numpy() for b in blocks]).reshape(-1, 16), want_bytes)


def test_side_stream_with_a_pending_producer(product, A, chain_6x6):
    """Level 0 arrives by a copy queued behind a long kernel on a side stream: work queued on another stream would read noise."""
    import torch
    c = chain_6x6
    image = images.flat_regions(50, 45)
    threshold, budget = c.median_threshold(), 13
    candidates, selected, replaced, want_bytes, want_records = c.expect(RGBA_W, threshold, budget)
    side = torch.cuda.Stream()
    h_img = torch.from_numpy(image).pin_memory()
    d_img = torch.from_numpy(np.random.default_rng(6).integers(0, 256, image.shape, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        d_img.copy_(h_img, non_blocking=True)
        err, stats, got, records, intact = c.run(RGBA_W, threshold, budget, True, side, [d_img] + c.t_images[1:])
    assert err == 0 and intact
    assert (stats.candidates, stats.selected, stats.replaced) == (candidates, int(selected.sum()), int(replaced.sum()))
    assert np.array_equal(got, want_bytes) and np.array_equal(records.view(np.uint64), want_records.view(np.uint64))


def test_mismatched_contexts_and_bad_arguments(product, A, contexts, chain_6x6):
    import torch
    c = chain_6x6
    err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, decompress_only = product.context_alloc(cfg, 1)
    assert err == 0
    whole = guarded(c.counts, 16)
    whole_r = torch.full((GUARD + c.blocks * 32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rec = whole_r.data_ptr() + GUARD
    good, swz, bad_swz = A.block_criterion(0.001), A.Swizzle(*A.SWZ_RGBA), A.Swizzle(0, 1, 2, 9)
    stats = A.AdaptiveSetStats()
    stats.blocks = 77
    L = product.lib

    def entries_of(change=None):
        e = [A.image_set_entry(t, w[GUARD:GUARD + n * 16]) for t, w, n in zip(c.t_images, whole, c.counts)]
        if change:
            change(e)
        return (A.ImageSetEntry * len(e))(*e)

    def call(base=c.base, strong=c.strong, entries=entries_of(), n=len(c.counts), ds=swz, crit=good, budget=NONE, rec=rec, rec_len=c.blocks * 32):
        return L.astcenc_amd_compress_images_adaptive_device(base, strong, entries, n, C.byref(ds) if ds else None, C.byref(crit) if crit else None, budget,
                                                             rec, rec_len, None, C.byref(stats))

    def untouched():
        return stats.blocks == 77 and all((w.cpu().numpy() == FILL).all() for w in whole) and (whole_r.cpu().numpy() == FILL).all()

    try:
        cases = [(contexts((4, 4), A.PRE_THOROUGH), A.ERR_BAD_PARAM, "footprint"), (contexts((6, 5), A.PRE_THOROUGH), A.ERR_BAD_PARAM, "footprint y"),
                 (contexts((6, 6), A.PRE_THOROUGH, A.PRF_LDR_SRGB), A.ERR_BAD_PARAM, "profile"),
                 (contexts((6, 6), A.PRE_THOROUGH, flags=A.FLG_USE_ALPHA_WEIGHT), A.ERR_BAD_PARAM, "flags"), (decompress_only, A.ERR_BAD_CONTEXT, "decompress only")]
        for strong, code, what in cases:
            assert call(strong=strong) == code and call(base=strong, strong=c.base) == code, what
        assert untouched()
    finally:
        product.context_free(decompress_only)

    def short(e):
        e[1].blocks_len = c.counts[1] * 16 - 1

    def null_image(e):
        e[2].image = None

    def null_blocks(e):
        e[5].blocks = None

    def zero_dim(e):
        e[3].dim_y = 0

    def bad_type(e):
        e[4].data_type = 3

    def bad_entry_swizzle(e):
        e[0].swizzle = bad_swz

    assert call(base=None) == A.ERR_BAD_PARAM and call(strong=None) == A.ERR_BAD_PARAM and call(entries=None) == A.ERR_BAD_PARAM
    assert call(ds=None) == A.ERR_BAD_PARAM and call(crit=None) == A.ERR_BAD_PARAM
    assert call(crit=A.block_criterion(float("nan"))) == A.ERR_BAD_PARAM and call(crit=A.block_criterion(0.1, (1, -1, 1, 1))) == A.ERR_BAD_PARAM
    assert call(entries=entries_of(bad_type)) == A.ERR_BAD_PARAM and call(entries=entries_of(zero_dim)) == A.ERR_BAD_PARAM
    assert call(entries=entries_of(bad_entry_swizzle)) == A.ERR_BAD_SWIZZLE and call(ds=bad_swz) == A.ERR_BAD_SWIZZLE
    assert call(entries=entries_of(short)) == A.ERR_OUT_OF_MEM and call(rec_len=c.blocks * 32 - 1) == A.ERR_OUT_OF_MEM
    assert call(entries=entries_of(null_image)) == A.ERR_BAD_CONTEXT and call(entries=entries_of(null_blocks)) == A.ERR_BAD_CONTEXT
    assert untouched()
    # (an empty set succeeds with zeroed stats; the z swizzle is legal for scoring)
    assert call(entries=None, n=0) == A.SUCCESS and stats.blocks == 0
    assert call(ds=A.Swizzle(0, 1, A.SWZ_Z, 3)) == A.SUCCESS and stats.blocks == c.blocks
