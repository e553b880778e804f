# SPDX-License-Identifier: Apache-2.0
"""The adaptive driver (astcenc_amd_compress_image_adaptive_device; csrc/astcenc_adaptive.cpp, backend_adaptive_refine).

Expected bytes and records are composed in numpy from calls that already exist: B0 / B1 = astcenc_amd_compress_volume_device with
the base / strong context, E0 / E1 = the per-block records of astcenc_amd_compare_blocks_device for them.  Block i of the output
is B1[i] if E0[i] is selected and e(E1[i]) < e(E0[i]), else B0[i]; the record is the matching one; `selected` and `replaced` are
the counts.  Everything is compared for equality: bytes, the bits of the records, the counts.  The threshold is the median of
the positive e(E0) / n of the base stream, computed here, unless a test says otherwise.

The output and the records lie between guard bytes, filled with 0xA5; a rejected call leaves all of it untouched."""
import ctypes as C

import numpy as np
import pytest

import images
from test_block_select import model, texels

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA5


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


def stream_and_records(product, A, ctx, t_image, blocks, swz, decode_swz):
    """(B, E) of one context: the existing full call and the existing scoring call."""
    import torch
    out = torch.zeros(blocks * 16, dtype=torch.uint8, device="cuda")
    args, s = product._image_args(t_image, None)
    err = product.lib.astcenc_amd_compress_volume_device(ctx, *args, C.byref(A.Swizzle(*swz)), out.data_ptr(), out.numel(), s, None)
    assert err == 0, product.error_string(err)
    records = torch.zeros(blocks * 4, dtype=torch.float64, device="cuda")
    err, _ = product.compare_blocks_device(ctx, out, t_image, swizzle=decode_swz, block_errors=records)
    assert err == 0, product.error_string(err)
    return out.cpu().numpy().reshape(blocks, 16), records.cpu().numpy().reshape(blocks, 4)


def weighted(records, weight):
    w = np.asarray(weight, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((w[0] * records[:, 0] + w[1] * records[:, 1]) + w[2] * records[:, 2]) + w[3] * records[:, 3]


def adaptive(product, A, base, strong, t_image, blocks, weight, threshold, swz, decode_swz, with_records=True, stream=None):
    """The call under test into guarded buffers: (error, stats, bytes [blocks, 16], records [blocks, 4] or None, guards intact)."""
    import torch
    whole = torch.full((GUARD + blocks * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    whole_r = torch.full((GUARD + blocks * 32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    records = whole_r[GUARD:GUARD + blocks * 32].view(torch.float64) if with_records else None
    err, stats = product.compress_image_adaptive_device(base, strong, t_image, A.block_criterion(threshold, weight), whole[GUARD:GUARD + blocks * 16],
                                                        swizzle=swz, decode_swizzle=decode_swz, block_errors=records, stream=stream)
    if stream is not None:
        stream.synchronize()
    h, r = whole.cpu().numpy(), whole_r.cpu().numpy()
    intact = (h[:GUARD] == FILL).all() and (h[GUARD + blocks * 16:] == FILL).all() and (r[:GUARD] == FILL).all() and (r[GUARD + blocks * 32:] == FILL).all()
    if not with_records:
        intact = intact and (r == FILL).all()
    return err, stats, h[GUARD:GUARD + blocks * 16].reshape(blocks, 16), r[GUARD:GUARD + blocks * 32].view(np.float64).reshape(blocks, 4) if with_records else None, intact


class Composition:
    """B0, B1, E0, E1 of an image and two contexts, and what the driver must make of them for a criterion."""

    def __init__(self, product, A, base, strong, image, block, swz=None, decode_swz=None):
        import torch
        self.product, self.A, self.base, self.strong = product, A, base, strong
        self.swz = A.SWZ_RGBA if swz is None else swz
        self.decode_swz = A.SWZ_RGBA if decode_swz is None else decode_swz
        self.t_image = torch.from_numpy(np.ascontiguousarray(image)).cuda()
        bl = tuple(block) + (1,) * (3 - len(block))
        self.n = texels(bl, dims_of(image))
        self.blocks = self.n.size
        self.b0, self.e0 = stream_and_records(product, A, base, self.t_image, self.blocks, self.swz, self.decode_swz)
        self.b1, self.e1 = stream_and_records(product, A, strong, self.t_image, self.blocks, self.swz, self.decode_swz)

    def median_threshold(self, weight=(1.0, 1.0, 1.0, 1.0)):
        per_texel = weighted(self.e0, weight) / self.n
        return float(np.median(per_texel[per_texel > 0]))

    def expect(self, weight, threshold):
        selected = model(self.e0, self.n, weight, threshold)
        with np.errstate(all="ignore"):
            replaced = selected & (weighted(self.e1, weight) < weighted(self.e0, weight))
        return selected, replaced, np.where(replaced[:, None], self.b1, self.b0), np.where(replaced[:, None], self.e1, self.e0)

    def check(self, weight=(1.0, 1.0, 1.0, 1.0), threshold=None, what="", stream=None):
        threshold = self.median_threshold(weight) if threshold is None else threshold
        selected, replaced, want_bytes, want_records = self.expect(weight, threshold)
        print(what, "blocks", self.blocks, "selected", int(selected.sum()), "replaced", int(replaced.sum()), "zero error", int((weighted(self.e0, weight) == 0).sum()))
        for with_records in (True, False):
            err, stats, got, records, intact = adaptive(self.product, self.A, self.base, self.strong, self.t_image, self.blocks, weight, threshold,
                                                        self.swz, self.decode_swz, with_records, stream)
            assert err == 0, (what, self.product.error_string(err))
            assert intact, (what, "guards")
            assert (stats.blocks, stats.selected, stats.replaced) == (self.blocks, int(selected.sum()), int(replaced.sum())), (what, with_records)
            bad = np.flatnonzero((got != want_bytes).any(axis=1))
            assert bad.size == 0, (what, "blocks that differ", bad[:16])
            if with_records:
                assert np.array_equal(records.view(np.uint64), want_records.view(np.uint64)), (what, "records")
                # ... which are bit for bit those of the existing call on the final stream
                import torch
                final = torch.zeros(self.blocks * 4, dtype=torch.float64, device="cuda")
                err, _ = self.product.compare_blocks_device(self.strong, torch.from_numpy(got.reshape(-1)).cuda(), self.t_image, swizzle=self.decode_swz, block_errors=final)
                assert err == 0 and np.array_equal(final.cpu().numpy().view(np.uint64).reshape(-1, 4), records.view(np.uint64)), (what, "records of the final stream")
            assert stats.kernel_ms_base > 0.0 and stats.kernel_ms_other > 0.0 and (stats.kernel_ms_strong > 0.0) == (stats.selected > 0), (what, "times")
        return selected, replaced


@pytest.fixture(scope="module")
def flat_6x6(product, A, contexts):
    """6x6 on the 50x45 flat_regions image, base -fastest, strong -thorough: computed once, read by several tests."""
    return Composition(product, A, contexts((6, 6), A.PRE_FASTEST), contexts((6, 6), A.PRE_THOROUGH), images.flat_regions(50, 45), (6, 6))


def test_fastest_then_thorough(flat_6x6):
    selected, replaced = flat_6x6.check(what="6x6 flat -fastest / -thorough")
    assert flat_6x6.blocks == 72
    assert replaced.sum() >= 1 and (~selected).sum() >= 1          # (not vacuous)


def test_roles_reversed_keeps_the_better_blocks(product, A, contexts):
    c = Composition(product, A, contexts((6, 6), A.PRE_THOROUGH), contexts((6, 6), A.PRE_FASTEST), images.flat_regions(50, 45), (6, 6))
    selected, replaced = c.check(what="6x6 flat -thorough / -fastest")
    kept_though_different = selected & ~replaced & (c.b0 != c.b1).any(axis=1)
    assert kept_though_different.sum() >= 1


def test_threshold_inf_and_zero(flat_6x6):
    c = flat_6x6
    selected, replaced = c.check(threshold=float("inf"), what="threshold +inf")
    assert selected.sum() == 0 and replaced.sum() == 0
    selected, _ = c.check(threshold=0.0, what="threshold 0")
    e0 = weighted(c.e0, (1.0, 1.0, 1.0, 1.0))
    assert np.array_equal(selected, e0 > 0) and 1 <= (e0 == 0).sum() < c.blocks


def test_the_same_context_twice(product, A, contexts):
    ctx = contexts((6, 6), A.PRE_FAST)
    c = Composition(product, A, ctx, ctx, images.flat_regions(50, 45), (6, 6))
    selected, replaced = c.check(what="the same context twice")
    assert selected.sum() >= 1 and replaced.sum() == 0
    err, stats, got, _, intact = adaptive(product, A, ctx, ctx, c.t_image, c.blocks, (1.0, 1.0, 1.0, 1.0), c.median_threshold(), A.SWZ_RGBA, A.SWZ_RGBA)
    assert err == 0 and stats.replaced == 0 and np.array_equal(got, c.b0)


def test_channel_weights(flat_6x6):
    """Other weights select and replace other blocks (the driver hands the criterion to both kernels)."""
    flat_6x6.check(weight=(0.0, 0.0, 0.0, 1.0), what="alpha only")
    flat_6x6.check(weight=(2.0, 0.5, 0.25, 0.0), what="rgb, uneven")


OTHER = {
    "bgra": ((6, 6), None, lambda: images.flat_regions(50, 45), "bgra"),
    "4x4": ((4, 4), None, lambda: images.flat_regions(50, 45), None),
    "12x12": ((12, 12), None, lambda: images.noisy(134, 50), None),
    "3x3x3": ((3, 3, 3), None, lambda: images.volume("grad", 5, 7, 10), None),
    "hdr_6x6": ((6, 6), "PRF_HDR", lambda: images.hdr_f16(50, 45).astype(np.float16), None),
    "6x6_slices": ((6, 6), None, lambda: np.stack([images.flat_regions(40, 20), images.noisy(40, 20, 8), images.grayscale(40, 20)]), None),
}


@pytest.mark.parametrize("name", list(OTHER))
def test_other_configurations(product, A, contexts, name):
    block, profile, make, swz = OTHER[name]
    profile = getattr(A, profile) if profile else A.PRF_LDR
    swz = (A.SWZ_B, A.SWZ_G, A.SWZ_R, A.SWZ_A) if swz == "bgra" else A.SWZ_RGBA
    c = Composition(product, A, contexts(block, A.PRE_FASTEST, profile), contexts(block, A.PRE_THOROUGH, profile), make(), block, swz, swz)
    selected, _ = c.check(what=name)
    assert selected.sum() >= 1


def test_mismatched_contexts_and_bad_arguments(product, A, contexts, flat_6x6):
    c = flat_6x6
    base = c.base
    err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, decompress_only = product.context_alloc(cfg, 1)
    assert err == 0
    try:
        cases = [(contexts((4, 4), A.PRE_THOROUGH), A.ERR_BAD_PARAM, "footprint"), (contexts((6, 5), A.PRE_THOROUGH), A.ERR_BAD_PARAM, "footprint y"),
                 (contexts((6, 6), A.PRE_THOROUGH, A.PRF_LDR_SRGB), A.ERR_BAD_PARAM, "profile"),
                 (contexts((6, 6), A.PRE_THOROUGH, flags=A.FLG_USE_ALPHA_WEIGHT), A.ERR_BAD_PARAM, "flags"), (decompress_only, A.ERR_BAD_CONTEXT, "decompress only")]
        for strong, code, what in cases:
            for pair in ((base, strong), (strong, base)):
                err, stats, got, records, intact = adaptive(product, A, pair[0], pair[1], c.t_image, c.blocks, (1.0, 1.0, 1.0, 1.0), 0.001, A.SWZ_RGBA, A.SWZ_RGBA)
                assert err == code, (what, err)
                assert intact and (got == FILL).all() and (records.view(np.uint8) == FILL).all(), what
    finally:
        product.context_free(decompress_only)
    # arguments: a bad criterion, a short stream, short records, a null image, a bad swizzle of either kind, an unknown type
    import torch
    L = product.lib
    whole = torch.full((GUARD + c.blocks * 16 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    whole_r = torch.full((GUARD + c.blocks * 32 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out, rec = whole.data_ptr() + GUARD, whole_r.data_ptr() + GUARD
    good, swz, bad_swz, z_swz = A.block_criterion(0.001), A.Swizzle(*A.SWZ_RGBA), A.Swizzle(0, 1, 2, 9), A.Swizzle(0, 1, A.SWZ_Z, 3)
    stats = A.AdaptiveStats()
    stats.blocks = 77

    def call(base=base, strong=c.strong, image=c.t_image.data_ptr(), dims=(50, 45, 1), dtype=0, s=swz, ds=swz, crit=good, out=out, out_len=c.blocks * 16,
             rec=rec, rec_len=c.blocks * 32):
        return L.astcenc_amd_compress_image_adaptive_device(base, strong, image, dims[0], dims[1], dims[2], dtype, C.byref(s) if s else None, C.byref(ds) if ds else None,
                                                            C.byref(crit) if crit else None, out, out_len, rec, rec_len, None, C.byref(stats))

    assert call(base=None) == A.ERR_BAD_PARAM and call(strong=None) == A.ERR_BAD_PARAM
    assert call(s=None) == A.ERR_BAD_PARAM and call(ds=None) == A.ERR_BAD_PARAM and call(crit=None) == A.ERR_BAD_PARAM
    assert call(crit=A.block_criterion(float("nan"))) == A.ERR_BAD_PARAM and call(crit=A.block_criterion(0.1, (1, -1, 1, 1))) == A.ERR_BAD_PARAM
    assert call(dtype=3) == A.ERR_BAD_PARAM and call(dims=(0, 45, 1)) == A.ERR_BAD_PARAM
    assert call(s=bad_swz) == A.ERR_BAD_SWIZZLE and call(ds=bad_swz) == A.ERR_BAD_SWIZZLE and call(s=z_swz) == A.ERR_BAD_SWIZZLE
    assert call(out_len=c.blocks * 16 - 1) == A.ERR_OUT_OF_MEM and call(rec_len=c.blocks * 32 - 1) == A.ERR_OUT_OF_MEM
    assert call(image=None) == A.ERR_BAD_CONTEXT and call(out=None) == A.ERR_BAD_CONTEXT
    assert stats.blocks == 77 and (whole.cpu().numpy() == FILL).all() and (whole_r.cpu().numpy() == FILL).all()
    # (the z swizzle is legal for scoring)
    assert call(ds=z_swz) == A.SUCCESS and stats.blocks == c.blocks


def test_side_stream_with_a_pending_producer(product, A, flat_6x6):
    """The image arrives by a copy queued behind a long kernel on a side stream: work queued on another stream would read noise."""
    import torch
    c = flat_6x6
    image = images.flat_regions(50, 45)
    weight, threshold = (1.0, 1.0, 1.0, 1.0), c.median_threshold()
    selected, replaced, want_bytes, want_records = c.expect(weight, threshold)
    side = torch.cuda.Stream()
    h_img = torch.from_numpy(image).pin_memory()
    d_img = torch.from_numpy(np.random.default_rng(6).integers(0, 256, image.shape, dtype=np.uint8)).cuda()
    out = torch.full((c.blocks * 16,), FILL, dtype=torch.uint8, device="cuda")
    records = torch.full((c.blocks * 4,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
        d_img.copy_(h_img, non_blocking=True)
        err, stats = product.compress_image_adaptive_device(c.base, c.strong, d_img, A.block_criterion(threshold, weight), out, block_errors=records, stream=side)
    assert err == 0
    side.synchronize()
    assert (stats.selected, stats.replaced) == (int(selected.sum()), int(replaced.sum()))
    assert np.array_equal(out.cpu().numpy().reshape(-1, 16), want_bytes)
    assert np.array_equal(records.cpu().numpy().view(np.uint64).reshape(-1, 4), want_records.view(np.uint64))
