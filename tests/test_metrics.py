# SPDX-License-Identifier: Apache-2.0
"""On-device quality metric (the CLI's -tl loop): blocks in device memory are
decoded into a device image and compared with the source there; only ten doubles come back.

  * astcenc_amd_decompress_image_device must produce the bytes astcenc_decompress_image produces;
  * astcenc_amd_compare_images_device must reproduce the sums of the reference's compute_error_metrics
    (Source/astcenccli_error_metrics.cpp:110-300), restated here in numpy: fp32 per-texel terms, fp64
    totals.  The totals are added in a different order, so the tolerance is 1e-12 relative.
Runs on the scalar CPU build here ("device" pointers are host pointers) and on the GPU with -m gpu.

The scalar build compares with one loop over the texels; the HIP build (csrc/kernel_metrics.hip) has launch logic of its own,
and each group of cases below is there for one part of it:

  * test_compare_tiny_rgba8_images: the four-texels-per-lane RGBA8 loop with no quad at all (1x1, 2x1, 3x1: the per-texel loop
    takes the whole image), one quad and an empty tail (4x1), and tails of 1, 2 and 3 texels (5x1, 7x6, 7x5).
  * test_compare_second_quad_trip_and_peak: 1031x2039 RGBA8 is 525 552 quads, more than the 2048 x 256 lanes of the capped grid,
    so the quad loop takes a second trip and pass 2 adds 32 partials per lane; the peak sits in turn in the first texel, in a
    second-trip quad and in the one-texel tail.
  * test_compare_generic_loop_past_the_group_cap: 733x719 is 527 027 texels, so the per-texel loop (any pair but U8-vs-U8, and
    every HDR call) takes a second trip under the cap.
  * test_compare_every_type_pair / test_compare_hdr_with_rgba8_operands: the nine type pairs through the per-texel loads (NaN,
    Inf, negative and > 65504 operands), and the HDR kernel with a U8 image on either side.
  * test_compare_volumes: dim_z > 1 is one flat texel list.
  * test_compare_sub_views_of_an_allocation: images at 4, 8 and 12 bytes from a 16-byte boundary take the per-texel loop instead
    of the 16-byte loads (both, or only one of the two), also past the group cap; F16 and F32 sub-views.
  * test_small_after_large_on_one_context: the per-slot partials buffer holds 2048 stale groups when a one-group call follows.
  * test_totals_are_bit_reproducible: fixed-order folds, no atomics: the same doubles on every run.
  * test_compare_stream_order_on_a_side_stream / test_decode_then_compare_on_a_side_stream: the caller's stream is honoured.
  * test_decode_into_guarded_memory*: astcenc_amd_decompress_image_device stores straight into caller memory: partial last
    blocks in x, y and z for every output type and swizzle, with guard bytes on both sides of the image and of the blocks.
  * test_figures_match_the_reference_report: the reference's own report also at the two sizes past the group cap.

What a wrong kernel would trip (each of these one-line changes reads owned memory only):
  * the tail starting one texel late (first = (quads << 2) + 1): every tiny image but 4x1, and the tail peak at 1031x2039;
  * the quad loop without its second trip: test_compare_second_quad_trip_and_peak, test_small_after_large_on_one_context,
    test_figures_match_the_reference_report;
  * the per-texel loop without its second trip: test_compare_generic_loop_past_the_group_cap, the 733x719 sub-views and
    the HDR pair of test_figures_match_the_reference_report;
  * a finish pass that adds its first 64 groups only: every case of more than 16 384 texels;
  * the 16-byte loads taken at any 4-byte alignment: no sum changes (the sub-views exist to show that)."""
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import pytest

import images

LIBS = [pytest.param("emu", id="emu"), pytest.param("product", id="hip", marks=pytest.mark.gpu)]
REL = 1e-12


@pytest.fixture(params=LIBS)
def lib(request):
    return request.getfixturevalue(request.param)


class Dev:
    """A buffer in the library's "device" memory: HBM through torch for the product, numpy for the emulator."""

    def __init__(self, lib, array, offset=None):
        """offset: the array starts that many bytes into an allocation 64 bytes larger than it (a sub-view)."""
        self.gpu = lib.backend_name().startswith("hip")
        self.dtype, self.shape = array.dtype, array.shape
        if offset is not None:
            flat = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
            self.view = slice(offset, offset + flat.size)
            whole = np.full(flat.size + 64, 0xEE, dtype=np.uint8)
            whole[self.view] = flat
            if self.gpu:
                import torch
                self.t = torch.from_numpy(whole).cuda()
                assert self.t.data_ptr() % 16 == 0
                self.ptr = self.t.data_ptr() + offset
            else:
                self.a = whole
                self.ptr = self.a.ctypes.data + offset
        elif self.gpu:
            import torch
            flat = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
            self.t = torch.from_numpy(flat.copy()).cuda()
            self.ptr = self.t.data_ptr()
        else:
            self.a = np.ascontiguousarray(array).copy()
            self.ptr = self.a.ctypes.data

    def host(self):
        whole = self.t.cpu().numpy() if self.gpu else self.a
        if hasattr(self, "view"):
            whole = whole[self.view].copy()
        return whole.view(self.dtype).reshape(self.shape)


def load_texels(x):
    """Texel components as compute_error_metrics sees them: U8 / 255, floats clamped to 0..65504 (fp32)."""
    if x.dtype == np.uint8:
        return x.astype(np.float32) / np.float32(255.0)
    v = x.astype(np.float32)
    v = np.where(v > 0, v, np.float32(0))          # NaN -> 0 like the reference's max/min pair
    return np.minimum(v, np.float32(65504.0))


def channel_totals(terms):
    """fp64 totals of [texels, 4] fp32 terms, one per channel, exactly rounded (math.fsum): the reference adds texel by texel,
    the kernel in a tree, and a total that is itself off by 1e-13 at two million texels would eat into REL."""
    t = np.ascontiguousarray(terms.astype(np.float64).T)
    return np.array([math.fsum(t[k].tolist()) for k in range(t.shape[0])])


def reference_sums(a, b):
    """compute_error_metrics' LDR accumulators, numpy restatement (fp32 terms, fp64 sums)."""
    c1, c2 = load_texels(a).reshape(-1, 4), load_texels(b).reshape(-1, 4)
    d = c1 - c2
    sq = channel_totals(d * d)
    ds = d.copy()
    ds[:, :3] *= c1[:, 3:4]
    asq = channel_totals(ds * ds)
    return sq, asq, float(c1[:, :3].max())


def compare(lib, ctx, A, a, b):
    da, db = Dev(lib, a), Dev(lib, b)
    types = {np.dtype(np.uint8): A.TYPE_U8, np.dtype(np.float16): A.TYPE_F16, np.dtype(np.float32): A.TYPE_F32}
    d = a.shape[0] if a.ndim == 4 else 1
    sums = A.ErrorSums()
    err = lib.lib.astcenc_amd_compare_images_device(ctx, da.ptr, types[a.dtype], db.ptr, types[b.dtype],
                                                    a.shape[-2], a.shape[-3], d, None, C.byref(sums))
    assert err == 0, lib.error_string(err)
    return sums


@pytest.fixture
def ctx66(lib, A):
    err, cfg = lib.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, lib.error_string(err)
    yield ctx
    lib.context_free(ctx)


def test_compare_matches_reference_formula(lib, A, ctx66):
    rng = np.random.default_rng(4)
    a = images.noisy(157, 93)
    b = np.clip(a.astype(np.int32) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    half = (a.astype(np.float32) / 255.0 * 3.0).astype(np.float16)
    half[3, 5, 1] = np.float16(np.nan); half[4, 6, 2] = np.float16(np.inf); half[9, 9, 0] = np.float16(-2.0)
    f32 = (b.astype(np.float32) / 255.0 * 2.5).astype(np.float32)
    for x, y in ((a, b), (a, a), (half, f32), (a, f32), (f32, half)):
        sums = compare(lib, ctx66, A, x, y)
        sq, asq, peak = reference_sums(x, y)
        assert np.allclose(np.array(sums.squared_error), sq, rtol=REL, atol=0), (x.dtype, y.dtype)
        assert np.allclose(np.array(sums.alpha_scaled_squared_error), asq, rtol=REL, atol=0)
        assert sums.rgb_peak == peak and sums.texels == 157 * 93
    assert compare(lib, ctx66, A, a, a).psnr() == 999.0
    # the formula of the CLI report, against the module's host-side restatement
    sums = compare(lib, ctx66, A, a, b)
    assert abs(sums.psnr() - A.psnr_rgba8(a, b)) < 1e-5
    assert sums.psnr(3) > 0 and sums.psnr(4, alpha_scaled=True) >= sums.psnr() - 1e-9


def reference_hdr_sums(a, b, fstop_lo, fstop_hi):
    """The HDR accumulators of compute_error_metrics (astcenccli_error_metrics.cpp:60-107, :262-268), numpy
    restatement: fp32 terms, fp64 sums; powf = correctly rounded float power (double pow, rounded)."""
    def log2_poly(x):
        i = x.view(np.int32)
        e = (((i.astype(np.int64) & 0x7F800000) >> 23) - 127).astype(np.float32)
        m = ((i & 0x007FFFFF) | 0x3F800000).view(np.float32)
        p = np.float32(0.0596515482674574969533)
        for c in (-0.465725644288844778798, 1.48116647521213171641, -2.52074962577807006663, 2.8882704548164776201):
            p = (p * m).astype(np.float32) + np.float32(c)
        p = p * (m - np.float32(1.0))
        return (p + e).astype(np.float32)

    def operator(v, stop):
        scale = np.float32(2.0) ** np.float32(stop)
        t = np.power((v * scale).astype(np.float32).astype(np.float64), np.float64(np.float32(1.0) / np.float32(2.2))).astype(np.float32)
        return np.clip(t * np.float32(255.0), np.float32(0), np.float32(255.0)).astype(np.float32)

    c1, c2 = np.ascontiguousarray(load_texels(a).reshape(-1, 4)), np.ascontiguousarray(load_texels(b).reshape(-1, 4))
    ld = log2_poly(c1) - log2_poly(c2)
    log_sq = channel_totals(ld * ld)
    summa = np.zeros_like(c1)
    for stop in range(fstop_lo, fstop_hi + 1):
        d = operator(c1, stop) - operator(c2, stop)
        summa = (summa + d * d).astype(np.float32)
    return log_sq, channel_totals(summa)


def test_hdr_sums_match_reference_formula(lib, A, ctx66):
    """mPSNR and log RMSE (what the reference CLI reports for BASELINE config 4).  Tolerance 1e-9 relative on the
    fp64 sums: the per-texel fp32 terms are the reference's arithmetic, the totals are added in another order, and
    the one libm call of the reference (powf) is a correctly rounded power on both sides."""
    rng = np.random.default_rng(12)
    src = images.hdr_f16(120, 88).astype(np.float16)
    noisy = (src.astype(np.float32) * (1.0 + rng.normal(0, 0.03, src.shape))).astype(np.float16)
    noisy[5, 7, 0] = np.float16(0.0); noisy[8, 3, 1] = np.float16(np.inf)
    types = {np.dtype(np.float16): A.TYPE_F16, np.dtype(np.float32): A.TYPE_F32}
    for x, y, lo, hi in ((src, noisy, -10, 10), (src.astype(np.float32), noisy, -4, 3), (src, src, 0, 0)):
        dx, dy = Dev(lib, x), Dev(lib, y)
        sums, hdr = A.ErrorSums(), A.HdrErrorSums()
        err = lib.lib.astcenc_amd_compare_images_hdr_device(ctx66, dx.ptr, types[x.dtype], dy.ptr, types[y.dtype], 120, 88, 1, lo, hi,
                                                            None, C.byref(sums), C.byref(hdr))
        assert err == 0, lib.error_string(err)
        log_sq, mp = reference_hdr_sums(x, y, lo, hi)
        assert np.allclose(np.array(hdr.log2_squared_error), log_sq, rtol=1e-9, atol=0)
        assert np.allclose(np.array(hdr.mpsnr_squared_error), mp, rtol=1e-9, atol=0)
        sq, asq, peak = reference_sums(x, y)
        assert np.allclose(np.array(sums.squared_error), sq, rtol=REL, atol=0) and sums.rgb_peak == peak
        assert (hdr.fstop_lo, hdr.fstop_hi) == (lo, hi)
        if x is y:
            assert hdr.mpsnr(sums.texels) == 999.0 and hdr.log_rmse(sums.texels) == 0.0
        else:
            assert 10.0 < hdr.mpsnr(sums.texels) < 80.0 and hdr.log_rmse(sums.texels) > 0.0
    sums, hdr = A.ErrorSums(), A.HdrErrorSums()
    d = Dev(lib, src)
    bad = lib.lib.astcenc_amd_compare_images_hdr_device(ctx66, d.ptr, A.TYPE_F16, d.ptr, A.TYPE_F16, 120, 88, 1, 3, 2, None, C.byref(sums), C.byref(hdr))
    assert bad == A.ERR_BAD_PARAM


def test_figures_match_the_reference_report(lib, A, ctx66, tmp_path):
    """The reference's own compute_error_metrics (astcenccli_error_metrics.cpp:110, compiled from where it lies into
    oracle/_ref/metrics_harness) prints its report for two raw images; the figures derived from the device sums must
    agree to the 4 decimals it prints -- LDR and HDR (mPSNR, LogRMSE, PSNR normalised to peak) alike."""
    import os
    import re
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "metrics_harness")
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/metrics_harness not built (no /root/reference on this machine)")
    rng = np.random.default_rng(31)
    a8 = images.noisy(150, 110)
    b8 = np.clip(a8.astype(np.int32) + rng.integers(-7, 8, a8.shape), 0, 255).astype(np.uint8)
    ah = images.hdr_f16(150, 110)
    bh = (ah.astype(np.float32) * (1.0 + rng.normal(0, 0.02, ah.shape))).astype(np.float16)
    types = {np.dtype(np.uint8): ("u8", A.TYPE_U8), np.dtype(np.float16): ("f16", A.TYPE_F16)}
    # ... and past the group cap: the RGBA8 quad loop's second trip, and the per-texel loop's on an HDR pair
    big8 = big_quads_images("tail")
    bigh_a = images.hdr_f16(*BIG_TEXELS)
    bigh_b = (bigh_a.astype(np.float32) * (1.0 + rng.normal(0, 0.02, bigh_a.shape))).astype(np.float16)
    # (on the scalar build this test takes 4.3 s with the CLI's default 21 f-stops at the large size -- double-precision pow over
    # 527 027 texels, 0.17 s per f-stop -- against 0.8 s for the slowest test this file had before, test_device_round_trip_psnr;
    # with 5 f-stops it takes 1.8 s.  That build's one loop has no launch logic to reach; the kernel gets the default range.)
    big_stops = (-10, 10) if lib.backend_name().startswith("hip") else (-2, 2)
    for x, y, hdr in ((a8, b8, False), (ah, bh, True), big8 + (None,), (bigh_a, bigh_b, True)):
        h, w = x.shape[:2]
        lo, hi = big_stops if x is bigh_a else (-10, 10)
        px, py = str(tmp_path / "x.raw"), str(tmp_path / "y.raw")
        x.tofile(px); y.tofile(py)
        tname, ttype = types[x.dtype]
        report = subprocess.run([exe, tname, str(w), str(h), px, py, "1" if hdr else "0", str(lo), str(hi)], capture_output=True, text=True, check=True).stdout

        def figure(label):
            m = re.search(re.escape(label) + r"\s*:?\s*(-?[0-9.]+)", report)
            assert m, (label, report)
            return float(m.group(1))
        dx, dy = Dev(lib, x), Dev(lib, y)
        sums, hs = A.ErrorSums(), A.HdrErrorSums()
        if hdr is None:         # (the LDR call: only that one takes the four-texel loop)
            err = lib.lib.astcenc_amd_compare_images_device(ctx66, dx.ptr, ttype, dy.ptr, ttype, w, h, 1, None, C.byref(sums))
        else:
            err = lib.lib.astcenc_amd_compare_images_hdr_device(ctx66, dx.ptr, ttype, dy.ptr, ttype, w, h, 1, lo, hi, None, C.byref(sums), C.byref(hs))
        assert err == 0 and sums.texels == w * h
        assert abs(sums.psnr() - figure("PSNR (LDR-RGBA):")) < 6e-5
        assert abs(sums.psnr(4, alpha_scaled=True) - figure("Alpha-weighted PSNR:")) < 6e-5
        assert abs(sums.psnr(3) - figure("PSNR (LDR-RGB):")) < 6e-5
        if hdr:
            assert abs(hs.mpsnr(sums.texels) - figure("mPSNR (RGB):")) < 6e-5
            assert abs(hs.log_rmse(sums.texels) - figure("LogRMSE (RGB):")) < 6e-5
            assert abs(sums.psnr(3) + 20.0 * np.log10(sums.rgb_peak) - figure("PSNR (RGB norm to peak):")) < 6e-5


def test_device_round_trip_psnr(lib, ref, A, ctx66):
    """compress -> (blocks stay on the device) -> decompress on the device -> compare on the device."""
    w, h = 200, 150
    img = images.noisy(w, h)
    blocks = lib.compress(img, (6, 6), A.PRE_MEDIUM)
    d_blocks = Dev(lib, blocks)
    d_out = Dev(lib, np.zeros_like(img))
    swz = A.Swizzle(*A.SWZ_RGBA)
    err = lib.lib.astcenc_amd_decompress_image_device(ctx66, d_blocks.ptr, blocks.nbytes, d_out.ptr, w, h, 1, A.TYPE_U8, C.byref(swz), None)
    assert err == 0, lib.error_string(err)
    decoded = d_out.host()
    assert np.array_equal(decoded, ref.decompress(blocks, w, h, (6, 6)))
    sums = compare(lib, ctx66, A, img, decoded)
    assert abs(sums.psnr() - A.psnr_rgba8(img, decoded)) < 1e-5
    assert sums.psnr() > 30.0
    # argument checks follow astcenc_decompress_image (ref: astcenc_entry.cpp:1296-1322)
    assert lib.lib.astcenc_amd_decompress_image_device(ctx66, d_blocks.ptr, blocks.nbytes - 1, d_out.ptr, w, h, 1, A.TYPE_U8, C.byref(swz), None) == A.ERR_OUT_OF_MEM
    assert lib.lib.astcenc_amd_decompress_image_device(ctx66, d_blocks.ptr, blocks.nbytes, d_out.ptr, 0, h, 1, A.TYPE_U8, C.byref(swz), None) == A.ERR_BAD_PARAM
    sums = A.ErrorSums()
    assert lib.lib.astcenc_amd_compare_images_device(ctx66, d_out.ptr, 0, d_out.ptr, 0, 0, h, 1, None, C.byref(sums)) == A.ERR_BAD_PARAM


def test_device_round_trip_volume(lib, ref, A):
    vol = images.volume("grad", 9, 14, 18)
    blocks = lib.compress(vol, (4, 4, 3), A.PRE_MEDIUM)
    err, cfg = lib.config_init(A.PRF_LDR, 4, 4, 3, A.PRE_MEDIUM, 0)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    try:
        d_blocks, d_out = Dev(lib, blocks), Dev(lib, np.zeros_like(vol))
        swz = A.Swizzle(*A.SWZ_RGBA)
        err = lib.lib.astcenc_amd_decompress_image_device(ctx, d_blocks.ptr, blocks.nbytes, d_out.ptr, 18, 14, 9, A.TYPE_U8, C.byref(swz), None)
        assert err == 0
        assert np.array_equal(d_out.host(), ref.decompress(blocks, 18, 14, (4, 4, 3), depth=9))
        sums = compare(lib, ctx, A, vol, d_out.host())
        assert sums.texels == 9 * 14 * 18 and sums.psnr() > 25.0
    finally:
        lib.context_free(ctx)


# ---- every launch path of the comparison, and the decoder's stores into caller memory (see the module docstring) ----

U8, F16, F32 = np.dtype(np.uint8), np.dtype(np.float16), np.dtype(np.float32)
NINE_PAIRS = [(ta, tb) for ta in (U8, F16, F32) for tb in (U8, F16, F32)]
BIG_QUADS = (1031, 2039)          # 2 102 209 texels = 525 552 quads + 1 texel: the quad loop's second trip starts at quad 524 288
BIG_TEXELS = (733, 719)           # 527 027 texels: the per-texel loop's second trip starts at texel 524 288
BIG_PEAKS = {"first": 0, "second_trip": 4 * 525000 + 2, "tail": 1031 * 2039 - 1}


def type_id(A, dtype):
    return {U8: A.TYPE_U8, F16: A.TYPE_F16, F32: A.TYPE_F32}[np.dtype(dtype)]


@contextlib.contextmanager
def context(lib, A, block=(6, 6), profile=None):
    err, cfg = lib.config_init(A.PRF_LDR if profile is None else profile, block[0], block[1], block[2] if len(block) > 2 else 1, A.PRE_MEDIUM, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, lib.error_string(err)
    try:
        yield ctx
    finally:
        lib.context_free(ctx)


def u8_pair(shape, seed, lo=0):
    """Random RGBA8 and a second image that differs from it by 1..9 in EVERY component (reflected at the ends of the range), so
    that no channel sum is anywhere near zero, even for a single texel; lo = 1 keeps zeros out."""
    rng = np.random.default_rng(seed)
    a = rng.integers(lo, 256, shape, dtype=np.int16)
    n = rng.integers(1, 10, shape, dtype=np.int16) * (2 * rng.integers(0, 2, shape, dtype=np.int16) - 1)
    b = np.where((a + n < lo) | (a + n > 255), a - n, a + n)
    return a.astype(np.uint8), b.astype(np.uint8)


def typed_pair(ta, tb, shape, seed, lo=0, specials=False):
    """The pair of u8_pair with each image in its own type: a float image holds value / 255 * 3.  specials: every float image
    gets a NaN and a negative at texels of its own, and +Inf and (F32) a value above 65504 in the blue of two texels that both
    images share.  Where both images are float, both sides of those two texels load as 65504 and their terms are 0, so every
    sum stays a sum of small terms and a lost texel shows in every channel.  Against a U8 image the blue sums are about 1e10
    and blind to one ordinary texel: such pairs are also run without specials (test_compare_every_type_pair)."""
    a8, b8 = u8_pair(shape, seed, lo)
    out = []
    texels = a8.size // 4
    for x8, t, at in ((a8, np.dtype(ta), texels // 7), (b8, np.dtype(tb), texels // 2)):
        if t == U8:
            out.append(x8)
            continue
        x = (x8.astype(np.float32) / np.float32(255.0) * np.float32(3.0)).astype(t)
        if specials:
            flat = x.reshape(-1, 4)
            flat[at, 0] = np.nan
            flat[at + 1, 1] = -2.0
            flat[texels // 3, 2] = np.inf
            flat[texels // 3 + 1, 2] = 1.0e5 if t == F32 else np.inf
        out.append(x)
    return out[0], out[1]


def run_compare(lib, ctx, A, da, db, dims, hdr=None, stream=None):
    """The LDR call, or with hdr = (fstop_lo, fstop_hi) the HDR call, on two Dev buffers; dims = (x, y, z)."""
    sums, hs = A.ErrorSums(), A.HdrErrorSums()
    ta, tb = type_id(A, da.dtype), type_id(A, db.dtype)
    if hdr is None:
        err = lib.lib.astcenc_amd_compare_images_device(ctx, da.ptr, ta, db.ptr, tb, dims[0], dims[1], dims[2], stream, C.byref(sums))
    else:
        err = lib.lib.astcenc_amd_compare_images_hdr_device(ctx, da.ptr, ta, db.ptr, tb, dims[0], dims[1], dims[2], hdr[0], hdr[1], stream,
                                                            C.byref(sums), C.byref(hs))
    assert err == 0, lib.error_string(err)
    return sums, hs


def dims_of(a):
    return (a.shape[-2], a.shape[-3], a.shape[0] if a.ndim == 4 else 1)


def doubles(sums, hs=None):
    """Every double of a result, bit for bit."""
    return bytes(sums) + (bytes(hs) if hs is not None else b"")


def assert_ldr(sums, want, what):
    sq, asq, peak = want
    got_sq, got_asq = np.array(sums.squared_error), np.array(sums.alpha_scaled_squared_error)
    assert (sq > 0).all() and (asq > 0).all(), what
    assert np.allclose(got_sq, sq, rtol=REL, atol=0), (what, got_sq, sq)
    assert np.allclose(got_asq, asq, rtol=REL, atol=0), (what, got_asq, asq)
    assert sums.rgb_peak == peak, (what, sums.rgb_peak, peak)


def assert_hdr(hs, want, what):
    log_sq, mp = want
    got_log, got_mp = np.array(hs.log2_squared_error), np.array(hs.mpsnr_squared_error)
    assert (log_sq > 0).all() and (mp > 0).all(), what
    assert np.allclose(got_log, log_sq, rtol=1e-9, atol=0), (what, got_log, log_sq)
    assert np.allclose(got_mp, mp, rtol=1e-9, atol=0), (what, got_mp, mp)


def check_pair(lib, ctx, A, a, b, hdr=None, what=None, off_a=None, off_b=None):
    """One comparison against the numpy reference of the flattened texel list; returns the result's doubles."""
    what = what or "%s-%s %s" % (a.dtype, b.dtype, a.shape)
    sums, hs = run_compare(lib, ctx, A, Dev(lib, a, off_a), Dev(lib, b, off_b), dims_of(a), hdr)
    assert sums.texels == a.size // 4, what
    assert_ldr(sums, reference_sums(a, b), what)
    if hdr is not None:
        assert_hdr(hs, reference_hdr_sums(a, b, hdr[0], hdr[1]), what)
        assert (hs.fstop_lo, hs.fstop_hi) == hdr
    return doubles(sums, hs if hdr is not None else None)


@functools.lru_cache(maxsize=None)
def big_quads_images(peak_at):
    """The 1031x2039 RGBA8 pair whose first image has its one largest R, G or B value at texel BIG_PEAKS[peak_at]."""
    w, h = BIG_QUADS
    a, b = u8_pair((h, w, 4), 2039)
    a[..., :3] = np.minimum(a[..., :3], 250)
    a.reshape(-1, 4)[BIG_PEAKS[peak_at], 1] = 255
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@functools.lru_cache(maxsize=None)
def big_quads_pair(peak_at):
    """... with its reference sums (computed once, shared, read only)."""
    a, b = big_quads_images(peak_at)
    return a, b, reference_sums(a, b)


@functools.lru_cache(maxsize=None)
def big_texels_pair(ta, tb, hdr):
    w, h = BIG_TEXELS
    a, b = typed_pair(ta, tb, (h, w, 4), 733, lo=1)
    a.setflags(write=False); b.setflags(write=False)
    return a, b, reference_sums(a, b), (reference_hdr_sums(a, b, hdr[0], hdr[1]) if hdr else None)


@pytest.fixture(scope="module", autouse=True)
def release_big_images():
    """The shared large images and their references (about 70 MB) live as long as this module's tests."""
    yield
    for cached in (big_quads_images, big_quads_pair, big_texels_pair):
        cached.cache_clear()


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (7, 6), (7, 5)])
def test_compare_tiny_rgba8_images(lib, A, ctx66, w, h):
    """RGBA8 against RGBA8 with no quad at all, with one quad and nothing after it, and with 1, 2 and 3 texels after the last quad."""
    a, b = u8_pair((h, w, 4), 100 * w + h)
    check_pair(lib, ctx66, A, a, b)
    peak_last = a.copy()
    peak_last[..., :3] = np.minimum(peak_last[..., :3], 250)
    peak_last[-1, -1, 2] = 255                          # the peak in the last texel: of the tail, or of the only quad
    check_pair(lib, ctx66, A, peak_last, b, what="peak in the last texel of %dx%d" % (w, h))


@pytest.mark.parametrize("peak_at", list(BIG_PEAKS))
def test_compare_second_quad_trip_and_peak(lib, A, ctx66, peak_at):
    a, b, want = big_quads_pair(peak_at)
    assert BIG_PEAKS["second_trip"] // 4 >= 2048 * 256 and BIG_PEAKS["tail"] == (a.size // 16) * 4
    sums, _ = run_compare(lib, ctx66, A, Dev(lib, a), Dev(lib, b), dims_of(a))
    assert sums.texels == 1031 * 2039 and want[2] == 1.0
    assert_ldr(sums, want, "1031x2039 peak at " + peak_at)


@pytest.mark.parametrize("ta,tb,hdr", [(F16, F32, None), (U8, F16, None), (F16, F16, (-1, 1))], ids=["f16-f32", "u8-f16", "f16-f16-hdr"])
def test_compare_generic_loop_past_the_group_cap(lib, A, ctx66, ta, tb, hdr):
    a, b, want, want_hdr = big_texels_pair(ta, tb, hdr)
    sums, hs = run_compare(lib, ctx66, A, Dev(lib, a), Dev(lib, b), dims_of(a), hdr)
    assert sums.texels == 733 * 719
    assert_ldr(sums, want, "733x719 %s-%s" % (ta, tb))
    if hdr:
        assert_hdr(hs, want_hdr, "733x719 hdr")


@pytest.mark.parametrize("ta,tb", NINE_PAIRS, ids=["%s-%s" % p for p in NINE_PAIRS])
def test_compare_every_type_pair(lib, A, ctx66, ta, tb):
    """Ordinary content first (every sum is one of small terms, so one lost texel shows in every channel), then the specials."""
    check_pair(lib, ctx66, A, *typed_pair(ta, tb, (37, 61, 4), 61), what="%s-%s plain" % (ta, tb))
    check_pair(lib, ctx66, A, *typed_pair(ta, tb, (37, 61, 4), 61, specials=True), what="%s-%s specials" % (ta, tb))


@pytest.mark.parametrize("ta,tb", [p for p in NINE_PAIRS if U8 in p], ids=["%s-%s" % p for p in NINE_PAIRS if U8 in p])
def test_compare_hdr_with_rgba8_operands(lib, A, ctx66, ta, tb):
    """(no zeros in the content: log2 of 0 is pinned by test_hdr_sums_match_reference_formula)"""
    a, b = typed_pair(ta, tb, (37, 61, 4), 37, lo=1)
    check_pair(lib, ctx66, A, a, b, hdr=(-10, 10))


def test_compare_volumes(lib, A, ctx66):
    a, b = u8_pair((3, 7, 5, 4), 375)
    check_pair(lib, ctx66, A, a, b)
    a, b = typed_pair(F16, F16, (2, 9, 11, 4), 2911, specials=True)
    check_pair(lib, ctx66, A, a, b)
    check_pair(lib, ctx66, A, *typed_pair(F16, F16, (2, 9, 11, 4), 2912, lo=1), hdr=(-3, 2))


def test_compare_sub_views_of_an_allocation(lib, A, ctx66):
    """Images that do not start on a 16-byte boundary (texel-aligned sub-views of a larger allocation)."""
    a, b = u8_pair((93, 157, 4), 157)
    for off in (4, 8, 12):
        for off_a, off_b in ((off, off), (off, 0), (0, off)):
            check_pair(lib, ctx66, A, a, b, off_a=off_a, off_b=off_b, what="u8 at +%d / +%d" % (off_a, off_b))
    a, b, ref_sums, _ = big_texels_pair(U8, U8, None)
    sums, _ = run_compare(lib, ctx66, A, Dev(lib, a, 4), Dev(lib, b, 4), dims_of(a))
    assert_ldr(sums, ref_sums, "733x719 u8 at +4")
    sums, _ = run_compare(lib, ctx66, A, Dev(lib, a, 12), Dev(lib, b, 0), dims_of(a))
    assert_ldr(sums, ref_sums, "733x719 u8 at +12 / +0")
    check_pair(lib, ctx66, A, *typed_pair(F16, F16, (93, 157, 4), 158, specials=True), off_a=8, off_b=8, what="f16 at +8")
    check_pair(lib, ctx66, A, *typed_pair(F32, F32, (93, 157, 4), 159, specials=True), off_a=16, off_b=16, what="f32 at +16")


def test_small_after_large_on_one_context(lib, A, ctx66):
    """The partials of a slot are allocated once: after a call that filled all 2048 group slots, calls of one and of nine groups
    must add their own groups only."""
    a, b, want = big_quads_pair("tail")
    sums, _ = run_compare(lib, ctx66, A, Dev(lib, a), Dev(lib, b), dims_of(a))
    assert_ldr(sums, want, "large")
    small = u8_pair((1, 5, 4), 51)
    first = check_pair(lib, ctx66, A, *small, what="5x1 after large")
    check_pair(lib, ctx66, A, *typed_pair(F16, U8, (37, 61, 4), 6137, lo=1), hdr=(-10, 10), what="61x37 hdr after large")
    again = check_pair(lib, ctx66, A, *small, what="5x1 after hdr")
    assert first == again


@pytest.mark.gpu
def test_totals_are_bit_reproducible(product, A):
    """No atomics, fixed-order folds: the same call gives the same doubles, bit for bit."""
    with context(product, A) as ctx:
        for a, b, hdr in (big_quads_images("tail") + (None,), big_texels_pair(F16, F32, None)[:2] + (None,),
                          big_texels_pair(F16, F16, (-1, 1))[:2] + ((-1, 1),)):
            da, db = Dev(product, a), Dev(product, b)
            runs = [doubles(*run_compare(product, ctx, A, da, db, dims_of(a), hdr)) for _ in range(3)]
            assert runs[0] == runs[1] == runs[2], (a.dtype, a.shape)


@pytest.mark.gpu
def test_compare_stream_order_on_a_side_stream(product, A):
    """The images arrive by copies queued on the caller's stream behind a long kernel: the comparison must run behind them."""
    import torch
    a, b = u8_pair((301, 403, 4), 403)
    other = np.random.default_rng(5).integers(0, 256, a.shape, dtype=np.uint8)
    with context(product, A) as ctx:
        side = torch.cuda.Stream()
        ha, hb = torch.from_numpy(a).pin_memory(), torch.from_numpy(b).pin_memory()
        da, db = torch.from_numpy(other).cuda(), torch.from_numpy(other[::-1].copy()).cuda()
        torch.cuda.synchronize()
        sums = A.ErrorSums()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            da.copy_(ha, non_blocking=True)
            db.copy_(hb, non_blocking=True)
            err = product.lib.astcenc_amd_compare_images_device(ctx, da.data_ptr(), A.TYPE_U8, db.data_ptr(), A.TYPE_U8, 403, 301, 1,
                                                                A.torch_stream(side), C.byref(sums))
        assert err == 0, product.error_string(err)
        side.synchronize()
        assert sums.texels == 403 * 301
        assert_ldr(sums, reference_sums(a, b), "side stream")


@pytest.mark.gpu
def test_decode_then_compare_on_a_side_stream(product, ref, A):
    """Blocks and source copied on the caller's stream, decoded there and compared there, nothing synchronised in between."""
    import torch
    w, h = 206, 135
    img = images.noisy(w, h, 21)
    blocks = ref.compress(img, (6, 6), 60.0)
    want = ref.decompress(blocks, w, h, (6, 6))
    rng = np.random.default_rng(6)
    with context(product, A) as ctx:
        side = torch.cuda.Stream()
        h_blocks, h_img = torch.from_numpy(blocks).pin_memory(), torch.from_numpy(img).pin_memory()
        d_blocks = torch.from_numpy(rng.integers(0, 256, blocks.shape, dtype=np.uint8)).cuda()
        d_img = torch.from_numpy(rng.integers(0, 256, img.shape, dtype=np.uint8)).cuda()
        d_out = torch.full(img.shape, 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        swz, sums = A.Swizzle(*A.SWZ_RGBA), A.ErrorSums()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            d_blocks.copy_(h_blocks, non_blocking=True)
            d_img.copy_(h_img, non_blocking=True)
            e1 = product.lib.astcenc_amd_decompress_image_device(ctx, d_blocks.data_ptr(), blocks.nbytes, d_out.data_ptr(), w, h, 1, A.TYPE_U8,
                                                                 C.byref(swz), A.torch_stream(side))
            e2 = product.lib.astcenc_amd_compare_images_device(ctx, d_img.data_ptr(), A.TYPE_U8, d_out.data_ptr(), A.TYPE_U8, w, h, 1,
                                                               A.torch_stream(side), C.byref(sums))
        assert (e1, e2) == (0, 0)
        side.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want)
        assert_ldr(sums, reference_sums(img, want), "decode then compare")


GUARD = 4096
SWIZZLES = ["SWZ_R SWZ_G SWZ_B SWZ_A", "SWZ_B SWZ_G SWZ_R SWZ_A", "SWZ_R SWZ_A SWZ_Z SWZ_1", "SWZ_0 SWZ_1 SWZ_G SWZ_G"]   # test_decode_srgb_and_swizzles'


class Guarded:
    """`content` in "device" memory between two guard regions of GUARD bytes of 0xAB, all of it one allocation of the test's."""

    def __init__(self, lib, content):
        self.gpu = lib.backend_name().startswith("hip")
        self.whole = np.full(GUARD + content.size + GUARD, 0xAB, dtype=np.uint8)
        self.whole[GUARD:GUARD + content.size] = content
        if self.gpu:
            import torch
            self.t = torch.from_numpy(self.whole).cuda()
            self.ptr = self.t.data_ptr() + GUARD
        else:
            self.a = self.whole.copy()
            self.ptr = self.a.ctypes.data + GUARD

    def payload(self, what):
        """The bytes between the guards, after checking that the guards are as they were."""
        now = self.t.cpu().numpy() if self.gpu else self.a
        for name, region in (("before", slice(0, GUARD)), ("after", slice(len(now) - GUARD, len(now)))):
            hit = np.flatnonzero(now[region] != 0xAB)
            assert hit.size == 0, "%s: %d guard bytes %s the buffer overwritten, first at %d" % (what, hit.size, name, hit[0])
        return now[GUARD:len(now) - GUARD]


def host_decode(L, A, data, dims, block, profile, out_type, swizzle):
    """astcenc_decompress_image of library L (the reference): [D, H, W, 4]."""
    w, h, d = dims
    err, cfg = L.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, A.PRE_MEDIUM, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, ctx = L.context_alloc(cfg, 1)
    assert err == 0, L.error_string(err)
    try:
        out = np.zeros((d, h, w, 4), dtype=out_type)
        slices = (C.c_void_p * d)(*[out.ctypes.data + z * out[0].nbytes for z in range(d)])
        img = A.Image(w, h, d, type_id(A, out.dtype), slices)
        swz = A.Swizzle(*swizzle)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        err = L.lib.astcenc_decompress_image(ctx, data.ctypes.data, data.nbytes, C.byref(img), C.byref(swz), 0)
        assert err == 0, L.error_string(err)
        return out
    finally:
        L.context_free(ctx)


def check_guarded_decodes(lib, ref, A, data, dims, block, profile, extra_len=0):
    """Every output type and swizzle into guarded caller memory: the reference's image bit for bit, guards and blocks untouched."""
    from test_decode import same
    w, h, d = dims
    tail = np.random.default_rng(77).integers(0, 256, extra_len, dtype=np.uint8)
    with context(lib, A, block, profile) as ctx:
        d_blocks = Guarded(lib, np.concatenate([data, tail]))
        for out_type in (np.uint8, np.float16, np.float32):
            for names in SWIZZLES:
                swizzle = tuple(getattr(A, n) for n in names.split())
                what = "%s %s %s %s" % (block, dims, np.dtype(out_type), names)
                want = host_decode(ref, A, data, dims, block, profile, out_type, swizzle)
                d_out = Guarded(lib, np.full(want.nbytes, 0xCD, dtype=np.uint8))
                swz = A.Swizzle(*swizzle)
                err = lib.lib.astcenc_amd_decompress_image_device(ctx, d_blocks.ptr, data.nbytes + extra_len, d_out.ptr, w, h, d,
                                                                  type_id(A, out_type), C.byref(swz), None)
                assert err == 0, (what, lib.error_string(err))
                got = d_out.payload(what).view(out_type).reshape(want.shape)
                assert same(want, got), (what, np.argwhere(want.view(np.uint8) != got.view(np.uint8))[:3])
        assert np.array_equal(d_blocks.payload("blocks of %s" % (block,)), np.concatenate([data, tail]))


def partial_block_image(block, hdr=False):
    """An image with a partial last block in every axis (test_decode_ldr_matches_reference's sizes; 2 * bz + 1 slices)."""
    w, h = block[0] * 5 + 2, block[1] * 4 + 3
    make = images.hdr_f16 if hdr else images.noisy
    if len(block) == 2:
        return make(w, h, 60 + block[0]), (w, h, 1)
    d = 2 * block[2] + 1
    return np.stack([make(w, h, 60 + z) for z in range(d)]), (w, h, d)


DEVICE_FOOTPRINTS = [(4, 4), (6, 6), (10, 8), (12, 12), (3, 3, 3), (6, 6, 6)]


@pytest.mark.parametrize("block", DEVICE_FOOTPRINTS, ids=["x".join(map(str, b)) for b in DEVICE_FOOTPRINTS])
def test_decode_into_guarded_memory(lib, ref, A, block):
    im, dims = partial_block_image(block)
    data = ref.compress(im, block, 60.0)
    check_guarded_decodes(lib, ref, A, data, dims, block, A.PRF_LDR, extra_len=48 if block == (6, 6) else 0)   # (6x6: data_len larger than needed)


@pytest.mark.parametrize("profile_name", ["PRF_LDR_SRGB", "PRF_HDR", "PRF_HDR_RGB_LDR_A"])
def test_decode_into_guarded_memory_profiles(lib, ref, A, profile_name):
    profile = getattr(A, profile_name)
    im, dims = partial_block_image((6, 6), hdr=profile_name != "PRF_LDR_SRGB")
    data = ref.compress(im, (6, 6), 60.0, profile=profile)
    check_guarded_decodes(lib, ref, A, data, dims, (6, 6), profile)


@pytest.mark.parametrize("block", [b for b in DEVICE_FOOTPRINTS if len(b) == 2], ids=["x".join(map(str, b)) for b in DEVICE_FOOTPRINTS if len(b) == 2])
def test_decode_into_guarded_memory_random_bit_patterns(lib, ref, A, block):
    """test_decode_random_bit_patterns' generator (reserved modes, illegal void extents, HDR endpoint formats), 12 x 8 blocks."""
    rng = np.random.default_rng(99 + block[0] + block[1])
    nbx, nby = 12, 8
    data = rng.integers(0, 256, size=nbx * nby * 16, dtype=np.uint8)
    blocks = data.reshape(-1, 16)
    blocks[::7, 0] = 0xFC
    blocks[::7, 1] |= 0x01
    blocks[::14, 1] = 0xFD
    blocks[::14, 2:8] = 0xFF
    blocks[::28, 1] = 0xFF
    blocks[1::5, 1] &= 0xE7
    for profile in (A.PRF_LDR, A.PRF_HDR):
        check_guarded_decodes(lib, ref, A, data, (nbx * block[0], nby * block[1], 1), block, profile)
