# SPDX-License-Identifier: Apache-2.0
"""The HIP decoder and everything that instantiates decode_row_batch (csrc/wave_decode.h) again -- windows, tensor stores, the
scaled staging sink, the block-quality sink -- over the streams of tests/decode_cases.py, against the reference decoder bit for
bit.  The CPU side (the matrix, the composed runs, the sequential build of the same source) is tests/test_decode_coverage_cpu.py.

The sinks are checked with the helpers of their own test modules (no model is added here); for each sink the builds of
decode_row_texels its runs select are computed from oracle info (decode_cases.run_build) and every one of the seven must occur."""
import numpy as np
import pytest

import decode_cases as D
import tensor_model as M
import test_block_quality as Q
import test_decode_regions as R
import test_decode_scaled as SC
import test_decode_tensors as T

pytestmark = pytest.mark.gpu

IDS = [D.block_id(b) for b in D.FOOTPRINTS]
SWZ_NAME = {"rgba": "rgba", "bgra": "bgra", "z": "raz1"}            # the sinks' modules' names -> decode_cases.SWIZZLES


def sink_stream(block):
    """The composed stream with the 17-block tail: it holds runs of every class (asserted where it is used)."""
    return next(s for s in D.composed(block) if s.name.endswith("tail17"))


def dev(stream):
    import torch
    return torch.from_numpy(np.array(stream.data)).cuda()


def block3(block):
    return (block[0], block[1], block[2] if len(block) > 2 else 1)


@pytest.fixture(scope="module")
def contexts(product, A):
    made = {}

    def get(block, profile, flags=None):
        flags = A.FLG_DECOMPRESS_ONLY if flags is None else flags
        key = (tuple(block), profile, flags)
        if key not in made:
            err, cfg = product.config_init(getattr(A, profile), block[0], block[1], block3(block)[2], A.PRE_FASTEST, flags)
            assert err == 0
            err, ctx = product.context_alloc(cfg, 1)
            assert err == 0, product.error_string(err)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


def builds_of(stream, profile, out_type, swizzle, first=0, last=None):
    return {b for (b, _), n in stream.build_census(profile, out_type, D.SWIZZLES[swizzle], first, last).items() if n}


@pytest.mark.parametrize("profile", D.PROFILES)
@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_image_decode_of_every_stream_is_the_references(product, ref, A, block, profile):
    """astcenc_decompress_image on the device: every stream (composed, shuffled, the whole pool), U8 / F16 / F32, the identity,
    BGRA and (R, A, Z, 1) swizzles."""
    for s in D.streams(block):
        for out_type in D.OUT_TYPES:
            for swz in D.SWIZZLES:
                want = D.reference_decode(ref, A, s, profile, out_type, swz, keep=s.name.endswith("tail17"))
                got = D.decode(product, A, s, profile, out_type, swz)
                bad = D.explain(s, want, got, profile, out_type, swz)
                assert bad is None, bad


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_image_set_decode_of_the_composed_streams_in_one_launch(product, ref, A, contexts, block):
    """astcenc_amd_decompress_images_device: the three composed streams of a footprint and the whole pool -- four widths, three
    data types, three swizzles -- as one set (a set's entries share the context's footprint)."""
    import torch
    dtypes = {np.uint8: torch.uint8, np.float16: torch.float16, np.float32: torch.float32}
    entries = list(zip(D.composed(block) + [D.streams(block)[-1]], (np.uint8, np.float16, np.float32, np.uint8), ("rgba", "raz1", "bgra", "bgra")))
    seen = set()
    for profile in ("PRF_HDR", "PRF_LDR_SRGB"):
        outs, args = [], []
        for s, out_type, swz in entries:
            w, h, d = s.dims
            outs.append(torch.full((d, h, w, 4) if d > 1 else (h, w, 4), 7, dtype=dtypes[out_type], device="cuda"))
            args.append((outs[-1], dev(s), D.swizzle_of(A, swz)))
            if len(block) == 2:
                seen |= builds_of(s, profile, out_type, swz)
        assert product.decompress_images_device(contexts(block, profile), args) == A.SUCCESS
        torch.cuda.synchronize()
        for (s, out_type, swz), out in zip(entries, outs):
            want = D.reference_decode(ref, A, s, profile, out_type, swz, keep=False)
            bad = D.explain(s, want, out.cpu().numpy().reshape(want.shape), profile, out_type, swz)
            assert bad is None, bad
    assert len(block) == 3 or seen == set(D.BUILDS_2D), seen


def coverage_windows(stream):
    """Windows that start and end inside blocks: one whose runs are the image's (it starts in block 0), one whose runs start at
    block 5 and cross the image's run boundaries, and the hand-picked ones of the regions test."""
    (w, h, d), (bx, by, bz) = stream.dims, block3(stream.block)
    out = [((1, 1, 0), (w - 2, h - 2, d)), ((5 * bx + 2, by // 2, 0), (40 * bx, h - by // 2, d))] + R.hand_picked(stream.dims, block3(stream.block))
    # (a volume of two block rows is lower than one of the hand-picked windows reaches)
    return [(o, n) for o, n in out if all(a + b <= c for a, b, c in zip(o, n, stream.dims))]


@pytest.mark.parametrize("block", [(6, 6), (4, 4, 4)], ids=["6x6", "4x4x4"])
def test_regions_of_a_composed_stream(product, ref, A, contexts, block):
    """astcenc_amd_decompress_regions_device, the regions test's combinations of profile, type and swizzle."""
    import torch
    s = sink_stream(block)
    blocks = dev(s)
    windows = coverage_windows(s)
    seen = set()
    for prf, t, z in R.COMBOS:
        swz = SWZ_NAME[z]
        whole = D.reference_decode(ref, A, s, prf, R.NP_TYPES[t], swz)
        outs = R.run_windows(product, A, contexts(block, prf), [(blocks, s.dims, t, D.swizzle_of(A, swz))], [(0, o, n) for o, n in windows])
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            origin, size = windows[i // 2]
            o.check(R.crop_of(whole, origin, size), "%s %s %s %s window %r %r%s" % (s.name, prf, t, swz, origin, size, " padded" if i % 2 else ""))
        if len(block) == 2:
            # (the first window's runs are the image's; the second's start at block 5)
            here = builds_of(s, prf, R.NP_TYPES[t], swz)
            assert set(D.expected_builds(prf, R.NP_TYPES[t], D.SWIZZLES[swz])) <= here, (prf, t, swz, here)
            seen |= here | builds_of(s, prf, R.NP_TYPES[t], swz, 5, 5 + 40)
    assert len(block) == 3 or seen == set(D.BUILDS_2D), seen


TENSOR_COMBOS = [
    T.COMBOS[0],                                                                             # LDR, U8 entry -> fp16 planar, three channels
    ("PRF_HDR", "u8", "bgra", M.F32, M.INTERLEAVED, 4, (1 / 255, 2.0, -0.5, 1.0), (0.0, -1.0, 0.25, 3.0)),      # -> fp32 interleaved
    T.COMBOS[2],                                                                             # HDR, F16 entry (NaN texels of error blocks)
]


@pytest.mark.parametrize("block", [(6, 6), (3, 3, 3)], ids=["6x6", "3x3x3"])
def test_tensors_of_a_composed_stream(product, ref, A, contexts, block):
    """astcenc_amd_decompress_tensors_device: fp16 planar and fp32 interleaved, the flips rotating over the windows."""
    s = sink_stream(block)
    blocks = dev(s)
    windows = coverage_windows(s)[:6]
    seen = set()
    for n, combo in enumerate(TENSOR_COMBOS):
        prf, t, z = combo[:3]
        swz = SWZ_NAME[z]
        whole = D.reference_decode(ref, A, s, prf, R.NP_TYPES[t], swz)
        entry = A.compressed_entry(blocks, s.dims, R.type_of(A, t), D.swizzle_of(A, swz))
        T.run_and_check(product, A, contexts(block, prf), entry, whole, windows, combo, flip0=n + 1, what="%s %s %s %s" % (s.name, prf, t, swz))
        if len(block) == 2:
            seen |= builds_of(s, prf, R.NP_TYPES[t], swz)
    assert len(block) == 3 or seen == set(D.BUILDS_2D), seen


def scaled_taps(S, D_, j):
    """(lo, hi) of output position j, bilinear (scaled_taps, csrc/decode_scaled.h)."""
    m = (2 * j + 1) * S
    if m < D_:
        return 0, 0
    i0 = (m - D_) // (2 * D_)
    return min(i0, S - 1), min(i0 + 1, S - 1)


def scaled_runs(stream, origin, size, out, texel_bytes):
    """The runs the scaled call decodes for one region, by the tiling of csrc/decode_scaled.h (decode_scaled_tiling,
    decode_scaled_rect, decode_scaled_tile) -- for the coverage claim only."""
    (bx, by), (x, y, _), (sx, sy), (ox, oy) = stream.block, origin, size, out
    run_blocks = min(6144 // texel_bytes // (bx * by), D.RUN)
    hold = (run_blocks - 1) * bx + 1
    c = (hold - 3) * ox // sx if hold > 3 else 0
    cols = 64 if c >= 64 else c if c >= 8 else 8
    band = min(oy, 8)
    runs = []
    for r0 in range(0, oy, band):
        rows = range(r0, min(r0 + band, oy))
        bya, byb = (y + scaled_taps(sy, oy, rows[0])[0]) // by, (y + scaled_taps(sy, oy, rows[-1])[1]) // by
        for c0 in range(0, ox, cols):
            last = min(c0 + cols, ox) - 1
            bxa, bxb = (x + scaled_taps(sx, ox, c0)[0]) // bx, (x + scaled_taps(sx, ox, last)[1]) // bx
            for row in range(bya, byb + 1):
                for b in range(bxa, bxb + 1, run_blocks):
                    runs.append(stream.infos[row * stream.nbx + b: row * stream.nbx + min(b + run_blocks, bxb + 1)])
    return runs


def test_scaled_tensors_of_a_composed_stream(product, A, contexts):
    """astcenc_amd_decompress_scaled_tensors_device, bilinear at 3 : 1 on 6x6: one window per composed run of the stream, each from
    inside the run's first block over two block rows, against tests/scaled_model.py on the texels the regions call gives for the
    window (which the regions test above holds to the reference)."""
    block = (6, 6)
    s = sink_stream(block)
    blocks = dev(s)
    cases = [(0, (k * D.RUN * 6 + 1, row * 6 + 1, 0), (189, 9), (63, 3)) for row in range(s.nby - 2) for k in (0, 1)]
    assert all(x + sx <= s.dims[0] and y + sy <= s.dims[1] for _, (x, y, _), (sx, sy), _ in cases)
    seen = set()
    for prf in ("PRF_HDR", "PRF_LDR"):
        entry = A.compressed_entry(blocks, s.dims, A.TYPE_U8)
        SC.run_and_check(product, A, contexts(block, prf), [entry], A.WINDOW_BILINEAR, (M.F16, M.PLANAR, 3), cases, flip0=1, what="%s %s" % (s.name, prf))
        for _, origin, size, out in cases:
            seen |= {D.run_build(infos, prf, np.uint8, D.SWIZZLES["rgba"]) for infos in scaled_runs(s, origin, size, out, 4)}
    assert seen == set(D.BUILDS_2D), seen


@pytest.mark.parametrize("block", [(6, 6), (4, 4, 4)], ids=["6x6", "4x4x4"])
def test_block_quality_of_a_composed_stream(product, A, contexts, block):
    """astcenc_amd_compare_blocks_device: the fused decode-and-compare against decoding and comparing in two calls, per block and
    in total (check_case of tests/test_block_quality.py), in an LDR and an HDR context."""
    s = sink_stream(block)
    w, h, d = s.dims
    original = np.random.default_rng(11).integers(0, 256, size=(d, h, w, 4), dtype=np.uint8)
    seen = set()
    for prf, swz in (("PRF_LDR", "rgba"), ("PRF_HDR", "bgra"), ("PRF_LDR", "ra_z1")):
        Q.check_case(product, A, contexts(block, prf, flags=0), block, s.dims, np.array(s.data), original, A.TYPE_U8, swz, what=s.name + " " + prf)
        if len(block) == 2:
            seen |= builds_of(s, prf, np.uint8, "raz1" if swz == "ra_z1" else swz)
    assert len(block) == 3 or seen == set(D.BUILDS_2D), seen
