# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_decompress_scaled_tensors_device on the GPU: windows of device-resident compressed images resampled into tensors.

Every case is bit for bit against the numpy model of the header's comment (tests/scaled_model.py) applied to what
astcenc_amd_decompress_regions_device writes for the window.  Every output buffer starts guard-filled and is compared whole: the
addressed elements must be the model's and every other byte the guard.  The images are the smallest at which the kernel can go
wrong: 33 blocks and three texels wide (more than one run of blocks), two block rows and one texel high, noise on a gradient
compressed by the library at -fast, one block replaced by a constant-colour block and one by a reserved block mode."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import images
import scaled_model as S
import tensor_model as M

pytestmark = pytest.mark.gpu

GUARD = 0xA5
FOOTPRINTS = {"4x4": (4, 4), "6x6": (6, 6), "10x8": (10, 8), "12x12": (12, 12)}
NP_TYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}
SCALE, BIAS = (1 / (255 * 0.229), -0.5, 3.0, 1 / 255), (-0.485 / 0.229, 0.25, 100.0, 0.0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def type_of(A, name):
    return {"u8": A.TYPE_U8, "f16": A.TYPE_F16, "f32": A.TYPE_F32}[name]


def make_stream(product, A, block, w, h, depth=1, seed=3, special=True):
    """[depth, h, w] noise on a gradient compressed at -fast; block 1 becomes a constant-colour block, block 2 a reserved mode."""
    img = np.stack([np.roll(images.noisy(w, h, seed), 11 * z, axis=1) for z in range(depth)])      # (every slice is another image)
    # (an array's stream is its slices' streams back to back)
    data = np.concatenate([product.compress(img[z], block, A.PRE_FAST) for z in range(depth)])
    b = data.reshape(-1, 16)
    assert b.shape[0] == depth * ((w + block[0] - 1) // block[0]) * ((h + block[1] - 1) // block[1])
    if special:
        b[1] = [0xFC, 0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0x34, 0x12, 0xFF, 0xFF, 0x00, 0x80, 0xCD, 0xAB]
        b[2] = 0
    return data


@pytest.fixture(scope="module")
def contexts(product, A):
    made = {}

    def get(block, profile):
        key = (tuple(block), profile)
        if key not in made:
            err, cfg = product.config_init(profile, block[0], block[1], block[2] if len(block) > 2 else 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
            assert err == 0
            err, ctx = product.context_alloc(cfg, 1)
            assert err == 0, product.error_string(err)
            made[key] = ctx
        return made[key]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


@pytest.fixture(scope="module")
def wide(product, A):
    """Per footprint: (block, (w, h), stream on the device) of the (33 block_x + 3) x (2 block_y + 1) image."""
    made = {}

    def get(name):
        if name not in made:
            bx, by = FOOTPRINTS[name]
            w, h = 33 * bx + 3, 2 * by + 1
            made[name] = ((bx, by), (w, h), dev(make_stream(product, A, (bx, by), w, h)))
        return made[name]
    return get


class Out:
    """A guard-filled device buffer for one region's tensor, tight or with padded pitches."""

    def __init__(self, out, ttype, layout, channels, padded=False, front=64):
        import torch
        ox, oy = out
        self.out, self.ttype, self.layout, self.channels, self.front, self.padded = out, ttype, layout, channels, front, padded
        self.element = 4 if ttype == M.F32 else 2
        self.row = (ox if layout == M.PLANAR else ox * channels) + (3 if padded else 0)
        self.plane = self.row * oy + (5 if padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * channels if layout == M.PLANAR else self.row * oy
        self.buf = torch.full((front + elements * self.element + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + front

    def region(self, A, entry, origin, size, flags, zero_pitches=False):
        pitches = (0, 0) if zero_pitches and not self.padded else (self.row, self.plane)
        return A.ScaledRegion(entry, origin[0], origin[1], origin[2], size[0], size[1], self.out[0], self.out[1], flags, self.ptr, *pitches)

    def want(self, texels, filt, scale, bias, flags):
        want = np.full(self.buf.numel(), GUARD, dtype=np.uint8).view(M.BITS_DTYPE[self.ttype])
        bits = S.convert(texels, filt, self.out[0], self.out[1], self.ttype, self.channels, scale, bias)
        M.scatter(want, self.front // self.element, bits, self.layout, flags, self.row, self.row * self.out[1], self.plane)
        return want

    def got(self):
        return self.buf.cpu().numpy().view(M.BITS_DTYPE[self.ttype])


def window_texels(product, A, ctx, entries, windows):
    """What astcenc_amd_decompress_regions_device writes for each (entry index, (x, y, z), (size_x, size_y)): [size_y, size_x, 4]."""
    import torch
    dtypes = {A.TYPE_U8: torch.uint8, A.TYPE_F16: torch.float16, A.TYPE_F32: torch.float32}
    outs = [torch.zeros((sy, sx, 4), dtype=dtypes[entries[e].data_type], device="cuda") for e, _, (sx, sy) in windows]
    err = product.decompress_regions_device(ctx, entries, [(e, o, (sx, sy, 1), t) for (e, o, (sx, sy)), t in zip(windows, outs)])
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


def run_and_check(product, A, ctx, entries, filt, fmt_args, cases, flip0=0, what=""):
    """cases: [(entry index, (x, y, z), (size_x, size_y), (out_x, out_y))], all in one call: flips rotate from flip0, padded and tight
    pitches alternate, tight ones as zeros or spelled out.  Returns the outputs' bits (for comparisons between calls)."""
    import torch
    ttype, layout, channels = fmt_args
    fmt = A.tensor_format(ttype, layout, channels, SCALE, BIAS)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    outs, regions = [], []
    for i, (e, origin, size, out) in enumerate(cases):
        o = Out(out, ttype, layout, channels, padded=i % 2 == 1)
        flags = (flip0 + i) & 3
        outs.append((o, flags))
        regions.append(o.region(A, e, origin, size, flags, zero_pitches=i % 4 == 0))
    err = product.decompress_scaled_tensors_device(ctx, entries, fmt, filt, regions)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    texels = window_texels(product, A, ctx, entries, [(e, o, s) for e, o, s, _ in cases])
    got_all = []
    for (o, flags), t, case in zip(outs, texels, cases):
        got, want = o.got(), o.want(t, filt, scale32, bias32, flags)
        if not np.array_equal(got, want):
            at = int(np.argwhere(got != want)[0][0])
            raise AssertionError("%s filter %d case %r flags %d%s: first differing element at %d (row %d, plane %d): got 0x%x, want 0x%x; %d differ" %
                                 (what, filt, case, flags, " padded" if o.padded else "", at - o.front // o.element, o.row, o.plane, got[at], want[at],
                                  int((got != want).sum())))
        got_all.append(got)
    return got_all


def wide_cases(block, dims):
    (bx, by), (w, h) = block, dims
    half = h // 2
    return [
        (0, (bx // 2, 1, 0), (37, h - 2), (37, h - 2)),                    # ratio 1, mid-block
        (0, (3, 0, 0), (20, half), (40, 2 * half)),                        # ratio 2
        (0, (1, 0, 0), (40, 2 * half), (20, half)),                        # ratio 1/2
        (0, (bx + 1, 2, 0), (37, 5), (23, 5)),                             # 37 -> 23 along x alone
        (0, (2, 1, 0), (23, 5), (37, 5)),                                  # 23 -> 37 along x alone
        (0, (0, 0, 0), (w, h), (1, 1)),                                    # the whole image to one element
        (0, (0, 0, 0), (w, h), (130, 5)),                                  # ... to more than 64 columns, more than 32 blocks under a row
        (0, (w // 2, h // 2, 0), (1, 1), (5, 3)),                          # one texel: everything clamps
        (0, (2 * bx - 1, by - 1, 0), (3, 3), (17, 11)),                    # 3 x 3 across a block corner, two bands
        (0, (w - bx - 3, h - by // 2 - 2, 0), (bx + 3, by // 2 + 2), (9, 7)),   # mid-block to the image's last texel
    ]


@pytest.mark.parametrize("name", list(FOOTPRINTS))
def test_windows_of_every_footprint_match_the_model(product, A, contexts, wide, name):
    block, dims, blocks = wide(name)
    ctx = contexts(block, A.PRF_LDR)
    entry = A.compressed_entry(blocks, dims, A.TYPE_U8)
    cases = wide_cases(block, dims)
    for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
        got = run_and_check(product, A, ctx, [entry], filt, (M.F16, M.PLANAR, 3), cases, flip0=filt, what=name)
        # the constant-colour block and the error block (opaque magenta under LDR) lie inside the ratio-1 window
        assert len(got) == len(cases)


@pytest.mark.parametrize("name", ["4x4", "12x12"])
def test_ratio_one_is_the_tensors_call(product, A, contexts, wide, name):
    """out = size on both axes: either filter writes bit for bit what astcenc_amd_decompress_tensors_device writes, for every data
    type (HDR profile: the F16 and F32 texels are not bytes; the reserved-mode block is NaN there)."""
    import torch
    block, (w, h), blocks = wide(name)
    ctx = contexts(block, A.PRF_HDR)
    entries = [A.compressed_entry(blocks, (w, h), type_of(A, t)) for t in ("u8", "f16", "f32")]
    fmt = A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4, SCALE, BIAS)
    origin, size = (block[0] // 2, 1, 0), (w - block[0], h - 1)
    for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
        a = torch.full((3, size[1], size[0], 4), 7.0, dtype=torch.float32, device="cuda")
        b = torch.full_like(a, 9.0)
        err = product.decompress_tensors_device(ctx, entries, fmt, [(e, origin, (size[0], size[1], 1), a[e], e == 1, e == 2) for e in range(3)])
        assert err == A.SUCCESS, product.error_string(err)
        err = product.decompress_scaled_tensors_device(ctx, entries, fmt, filt, [(e, origin, size, b[e], e == 1, e == 2) for e in range(3)])
        assert err == A.SUCCESS, product.error_string(err)
        torch.cuda.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.isnan(a[1]).any() and not np.isnan(a[1]).all()
        assert a.tobytes() == b.tobytes(), (name, filt, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def test_each_axis_alone_and_a_slice_of_an_array(product, A, contexts):
    """37 -> 23 and 23 -> 37 along y alone on a tall image (21 x 40), both axes at once on slice 2 of a 40 x 30 x 3 array."""
    block = (6, 6)
    ctx = contexts(block, A.PRF_LDR)
    tall = dev(make_stream(product, A, block, 21, 40, seed=9))
    array = dev(make_stream(product, A, block, 40, 30, depth=3, seed=20))
    entries = [A.compressed_entry(tall, (21, 40), A.TYPE_U8), A.compressed_entry(array, (40, 30, 3), A.TYPE_U8)]
    cases = [
        (0, (3, 2, 0), (5, 37), (5, 23)),
        (0, (9, 11, 0), (5, 23), (5, 37)),
        (1, (1, 2, 2), (37, 23), (23, 37)),
        (1, (2, 5, 2), (23, 23), (37, 23)),
        (1, (0, 0, 2), (40, 30), (40, 30)),
        (1, (0, 0, 1), (40, 30), (7, 3)),
    ]
    for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
        got = run_and_check(product, A, ctx, entries, filt, (M.BF16, M.INTERLEAVED, 4), cases, flip0=2, what="axes")
        # slices differ: the whole of slice 2 is not the whole of slice 1 or 0
        other = window_texels(product, A, ctx, entries, [(1, (0, 0, z), (40, 30)) for z in range(3)])
        assert not np.array_equal(other[2], other[1]) and not np.array_equal(other[2], other[0])
        assert len(got) == len(cases)


@pytest.mark.parametrize("ttype,layout", [(t, l) for t in (M.F32, M.F16, M.BF16) for l in (M.PLANAR, M.INTERLEAVED)])
def test_formats_flips_pitches_and_mixed_data_types(product, A, contexts, wide, ttype, layout):
    """Every tensor type with both layouts; channels 1 to 4; the four flip states; tight (as zeros and spelled out) and padded
    pitches; regions of a U8, an F16 and an F32 entry in one call."""
    block, (w, h), blocks = wide("6x6")
    ctx = contexts(block, A.PRF_LDR)
    entries = [A.compressed_entry(blocks, (w, h), type_of(A, t)) for t in ("u8", "f16", "f32")]
    windows = [((4, 1, 0), (70, 11), (45, 9)), ((0, 0, 0), (31, 13), (67, 17)), ((100, 3, 0), (29, 7), (29, 7)), ((w - 50, 0, 0), (50, 13), (8, 2))]
    for channels in range(1, 5):
        cases = [((i + channels) % 3, o, s, d) for i, (o, s, d) in enumerate(windows)]
        assert {c[0] for c in cases} == {0, 1, 2}
        for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
            run_and_check(product, A, ctx, entries, filt, (ttype, layout, channels), cases, flip0=channels + filt, what="formats")


def test_hdr_profile_and_an_invalid_block(product, A, contexts, wide):
    """The HDR profile with an F16 entry.  The reserved-mode block (block 2 of the first block row) decodes to NaN there: every
    output with a non-zero-weight tap in it is the canonical NaN, and at ratio 1 its neighbours -- whose only contact with it
    would be BILINEAR's zero-weight second tap -- are not."""
    block, (w, h), blocks = wide("6x6")
    ctx = contexts(block, A.PRF_HDR)
    entry = A.compressed_entry(blocks, (w, h), A.TYPE_F16)
    texels = window_texels(product, A, ctx, [entry], [(0, (0, 0, 0), (30, 13))])[0]
    nan = np.isnan(texels.astype(np.float32)).any(axis=2)
    assert nan[:6, 12:18].all() and nan.sum() == 36
    for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
        cases = [(0, (0, 0, 0), (30, 13), (30, 13)), (0, (0, 0, 0), (30, 13), (47, 20)), (0, (3, 1, 0), (27, 11), (10, 4)), (0, (6, 0, 0), (12, 6), (1, 1))]
        got = run_and_check(product, A, ctx, [entry], filt, (M.F16, M.PLANAR, 3), cases, flip0=0, what="hdr")
        # case 0: flags 0, tight from element 32: [3, 13, 30]
        ratio_one = got[0][32:32 + 3 * 13 * 30].reshape(3, 13, 30)
        assert (ratio_one[:, :6, 12:18] == 0x7E00).all() and int((ratio_one == 0x7E00).sum()) == 3 * 36
        # case 1 (padded, flipped in x): more NaNs than the block has texels -- the taps around it reach in -- but not all
        n = int((got[1] == 0x7E00).sum())
        assert 3 * 36 < n < 3 * 47 * 20
        # case 3 (padded: row pitch 4, plane pitch 9): the one output has taps in the NaN block with either filter (BILINEAR: window
        # columns 5 and 6, image columns 11 and 12, weights 1 and 1)
        assert [int(got[3][32 + 9 * c]) for c in range(3)] == [0x7E00] * 3


LIMIT_SCRIPT = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
torch.zeros(1, device="cuda:0")
import astcenc_amd as A
import scaled_model as S, tensor_model as M
import test_decode_scaled as T
gpu = A.Library(A.LIB_PRODUCT)
block, (w, h) = (6, 6), (201, 13)
err, cfg = gpu.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
err, ctx = gpu.context_alloc(cfg, 1)
assert err == 0
blocks = T.dev(T.make_stream(gpu, A, block, w, h))
entry = A.compressed_entry(blocks, (w, h), A.TYPE_U8)
bad = checked = 0
for filt in (A.WINDOW_BILINEAR, A.WINDOW_BOX):
    try:
        checked += len(T.run_and_check(gpu, A, ctx, [entry], filt, (M.F16, M.PLANAR, 3), T.wide_cases(block, (w, h)), what="limit"))
    except AssertionError as e:
        bad += 1
        print("MISMATCH", e)
gpu.context_free(ctx)
print("limit cases checked:", checked, "mismatching:", bad)
"""


def test_tiles_spanning_several_launches(product, A):
    """The 1D grid of tiles cut into launches of two (the limit is read once per process: a fresh child process): the 130 x 5
    output alone is three tiles, and the regions of a call sit anywhere among the launches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ASTCENC_AMD_DECODE_GRID_LIMIT="2")
    script = LIMIT_SCRIPT % (os.path.join(root, "astc-encoder_amd", "python"), os.path.join(root, "oracle"), os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mismatching: 0" in out.stdout and "limit cases checked: 20" in out.stdout, out.stdout[-2000:]


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts, wide):
    import torch
    block, (w, h), blocks = wide("6x6")
    ctx = contexts(block, A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((3, 40 * 40 * 4 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        # entry, x, y, z, size_x, size_y, out_x, out_y, flags, out, row_pitch, plane_pitch
        good = [A.ScaledRegion(0, 1, 2, 0, 50, 9, 30, 20, 0, out[0].data_ptr(), 0, 0), A.ScaledRegion(1, 0, 0, 0, 13, 13, 40, 40, 1, out[1].data_ptr(), 0, 0),
                A.ScaledRegion(0, 171, 3, 0, 30, 10, 30, 40, 3, out[2].data_ptr(), 0, 0)]
        entries = [A.compressed_entry(blocks, (w, h), A.TYPE_U8), A.compressed_entry(blocks, (w, h), A.TYPE_F32)]

        def call(fmt, regions, filt=A.WINDOW_BILINEAR, context=None):
            arr = (A.ImageSetEntry * 2)(*entries)
            rarr = (A.ScaledRegion * len(regions))(*regions)
            return product.lib.astcenc_amd_decompress_scaled_tensors_device(context or ctx, arr, 2, C.byref(fmt) if fmt is not None else None, filt, rarr, len(regions), None)

        def region(index, **change):
            r = [A.ScaledRegion.from_buffer_copy(g) for g in good]
            for k, v in change.items():
                setattr(r[index], k, v)
            return r

        def fmt(type=A.TENSOR_F16, layout=A.TENSOR_PLANAR, channels=3, scale=(1.0,) * 4, bias=(0.0,) * 4):
            return A.tensor_format(type, layout, channels, scale, bias)

        inf = float("inf")
        cases = [
            # the additional ones
            ("an unknown filter", fmt(), good, A.ERR_BAD_PARAM, "filter", dict(filt=2)),
            ("a negative filter", fmt(), good, A.ERR_BAD_PARAM, "filter", dict(filt=-1)),
            ("a zero window size", fmt(), region(2, size_y=0), A.ERR_BAD_PARAM, "region 2", {}),
            ("a zero output size", fmt(), region(1, out_x=0), A.ERR_BAD_PARAM, "region 1", {}),
            ("an output size above 65535", fmt(), region(0, out_y=65536), A.ERR_BAD_PARAM, "region 0", {}),
            ("a window size above 65535", fmt(), region(0, size_x=65536), A.ERR_BAD_PARAM, "region 0", {}),
            ("z outside the image", fmt(), region(1, z=1), A.ERR_BAD_PARAM, "region 1", {}),
            # shared with the tensors call
            ("a null format", None, good, A.ERR_BAD_PARAM, "format", {}),
            ("an unknown type", fmt(type=3), good, A.ERR_BAD_PARAM, "format", {}),
            ("an unknown layout", fmt(layout=2), good, A.ERR_BAD_PARAM, "format", {}),
            ("five channels", fmt(channels=5), good, A.ERR_BAD_PARAM, "format", {}),
            ("an infinite scale", fmt(scale=(1.0, inf, 1.0, 1.0)), good, A.ERR_BAD_PARAM, "channel 1", {}),
            ("unknown flag bits", fmt(), region(1, flags=4), A.ERR_BAD_PARAM, "region 1", {}),
            ("a row pitch below the output's", fmt(), region(2, row_pitch=29), A.ERR_BAD_PARAM, "region 2", {}),
            ("a plane pitch below the output's", fmt(), region(1, plane_pitch=40 * 40 - 1), A.ERR_BAD_PARAM, "region 1", {}),
            ("an interleaved row pitch below out_x * channels", fmt(layout=A.TENSOR_INTERLEAVED), region(0, row_pitch=30 * 3 - 1), A.ERR_BAD_PARAM, "region 0", {}),
            ("a pitch whose tensor overflows 64 bits", fmt(), region(1, plane_pitch=1 << 63), A.ERR_BAD_PARAM, "region 1", {}),
            ("a plane pitch with the interleaved layout", fmt(layout=A.TENSOR_INTERLEAVED), region(2, plane_pitch=1 << 20), A.ERR_BAD_PARAM, "region 2", {}),
            ("an out that is not aligned to the element", fmt(), region(1, out=out[1].data_ptr() + 1), A.ERR_BAD_PARAM, "region 1", {}),
            ("a null out", fmt(), region(2, out=None), A.ERR_BAD_CONTEXT, "region 2", {}),
            ("a window one texel outside the image", fmt(), region(2, x=172), A.ERR_BAD_PARAM, "region 2", {}),
            ("a bad entry index", fmt(), region(1, entry=2), A.ERR_BAD_PARAM, "region 1", {}),
        ]
        for what, f, regions, code, named, kw in cases:
            del logged[:]
            assert call(f, regions, **kw) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(named in m for m in logged), (what, logged)
        # More work items than 32 bits hold.  A 1 x 1 window to 65535 x 65535 is 1024 strips of 64 columns by 8192 bands of 8 rows,
        # 2^23 tiles: 512 such regions are 2^32, one too many, and the 512th is named; 511 of them fit -- the checks go on to the
        # region behind them, whose unknown flag bits are then what is reported.  (Every check runs before the launch: all regions
        # point at the one small buffer, which must keep its guard.)
        huge = A.ScaledRegion(0, 5, 5, 0, 1, 1, 65535, 65535, 0, out[0].data_ptr(), 0, 0)

        def many(n, last=None):
            arr = (A.ImageSetEntry * 2)(*entries)
            regions = [huge] * n + ([last] if last is not None else [])
            rarr = (A.ScaledRegion * len(regions))(*regions)
            f = fmt()
            return product.lib.astcenc_amd_decompress_scaled_tensors_device(ctx, arr, 2, C.byref(f), A.WINDOW_BOX, rarr, len(regions), None)

        del logged[:]
        assert many(512) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        assert any("region 511 of 512" in m and "2^32" in m for m in logged), logged
        del logged[:]
        assert many(511, A.ScaledRegion(0, 5, 5, 0, 1, 1, 4, 4, 4, out[1].data_ptr(), 0, 0)) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all())
        assert any("region 511 of 512" in m and "flags" in m for m in logged) and not any("2^32" in m for m in logged), logged
        # a context whose footprint is 3D
        del logged[:]
        assert call(fmt(), good, context=contexts((3, 3, 3), A.PRF_LDR)) == A.ERR_BAD_PARAM
        torch.cuda.synchronize()
        assert bool((out == GUARD).all()) and any("3D" in m for m in logged), logged
        # the good call is good
        assert call(fmt(), good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:, :64] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)
