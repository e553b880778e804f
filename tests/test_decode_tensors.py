# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_decompress_tensors_device on the GPU: windows of device-resident compressed images decoded straight into tensors.

The oracle is the reference library's astcenc_decompress_image of the whole stream (oracle/_ref), cropped with numpy and put
through the numpy model of the call (tests/tensor_model.py, written from the header's comment).  Every comparison is bitwise, on
the integer view of the output.  Every output buffer starts guard-filled and is compared whole: the window's elements must be the
model's and every other byte -- in front, behind, in the padding of a pitch, between planes, between the tiles of a canvas -- the
guard.  Streams and shapes are those of tests/test_decode_regions.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import images
import tensor_model as M
import test_decode_regions as R

pytestmark = pytest.mark.gpu

GUARD = R.GUARD
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# profile, the entry's data type and swizzle -> the tensor's type, layout, channels; scale and bias per channel
COMBOS = [
    ("PRF_LDR", "u8", "rgba", M.F16, M.PLANAR, 3, (1 / (255 * 0.229), 1 / (255 * 0.224), 1 / (255 * 0.225), 1.0), (-0.485 / 0.229, -0.456 / 0.224, -0.406 / 0.225, 0.0)),
    ("PRF_LDR_SRGB", "u8", "bgra", M.BF16, M.INTERLEAVED, 4, (0.0078125, -1 / 255, 1 / 3, 257.0), (-1.0, 1.0, 0.1, -40000.0)),
    ("PRF_HDR", "f16", "rgba", M.F32, M.PLANAR, 4, (1.5, -0.001, 1e-40, 3.0e34), (0.1, 2.0, 0.0, 1.0)),
    ("PRF_HDR_RGB_LDR_A", "f32", "z", M.F16, M.INTERLEAVED, 1, (7.0, 1.0, 1.0, 1.0), (-0.3, 0.0, 0.0, 0.0)),
]


def swizzle_of(A, name):
    return {"rgba": A.SWZ_RGBA, "bgra": R.BGRA(A), "z": R.ZSWZ(A)}[name]


class TensorOut:
    """A guard-filled device buffer for one window's tensor, tight or with padded pitches, and what it must hold afterwards."""

    def __init__(self, size, ttype, layout, channels, padded=False, front=64):
        import torch
        sx, sy, sz = size
        self.size, self.ttype, self.layout, self.channels, self.front, self.padded = size, ttype, layout, channels, front, padded
        self.element = 4 if ttype == M.F32 else 2
        tight_row = sx if layout == M.PLANAR else sx * channels
        self.row = tight_row + (3 if padded else 0)
        self.slice = self.row * (sy + (1 if padded else 0))
        self.plane = self.slice * sz + (5 if padded else 0) if layout == M.PLANAR else 0
        elements = self.plane * channels if layout == M.PLANAR else self.slice * sz
        self.buf = torch.full((front + elements * self.element + 64,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + front

    def region(self, A, entry, origin, flags, zero_pitches=False):
        pitches = (0, 0, 0) if zero_pitches and not self.padded else (self.row, self.slice, self.plane)
        return A.TensorRegion(entry, origin[0], origin[1], origin[2], self.size[0], self.size[1], self.size[2], flags, self.ptr, *pitches)

    def check(self, crop, scale, bias, flags, what):
        got = self.buf.cpu().numpy().view(M.BITS_DTYPE[self.ttype])
        want = np.full(self.buf.numel(), GUARD, dtype=np.uint8).view(M.BITS_DTYPE[self.ttype])
        M.scatter(want, self.front // self.element, M.convert(crop, self.ttype, self.channels, scale, bias), self.layout, flags, self.row, self.slice, self.plane)
        if not np.array_equal(got, want):
            at = int(np.argwhere(got != want)[0][0])
            raise AssertionError("%s: first differing element at %d of the tensor (row %d, slice %d, plane %d): got 0x%x, want 0x%x; %d differ" %
                                 (what, at - self.front // self.element, self.row, self.slice, self.plane, got[at], want[at], int((got != want).sum())))


def run_and_check(product, A, ctx, entry, whole, windows, combo, flip0=0, stream=None, what=""):
    """All `windows` of one entry in one call with the format of `combo`: each once tight (pitches 0 or spelled out, alternating)
    and once padded, the flips rotating through the four states from window to window, starting at flip0."""
    import torch
    ttype, layout, channels, scale, bias = combo[3:]
    fmt = A.tensor_format(ttype, layout, channels, scale, bias)
    outs, regions = [], []
    for i, (origin, size) in enumerate(windows):
        flags = (flip0 + i) & 3
        for padded in (False, True):
            o = TensorOut(size, ttype, layout, channels, padded)
            outs.append((o, origin, size, flags))
            regions.append(o.region(A, 0, origin, flags, zero_pitches=i % 2 == 0))
    err = product.decompress_tensors_device(ctx, [entry], fmt, regions, stream)
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    # (the model sees exactly the float32 values the C structure holds)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    for o, origin, size, flags in outs:
        o.check(R.crop_of(whole, origin, size), scale32, bias32, flags, "%s window %r %r flags %d%s" % (what, origin, size, flags, " padded" if o.padded else ""))
    return len(outs)


oracle = R.oracle
contexts = R.contexts


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_hand_picked_windows_match_the_model_of_the_cropped_reference(product, A, oracle, contexts, shape):
    """Every footprint and image of the regions test; the hand-picked windows -- one texel, inside one block, mid-block to mid-block
    across the 32-block run boundary, wider than 64 texels, the whole image, the partial last block row and column, two slices --
    with each of the four combinations, each window tight and padded, every combination with all four flip states."""
    block, dims = R.SHAPES[shape]
    data = R.random_stream(dims, block, 40 + len(shape))
    blocks = R.dev(data)
    windows = R.hand_picked(dims, block) + [((2 * block[0], 0, 0), (block[0], block[1], 1))]          # ... and exactly one block
    for n, combo in enumerate(COMBOS):
        prf, t, s = combo[:3]
        profile, swz = getattr(A, prf), swizzle_of(A, s)
        whole = oracle(shape, data, dims, block, profile, t, swz)
        entry = A.compressed_entry(blocks, dims, R.type_of(A, t), swz)
        run_and_check(product, A, contexts(block, profile), entry, whole, windows, combo, flip0=n, what="%s %s %s %s" % (shape, prf, t, s))
    # the HDR stream has error blocks, whose texels are NaN: they must have come out canonical (the model says so; make sure the
    # case occurred)
    assert np.isnan(oracle(shape, data, dims, block, A.PRF_HDR, "f16", A.SWZ_RGBA).astype(np.float32)).any()


def test_crops_into_a_training_batch_and_tiles_into_a_canvas(product, A, oracle, contexts):
    """The loader case: 16 random 32 x 32 crops of two entries into one [16, 3, 32, 32] fp16 tensor, ImageNet mean and deviation
    folded into scale and bias, odd samples mirrored -- equal to the regions call into [16, 32, 32, 4] u8 followed by the model.
    Then tiles into views of a larger [3, 64, 96] canvas, pitches from the strides; the rest of the canvas keeps its guard."""
    import torch
    block = (6, 6, 1)
    dims = [R.SHAPES["6x6"][1], (45, 70, 1)]
    streams = [R.random_stream(d, block, 40 + n) for n, d in enumerate(dims)]
    blocks = [R.dev(s) for s in streams]               # (an entry holds a pointer, not the tensor)
    entries = [A.compressed_entry(b, d, A.TYPE_U8) for b, d in zip(blocks, dims)]
    ctx = contexts(block, A.PRF_LDR)
    scale = [1.0 / (255.0 * s) for s in IMAGENET_STD]
    bias = [-m / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, scale, bias)
    scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
    rng = np.random.default_rng(11)
    crops = []
    for i in range(16):
        e = int(rng.integers(0, 2))
        crops.append((e, (int(rng.integers(0, dims[e][0] - 32 + 1)), int(rng.integers(0, dims[e][1] - 32 + 1)), 0)))
    assert {e for e, _ in crops} == {0, 1}

    rgba = torch.full((16, 32, 32, 4), GUARD, dtype=torch.uint8, device="cuda")
    err = product.decompress_regions_device(ctx, entries, [(e, o, (32, 32, 1), rgba[i]) for i, (e, o) in enumerate(crops)])
    assert err == A.SUCCESS, product.error_string(err)
    batch = torch.full((16, 3, 32, 32), -23131, dtype=torch.int16, device="cuda").view(torch.float16)            # 0xA5A5
    err = product.decompress_tensors_device(ctx, entries, fmt, [(e, o, (32, 32, 1), batch[i], i % 2 == 1) for i, (e, o) in enumerate(crops)])
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    texels = rgba.cpu().numpy()
    want = np.stack([M.tensor(texels[i][None], M.F16, M.PLANAR, 3, scale32, bias32, M.FLIP_X if i % 2 else 0)[:, 0] for i in range(16)])
    got = batch.view(torch.int16).cpu().numpy().view(np.uint16)
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    # (what the numbers mean: the mirrored sample is the plain one read right to left)
    plain = M.tensor(texels[1][None], M.F16, M.PLANAR, 3, scale32, bias32)[:, 0]
    assert np.array_equal(got[1], plain[:, :, ::-1])

    canvas = torch.full((3, 64, 96), -23131, dtype=torch.int16, device="cuda").view(torch.float16)
    # entry, origin, size, (row, column) of the tile in the canvas, flip_x, flip_y
    tiles = [(0, (3, 2, 0), (40, 30, 1), (1, 5), False, False), (0, (190, 18, 0), (40, 32, 1), (32, 56), True, True),
             (1, (0, 0, 0), (45, 33, 1), (31, 0), False, True), (1, (13, 60, 0), (32, 10, 1), (0, 50), True, False)]
    err = product.decompress_tensors_device(ctx, entries, fmt, [(e, o, s, canvas[:, y0:y0 + s[1], x0:x0 + s[0]], fx, fy) for e, o, s, (y0, x0), fx, fy in tiles])
    assert err == A.SUCCESS, product.error_string(err)
    torch.cuda.synchronize()
    wholes = [oracle("loader-%d" % n, streams[n], dims[n], block, A.PRF_LDR, "u8", A.SWZ_RGBA) for n in range(2)]
    want = np.full((3, 64, 96), 0xA5A5, dtype=np.uint16)
    for e, origin, size, (y0, x0), fx, fy in tiles:
        want[:, y0:y0 + size[1], x0:x0 + size[0]] = M.tensor(R.crop_of(wholes[e], origin, size), M.F16, M.PLANAR, 3, scale32, bias32,
                                                             (M.FLIP_X if fx else 0) | (M.FLIP_Y if fy else 0))[:, 0]
    got = canvas.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), int((got != want).sum())


def test_identity_format_writes_what_the_regions_call_writes(product, ref, A, contexts):
    """Four interleaved F32 channels, scale 1, bias 0, no flips, of an F32 entry: the regions call's bytes (a stream the product
    compressed: no error blocks, so no NaN whose payload the tensor call would canonicalise)."""
    import torch
    block, (w, h) = (6, 6, 1), (230, 50)
    data = product.compress(images.noisy(w, h, 21), block, A.PRE_FASTEST)
    ctx = contexts(block, A.PRF_LDR)
    blocks = R.dev(data)
    entry = A.compressed_entry(blocks, (w, h), A.TYPE_F32)
    fmt = A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4)
    for origin, size in [((0, 0, 0), (w, h, 1)), ((7, 3, 0), (200, 41, 1))]:
        a = torch.full((size[1], size[0], 4), 7.0, dtype=torch.float32, device="cuda")
        b = torch.full_like(a, 9.0)
        assert product.decompress_regions_device(ctx, [entry], [(0, origin, size, a)]) == A.SUCCESS
        assert product.decompress_tensors_device(ctx, [entry], fmt, [(0, origin, size, b)]) == A.SUCCESS
        torch.cuda.synchronize()
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert not np.isnan(a).any()
        assert a.tobytes() == b.tobytes()


def test_on_a_torch_stream(product, A, oracle, contexts):
    import torch
    block, dims = R.SHAPES["6x6"]
    data = R.random_stream(dims, block, 40 + len("6x6"))
    whole = oracle("6x6", data, dims, block, A.PRF_LDR, "u8", A.SWZ_RGBA)
    blocks = R.dev(data)
    entry = A.compressed_entry(blocks, dims, A.TYPE_U8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run_and_check(product, A, contexts(block, A.PRF_LDR), entry, whole, R.hand_picked(dims, block), COMBOS[0], flip0=1, stream=side, what="side stream")


def test_bad_arguments_write_nothing_and_name_the_index(product, A, contexts):
    import torch
    block, dims = R.SHAPES["6x6"]
    w, h, _ = dims
    blocks = R.dev(R.random_stream(dims, block, 1))
    ctx = contexts(block, A.PRF_LDR)
    logged = []
    log_cb = C.CFUNCTYPE(None, C.c_char_p)(lambda m: logged.append(m.decode()))
    product.lib.astcenc_amd_set_log_callback.argtypes = [C.c_void_p]
    product.lib.astcenc_amd_set_log_callback(C.cast(log_cb, C.c_void_p))
    try:
        out = torch.full((3, 40 * 40 * 4 * 4 + 64), GUARD, dtype=torch.uint8, device="cuda")
        good = [A.TensorRegion(0, 1, 2, 0, 30, 20, 1, 0, out[0].data_ptr(), 0, 0, 0), A.TensorRegion(1, 0, 0, 0, 40, 40, 1, 1, out[1].data_ptr(), 0, 0, 0),
                A.TensorRegion(0, 200, 10, 0, 30, 40, 1, 3, out[2].data_ptr(), 0, 0, 0)]
        entries = [A.compressed_entry(blocks, (w, h), A.TYPE_U8), A.compressed_entry(blocks, (w, h), A.TYPE_F32)]

        def call(fmt, regions):
            arr = (A.ImageSetEntry * 2)(*entries)
            rarr = (A.TensorRegion * len(regions))(*regions)
            return product.lib.astcenc_amd_decompress_tensors_device(ctx, arr, 2, C.byref(fmt) if fmt is not None else None, rarr, len(regions), None)

        def region(index, **change):
            r = [A.TensorRegion.from_buffer_copy(g) for g in good]
            for k, v in change.items():
                setattr(r[index], k, v)
            return r

        def fmt(type=A.TENSOR_F16, layout=A.TENSOR_PLANAR, channels=3, scale=(1.0,) * 4, bias=(0.0,) * 4):
            return A.tensor_format(type, layout, channels, scale, bias)

        inf, nan = float("inf"), float("nan")
        cases = [
            ("a null format", None, good, A.ERR_BAD_PARAM, "format"),
            ("an unknown type", fmt(type=3), good, A.ERR_BAD_PARAM, "format"),
            ("a negative type", fmt(type=-1), good, A.ERR_BAD_PARAM, "format"),
            ("an unknown layout", fmt(layout=2), good, A.ERR_BAD_PARAM, "format"),
            ("no channels", fmt(channels=0), good, A.ERR_BAD_PARAM, "format"),
            ("five channels", fmt(channels=5), good, A.ERR_BAD_PARAM, "format"),
            ("an infinite scale", fmt(scale=(1.0, inf, 1.0, 1.0)), good, A.ERR_BAD_PARAM, "channel 1"),
            ("a NaN bias", fmt(bias=(0.0, 0.0, nan, 0.0)), good, A.ERR_BAD_PARAM, "channel 2"),
            ("unknown flag bits", fmt(), region(1, flags=4), A.ERR_BAD_PARAM, "region 1"),
            ("a row pitch below tight", fmt(), region(2, row_pitch=29), A.ERR_BAD_PARAM, "region 2"),
            ("a slice pitch below tight", fmt(), region(0, slice_pitch=30 * 20 - 1), A.ERR_BAD_PARAM, "region 0"),
            ("a plane pitch below tight", fmt(), region(1, plane_pitch=40 * 40 - 1), A.ERR_BAD_PARAM, "region 1"),
            ("an interleaved row pitch below size_x * channels", fmt(layout=A.TENSOR_INTERLEAVED), region(0, row_pitch=30 * 3 - 1), A.ERR_BAD_PARAM, "region 0"),
            ("a pitch whose tensor overflows 64 bits", fmt(), region(1, plane_pitch=1 << 63), A.ERR_BAD_PARAM, "region 1"),
            ("a plane pitch with the interleaved layout", fmt(layout=A.TENSOR_INTERLEAVED), region(2, plane_pitch=1 << 20), A.ERR_BAD_PARAM, "region 2"),
            ("an out that is not aligned to the element", fmt(), region(1, out=out[1].data_ptr() + 1), A.ERR_BAD_PARAM, "region 1"),
            ("... to a four-byte element", fmt(type=A.TENSOR_F32), region(0, out=out[0].data_ptr() + 2), A.ERR_BAD_PARAM, "region 0"),
            ("a null out", fmt(), region(2, out=None), A.ERR_BAD_CONTEXT, "region 2"),
            # carried over from the regions call
            ("a window one texel outside the image", fmt(), region(2, x=201), A.ERR_BAD_PARAM, "region 2"),
            ("a zero size", fmt(), region(2, size_y=0), A.ERR_BAD_PARAM, "region 2"),
            ("a bad entry index", fmt(), region(1, entry=2), A.ERR_BAD_PARAM, "region 1"),
        ]
        for what, f, regions, code, named in cases:
            del logged[:]
            assert call(f, regions) == code, what
            torch.cuda.synchronize()
            assert bool((out == GUARD).all()), what
            assert any(named in m for m in logged), (what, logged)
        # a non-finite factor of a channel the format does not use is not looked at; the good call is good
        assert call(fmt(scale=(1.0, 1.0, 1.0, nan)), good) == A.SUCCESS
        torch.cuda.synchronize()
        assert not bool((out[:, :64] == GUARD).all())
    finally:
        product.lib.astcenc_amd_set_log_callback(None)


LIMIT_SCRIPT = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np, torch
torch.zeros(1, device="cuda:0")
import astcenc_amd as A, oracle_libs as O
import test_decode_regions as R
import test_decode_tensors as T
gpu, ref = A.Library(A.LIB_PRODUCT), A.Library(O.LIB_REF_NONE)
bad = checked = 0
for n, shape in enumerate(("6x6", "3x3x3", "6x6-array")):
    block, dims = R.SHAPES[shape]
    data = R.random_stream(dims, block, 9)
    combo = T.COMBOS[n]
    prf, t, s = combo[:3]
    swz = T.swizzle_of(A, s)
    whole = R.reference_decode(ref, A, data, dims, block, getattr(A, prf), R.NP_TYPES[t], swz)
    err, cfg = gpu.config_init(getattr(A, prf), block[0], block[1], block[2], A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
    err, ctx = gpu.context_alloc(cfg, 1)
    assert err == 0
    blocks = R.dev(data)
    try:
        checked += T.run_and_check(gpu, A, ctx, A.compressed_entry(blocks, dims, R.type_of(A, t), swz), whole, R.hand_picked(dims, block), combo, flip0=n, what=shape)
    except AssertionError as e:
        bad += 1
        print("MISMATCH", e)
    gpu.context_free(ctx)
print("limit cases checked:", checked, "mismatching:", bad)
"""


def test_runs_spanning_several_launches(product, ref, A):
    """The 1D grid of runs cut into launches of seven (the limit is read once per process: a fresh child process): the whole
    image alone is 18 runs on 6x6, and the windows of a call sit anywhere among the launches."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ASTCENC_AMD_DECODE_GRID_LIMIT="7")
    script = LIMIT_SCRIPT % (os.path.join(root, "astc-encoder_amd", "python"), os.path.join(root, "oracle"), os.path.join(root, "tests"))
    out = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "mismatching: 0" in out.stdout and "limit cases checked: 0" not in out.stdout, out.stdout[-2000:]
