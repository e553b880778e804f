# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_decompress_tensors_device (windows of compressed images decoded straight into tensors): what can be checked
without a GPU.

  - tests/harness/decode_tensor_check.cpp: the tensor sink and window policy (decode_tensors.h), run by run from the host-built
    table, against decode_row_batch of the whole image followed by crop, convert and place in plain C++, as sequential code
    under the address and undefined-behaviour sanitizers.  It would catch: a mirrored row or column one off; a plane, slice or
    row pitch taken in bytes or texels instead of elements; a channel stored that the format does not have; a write into
    padding or between planes; a fused multiply-add; a rounding that is not to nearest even; a NaN that keeps its payload;
  - the numpy model (tests/tensor_model.py) on hand-made bit patterns;
  - the table builder on hand-computed cases;
  - the ctypes structures against the C ones, the argument checks that need no context, tensor_region on torch views;
  - the code object of the new kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tensor_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_tensor_check.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_tensor") / "decode_tensor_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_tensor_routine_matches_decode_crop_convert_place_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # four footprints x four profiles x three data types x three swizzles x six formats (every type with both layouts)
    assert int(out.stdout.split()[0]) == 4 * 4 * 3 * 3 * 6


def test_table_builder_on_hand_computed_cases(harness):
    """6x6 blocks, DECODE_BATCH = 32.  Entry 0 is 230 x 50 x 2 (39 x 9 blocks a slice), entry 1 is 100 x 30 (17 x 5 blocks)."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(": ", 1) for line in out.stdout.strip().splitlines())

    def parse(line):
        head = re.match(r"count (\d+) total (\d+) returned (\d+) first ([\d ]+) records (.*)$", line)
        recs = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(5))]
        return int(head.group(1)), int(head.group(2)), int(head.group(3)), [int(v) for v in head.group(4).split()], recs

    # planar F16, 3 channels.  Region 0: x 6 .. 197 is blocks 1 .. 32, one run; region 1: x 5 .. 197 is blocks 0 .. 32, two runs a
    # row, y 5 .. 6 block rows 0 and 1; region 2: the last two blocks of entry 1's last row.  A column is one element
    count, total, returned, first, recs = parse(lines["planar"])
    assert (count, total, returned, first) == (3, 6, 6, [0, 1, 5])
    fmt = dict(type=1, layout=0, channels=3, x_step=1)
    assert recs[0] == dict(bx0=1, by0=0, bz0=0, cols=32, runs_x=1, runs_xy=1, dim_x=230, row=192, slice=1152, plane=1152, flags=1, **fmt)
    assert recs[1] == dict(bx0=0, by0=0, bz0=0, cols=33, runs_x=2, runs_xy=4, dim_x=230, row=200, slice=400, plane=500, flags=2, **fmt)
    assert recs[2] == dict(bx0=15, by0=4, bz0=0, cols=2, runs_x=1, runs_xy=1, dim_x=100, row=6, slice=6, plane=6, flags=0, **fmt)
    # interleaved BF16, 4 channels: the whole of entry 0 (2 runs x 9 rows x 2 slices = 36) and one texel of entry 1; a column is
    # four elements, there are no planes
    count, total, returned, first, recs = parse(lines["interleaved"])
    assert (count, total, returned, first) == (2, 37, 37, [0, 36])
    fmt = dict(type=2, layout=1, channels=4, x_step=4, plane=0)
    assert recs[0] == dict(bx0=0, by0=0, bz0=0, cols=39, runs_x=2, runs_xy=18, dim_x=230, row=920, slice=46000, flags=3, **fmt)
    assert recs[1] == dict(bx0=1, by0=1, bz0=0, cols=1, runs_x=1, runs_xy=1, dim_x=100, row=4, slice=4, flags=0, **fmt)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_model_bf16_rounds_ties_to_even():
    #               exact     below tie   tie, even   tie, odd    above tie   largest finite -> inf   -tie, odd
    bits = [0x3F800000, 0x3F807FFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0xBF818000, 0x00000001, 0x00008000, 0x00018000]
    want = [0x3F80, 0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x7F80, 0xBF82, 0x0000, 0x0000, 0x0002]
    assert M.store_bits(f32(bits), M.BF16).tolist() == want


def test_model_f16_overflow_and_subnormals():
    #       65504      65519.996 (below the tie)  65520 (tie -> inf)   -70000      2^-24       2^-25 (tie -> 0)   2^-25 + ulp   2^-14 - 2^-25 (tie -> 2^-14)   1.5 * 2^-24 (tie -> 2)
    bits = [0x477FE000, 0x477FEFFF, 0x477FF000, 0xC788B800, 0x33800000, 0x33000000, 0x33000001, 0x387FE000, 0x33C00000]
    want = [0x7BFF, 0x7BFF, 0x7C00, 0xFC00, 0x0001, 0x0000, 0x0001, 0x0400, 0x0002]
    assert M.store_bits(f32(bits), M.F16).tolist() == want


def test_model_nans_are_canonical():
    nans = f32([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFE000, 0x7FFFFFFF])
    assert M.store_bits(nans, M.F32).tolist() == [0x7FC00000] * 5
    assert M.store_bits(nans, M.F16).tolist() == [0x7E00] * 5
    assert M.store_bits(nans, M.BF16).tolist() == [0x7FC0] * 5
    # infinities are not NaNs; infinity times a zero scale is one
    assert M.store_bits(f32([0x7F800000, 0xFF800000]), M.BF16).tolist() == [0x7F80, 0xFF80]
    texels = np.zeros((1, 1, 1, 4), dtype=np.float32)
    texels[..., 0] = np.inf
    assert M.convert(texels, M.F16, 1, [0.0], [1.0]).ravel().tolist() == [0x7E00]


def test_model_keeps_subnormal_products_and_does_not_fuse():
    # 255 * 2^-140: a float32 subnormal (255 * 2^9 units of 2^-149), kept, then + 0 leaves it
    texels = np.full((1, 1, 1, 4), 255, dtype=np.uint8)
    tiny = float(f32([0x04800000])[0])                                                  # 2^-118
    assert M.convert(texels, M.F32, 1, [float(f32([0x00000200])[0])], [0.0]).ravel().tolist() == [255 * 0x200]
    assert M.convert(texels, M.F32, 1, [tiny * 2.0 ** -22], [0.0]).ravel().tolist() == [255 * 0x200]
    # two roundings: 3 * (1 + 2^-23) = 3 + 3 * 2^-23 rounds to 3 + 2^-21 (tie to even would differ from the exact sum), and
    # adding -3 gives 2^-21; a fused multiply-add would give 3 * 2^-23
    three = np.full((1, 1, 1, 4), 3, dtype=np.uint8)
    got = M.convert(three, M.F32, 1, [float(f32([0x3F800001])[0])], [-3.0]).view(np.float32).ravel()[0]
    assert got == 2.0 ** -21 and got != 3 * 2.0 ** -23


def test_model_places_planar_and_interleaved_with_flips():
    texels = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(1, 2, 3, 4)               # texel (j, i) = 12 j + 4 i + c
    one = [1.0] * 4
    zero = [0.0] * 4
    t = M.tensor(texels, M.F32, M.PLANAR, 3, one, zero).view(np.float32)
    assert t.shape == (3, 1, 2, 3) and t[1, 0].tolist() == [[1, 5, 9], [13, 17, 21]]
    t = M.tensor(texels, M.F32, M.PLANAR, 3, one, zero, M.FLIP_X).view(np.float32)
    assert t[1, 0].tolist() == [[9, 5, 1], [21, 17, 13]]
    t = M.tensor(texels, M.F32, M.INTERLEAVED, 2, one, zero, M.FLIP_Y).view(np.float32)
    assert t.shape == (1, 2, 3, 2) and t[0, 0].tolist() == [[12, 13], [16, 17], [20, 21]]
    # pitches: a 2 x 1 window into rows of 5 elements, planes of 11, from element 3
    buf = np.full(40, 0xA5A5A5A5, dtype=np.uint32)
    M.scatter(buf, 3, M.convert(texels[:, :, :1], M.F32, 2, one, zero), M.PLANAR, M.FLIP_X | M.FLIP_Y, row_pitch=5, slice_pitch=10, plane_pitch=11)
    written = {3: 12.0, 8: 0.0, 14: 13.0, 19: 1.0}
    assert {i: float(buf[i:i + 1].view(np.float32)[0]) for i in range(40) if buf[i] != 0xA5A5A5A5} == written


def test_structures_are_the_c_ones(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    pairs = [("astcenc_amd_tensor_format", A.TensorFormat), ("astcenc_amd_tensor_region", A.TensorRegion)]
    body = ""
    for cname, cls in pairs:
        body += '  printf("%%zu", sizeof(%s));\n' % cname
        body += "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f, _ in cls._fields_) + '  printf("\\n");\n'
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n' + body +
                     '  printf("%d %d %d %d %d %u %u\\n", ASTCENC_AMD_TENSOR_F32, ASTCENC_AMD_TENSOR_F16, ASTCENC_AMD_TENSOR_BF16, ASTCENC_AMD_TENSOR_PLANAR,\n'
                     "         ASTCENC_AMD_TENSOR_INTERLEAVED, ASTCENC_AMD_TENSOR_FLIP_X, ASTCENC_AMD_TENSOR_FLIP_Y);\n  return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    for line, (cname, cls) in zip(lines, pairs):
        got = [int(v) for v in line.split()]
        assert got[0] == C.sizeof(cls), cname
        assert got[1:] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    assert [f for f, _ in A.TensorFormat._fields_] == ["type", "layout", "channels", "scale", "bias"]
    assert [f for f, _ in A.TensorRegion._fields_] == ["entry", "x", "y", "z", "size_x", "size_y", "size_z", "flags", "out", "row_pitch", "slice_pitch", "plane_pitch"]
    assert [int(v) for v in lines[2].split()] == [A.TENSOR_F32, A.TENSOR_F16, A.TENSOR_BF16, A.TENSOR_PLANAR, A.TENSOR_INTERLEAVED, A.TENSOR_FLIP_X, A.TENSOR_FLIP_Y]
    assert (M.F32, M.F16, M.BF16, M.PLANAR, M.INTERLEAVED, M.FLIP_X, M.FLIP_Y) == (A.TENSOR_F32, A.TENSOR_F16, A.TENSOR_BF16, A.TENSOR_PLANAR, A.TENSOR_INTERLEAVED,
                                                                                 A.TENSOR_FLIP_X, A.TENSOR_FLIP_Y)


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_decompress_tensors_device
    assert "astcenc_amd_decompress_tensors_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 7
    assert callable(lib.decompress_tensors_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3)
    region = (A.TensorRegion * 1)(A.TensorRegion(0, 0, 0, 0, 1, 1, 1, 0, None, 0, 0, 0))
    # no regions: nothing to do, whatever else is passed
    assert fn(None, None, 0, None, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, C.byref(fmt), region, 0, None) == A.SUCCESS
    # a null context; a count without regions; a count without entries
    assert fn(None, one, 1, C.byref(fmt), region, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, C.byref(fmt), None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, C.byref(fmt), region, 1, None) == A.ERR_BAD_PARAM


def test_tensor_format_helper(A):
    f = A.tensor_format(A.TENSOR_BF16, A.TENSOR_INTERLEAVED, 3, scale=(0.5, 0.25, 2.0), bias=(1.0,))
    assert (f.type, f.layout, f.channels) == (2, 1, 3)
    assert list(f.scale) == [0.5, 0.25, 2.0, 1.0] and list(f.bias) == [1.0, 0.0, 0.0, 0.0]


def test_tensor_region_from_views(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    # [C, H, W]: one sample of a batch, then a tile of it
    r = A.tensor_region(2, (5, 6, 0), (50, 40, 1), batch[3], flip_x=True)
    assert (r.entry, r.x, r.y, r.z, r.size_x, r.size_y, r.size_z, r.flags) == (2, 5, 6, 0, 50, 40, 1, A.TENSOR_FLIP_X)
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch) == (batch[3].data_ptr(), 50, 0, 2000)
    view = batch[1, :, 4:14, 8:28]
    r = A.tensor_region(0, (0, 0, 0), (20, 10, 1), view, flip_y=True)
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch, r.flags) == (view.data_ptr(), 50, 0, 2000, A.TENSOR_FLIP_Y)
    # the first two channels of a wider tensor
    r = A.tensor_region(0, (0, 0, 0), (50, 40, 1), batch[0, :2])
    assert r.plane_pitch == 2000
    # [C, D, H, W]
    vol = torch.zeros((4, 6, 20, 30), dtype=torch.float32)
    view = vol[:, 1:3, 2:12, 3:23]
    r = A.tensor_region(1, (1, 2, 3), (20, 10, 2), view, flip_x=True, flip_y=True)
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch, r.flags) == (view.data_ptr(), 30, 600, 3600, 3)
    # [H, W, C] and [D, H, W, C]
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.bfloat16)
    view = nhwc[2, 4:14, 8:28]
    r = A.tensor_region(0, (0, 0, 0), (20, 10, 1), view, layout=A.TENSOR_INTERLEAVED)
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch) == (view.data_ptr(), 200, 0, 0)
    view = nhwc[1:4, 4:14, 8:28]
    r = A.tensor_region(0, (0, 0, 0), (20, 10, 3), view, layout=A.TENSOR_INTERLEAVED)
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch) == (view.data_ptr(), 200, 8000, 0)
    # explicit pointer and pitches
    r = A.tensor_region(0, (1, 2, 3), (4, 5, 6), (4096, 64, 0, 9000))
    assert (r.out, r.row_pitch, r.slice_pitch, r.plane_pitch) == (4096, 64, 0, 9000)


def test_tensor_region_rejects_views_the_layouts_cannot_express(A):
    torch = pytest.importorskip("torch")
    batch = torch.zeros((8, 3, 40, 50), dtype=torch.float16)
    nhwc = torch.zeros((5, 40, 50, 4), dtype=torch.float16)
    bad = [
        (batch[0, :, :, 0:40:2], (20, 40, 1), A.TENSOR_PLANAR),            # every second column
        (batch[0].permute(0, 2, 1), (40, 50, 1), A.TENSOR_PLANAR),         # transposed: columns a row apart
        (nhwc[0, :, :, :3], (50, 40, 1), A.TENSOR_INTERLEAVED),            # three channels of four: columns are not C apart
        (nhwc[0, :, :, ::2], (50, 40, 1), A.TENSOR_INTERLEAVED),           # channels that are not adjacent
        (nhwc[0].permute(2, 0, 1), (50, 40, 1), A.TENSOR_PLANAR),          # a channels-last tensor seen as planar
        (batch[0], (50, 41, 1), A.TENSOR_PLANAR),                          # not the window's shape
        (batch, (50, 40, 1), A.TENSOR_PLANAR),                             # [N, C, H, W] is no [C, D, H, W] of this window
        (batch[0, 0], (50, 40, 1), A.TENSOR_PLANAR),                       # two dimensions
    ]
    for view, size, layout in bad:
        with pytest.raises(ValueError):
            A.tensor_region(0, (0, 0, 0), size, view, layout=layout)


def test_tensors_kernel_descriptor(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    tensors = {n: d for n, d in by_short.items() if n.startswith("astc_decode_tensors")}
    assert len(tensors) >= 1, sorted(by_short)
    for name, d in tensors.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
        # (the decoder's scratch -- DecodeBatch -- and little more: the bound of the regions kernel)
        assert d["group_segment_fixed_size"] <= 7040 + 256, (name, d)
        # the names the other code-object tests pick kernels by do not match the new one
        assert not name.startswith(("astc_decode_regions", "astc_decompress_blocks", "astc_decompress_set", "astc_compare_"))
