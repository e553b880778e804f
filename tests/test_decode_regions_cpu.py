# SPDX-License-Identifier: Apache-2.0
"""astcenc_amd_decompress_regions_device (windows of compressed images, many per launch): what can be checked without a GPU.

  - tests/harness/decode_region_check.cpp: the windowed routine (decode_regions.h over the window policy of wave_decode.h), run
    by run from the host-built table, against decode_row_batch of the whole image followed by a crop, as sequential code under
    the address and undefined-behaviour sanitizers.  It would catch: a window row or column computed and stored outside the
    window; a write into pitch padding; a run that starts at block 0 instead of the first covered block; lanes dealt to the
    blocks' columns instead of the window's (the trip count); a per-row infill term that starts at the block's first row; a
    run too many or too few;
  - the table builder on hand-computed cases;
  - the ctypes structure against the C one, the argument checks that need no context, the signature;
  - the code object of the new kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "harness", "decode_region_check.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("decode_region") / "decode_region_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, HARNESS, "-o", exe], check=True)
    return exe


def test_windowed_routine_matches_decode_then_crop_on_the_host(harness):
    out = subprocess.run([harness], capture_output=True, text=True)
    assert out.returncode == 0 and re.search(r"^\d+ configurations, 0 mismatches$", out.stdout, re.M), out.stdout + out.stderr
    # six footprints x four profiles x three data types x three swizzles
    assert int(out.stdout.split()[0]) == 6 * 4 * 3 * 3


def test_table_builder_on_hand_computed_cases(harness):
    """6x6 blocks, DECODE_BATCH = 32.  Entry 0 is 230 x 50 x 2 (39 x 9 blocks a slice), entry 1 is 100 x 30 (17 x 5 blocks)."""
    out = subprocess.run([harness, "tables"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = dict(line.split(": ", 1) for line in out.stdout.strip().splitlines())

    def parse(line):
        head = re.match(r"count (\d+) total (\d+) returned (\d+) first ([\d ]+) records (.*)$", line)
        recs = [dict((k, int(v)) for k, v in re.findall(r"(\w+) (\d+)", r)) for r in re.findall(r"\[([^\]]*)\]", head.group(5))]
        return int(head.group(1)), int(head.group(2)), int(head.group(3)), [int(v) for v in head.group(4).split()], recs

    # x 6 .. 197: blocks 1 .. 32, exactly one run; y 0 .. 5: block row 0
    assert parse(lines["exactly 32 blocks"]) == (1, 1, 1, [0], [dict(bx0=1, by0=0, bz0=0, cols=32, runs_x=1, runs_xy=1, dim_x=230)])
    # x 5 .. 197: blocks 0 .. 32, two runs a row; y 5 .. 6: block rows 0 and 1
    assert parse(lines["33 blocks"]) == (1, 4, 4, [0], [dict(bx0=0, by0=0, bz0=0, cols=33, runs_x=2, runs_xy=4, dim_x=230)])
    # texel (7, 7) of slice 1: block (1, 1) of layer 1
    assert parse(lines["one block"]) == (1, 1, 1, [0], [dict(bx0=1, by0=1, bz0=1, cols=1, runs_x=1, runs_xy=1, dim_x=230)])
    # the three above, the whole of entry 0 (2 runs x 9 rows x 2 slices = 36) and the last two blocks of entry 1's last row
    count, total, returned, first, recs = parse(lines["shared entry"])
    assert (count, total, returned, first) == (5, 43, 43, [0, 1, 5, 6, 42])
    assert [r["dim_x"] for r in recs] == [230, 230, 100, 230, 100]           # regions 0, 1, 3 share entry 0; 2 and 4 entry 1
    assert recs[3] == dict(bx0=0, by0=0, bz0=0, cols=39, runs_x=2, runs_xy=18, dim_x=230)
    assert recs[4] == dict(bx0=15, by0=4, bz0=0, cols=2, runs_x=1, runs_xy=1, dim_x=100)


def test_region_structure_is_the_c_one(A, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    fields = [name for name, _ in A.DecodeRegion._fields_]
    probe = tmp_path / "probe.cpp"
    probe.write_text('#include "astcenc_amd.h"\n#include <cstddef>\n#include <cstdio>\nint main() {\n'
                     '  printf("%zu", sizeof(astcenc_amd_decode_region));\n' +
                     "".join('  printf(" %%zu", offsetof(astcenc_amd_decode_region, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(probe), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got[0] == C.sizeof(A.DecodeRegion)
    assert got[1:] == [getattr(A.DecodeRegion, f).offset for f in fields]
    assert fields == ["entry", "x", "y", "z", "size_x", "size_y", "size_z", "out", "row_pitch", "slice_pitch"]


def test_entry_point_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    fn = lib.lib.astcenc_amd_decompress_regions_device
    assert "astcenc_amd_decompress_regions_device" in A.EXPORTS_AMD
    assert fn.restype is C.c_int and len(fn.argtypes) == 6
    assert callable(lib.decompress_regions_device)
    swz = A.Swizzle(*A.SWZ_RGBA)
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    region = (A.DecodeRegion * 1)(A.DecodeRegion(0, 0, 0, 0, 1, 1, 1, None, 0, 0))
    # no regions: nothing to do, whatever else is passed
    assert fn(None, None, 0, None, 0, None) == A.SUCCESS
    assert fn(None, one, 1, region, 0, None) == A.SUCCESS
    # a null context; a count without regions
    assert fn(None, one, 1, region, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, one, 1, None, 1, None) == A.ERR_BAD_PARAM
    assert fn(None, None, 1, region, 1, None) == A.ERR_BAD_PARAM


def test_decode_region_from_a_view(A):
    torch = pytest.importorskip("torch")
    atlas = torch.zeros((3, 40, 50, 4), dtype=torch.float16)
    r = A.decode_region(2, (5, 6, 0), (20, 10, 2), atlas[1:3, 4:14, 8:28])
    assert (r.entry, r.x, r.y, r.z, r.size_x, r.size_y, r.size_z) == (2, 5, 6, 0, 20, 10, 2)
    assert r.out == atlas[1:3, 4:14, 8:28].data_ptr() and r.row_pitch == 50 * 8 and r.slice_pitch == 40 * 50 * 8
    r = A.decode_region(0, (0, 0, 0), (20, 10, 1), atlas[0, 4:14, 8:28])
    assert r.row_pitch == 50 * 8 and r.slice_pitch == 0
    r = A.decode_region(0, (1, 2, 3), (4, 5, 6), (4096, 64, 0))
    assert (r.out, r.row_pitch, r.slice_pitch) == (4096, 64, 0)
    # texels of a row that are not contiguous: every second column, a channel slice
    with pytest.raises(ValueError):
        A.decode_region(0, (0, 0, 0), (10, 10, 1), atlas[0, :10, 0:20:2])
    with pytest.raises(ValueError):
        A.decode_region(0, (0, 0, 0), (10, 10, 1), torch.zeros((10, 10, 8), dtype=torch.uint8)[:, :, ::2])


def test_regions_kernel_descriptor(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    regions = {n: d for n, d in by_short.items() if n.startswith("astc_decode_regions")}
    assert len(regions) == 1, sorted(by_short)
    (name, d), = regions.items()
    assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
    # (the decoder's scratch -- DecodeBatch -- and little more)
    assert d["group_segment_fixed_size"] <= 7040 + 256, (name, d)
    # the names the other code-object tests pick the decoder's kernels by do not match the new one
    assert not name.startswith(("astc_decompress_blocks", "astc_decompress_set"))
