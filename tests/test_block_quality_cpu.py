# SPDX-License-Identifier: Apache-2.0
"""Block quality calls (astcenc_amd_compare_blocks_device, its _hdr_ form, astcenc_amd_compare_image_set_device): what can be
checked without a GPU.

  - the argument checks that need no context, the ctypes signatures and the 32-byte block record;
  - the code objects of the astc_quality_* kernels: no scratch memory, no spills, one wavefront per workgroup -- and the
    image comparison still has its three kernels;
  - tests/harness/block_quality_check.cpp: the fused routine (the batched decoder with the comparing texel sink,
    wave_quality.h) against decode-then-compare on the host, as sequential code under the address and undefined-behaviour
    sanitizers: every texel's terms bit equal, per-block and total sums within 1e-12 relative.  It would catch: the F16
    operand compared before it is rounded to half; the U8 operand taken from the floats and not from the packed pixel; a
    missing operand clamp; a swizzle applied to the original; a per-block fold that takes the first trip only or cuts a
    block at a trip boundary; a column or texel visited twice or not at all; a record written past the run's blocks."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    L = lib.lib
    swz = A.Swizzle(*A.SWZ_RGBA)
    sums, hdr = A.ErrorSums(), A.HdrErrorSums()
    sums.texels = -1.0
    image_args = [None, 16, None, 1, 1, 1, A.TYPE_U8, A.TYPE_U8, C.byref(swz), None, 0]
    # a null context, with and without somewhere to put the sums
    assert L.astcenc_amd_compare_blocks_device(None, *image_args, None, C.byref(sums)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_device(None, *image_args, None, None) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_hdr_device(None, *image_args, -10, 10, None, C.byref(sums), C.byref(hdr)) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_hdr_device(None, *image_args, -10, 10, None, C.byref(sums), None) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_blocks_hdr_device(None, *image_args, -10, 10, None, None, C.byref(hdr)) == A.ERR_BAD_PARAM
    # no entries: nothing to do, whatever else is passed
    assert L.astcenc_amd_compare_image_set_device(None, None, 0, None, 0, None, None) == A.SUCCESS
    # entries without a context, a count without entries, entries without sums
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, swz))
    set_sums = (A.ErrorSums * 1)()
    assert L.astcenc_amd_compare_image_set_device(None, one, 1, None, 0, None, set_sums) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_image_set_device(None, None, 3, None, 0, None, set_sums) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compare_image_set_device(None, one, 1, None, 0, None, None) == A.ERR_BAD_PARAM
    # an error writes nothing
    assert sums.texels == -1.0
    # the ctypes structure is the C one: four doubles
    assert C.sizeof(A.BlockError) == 32


def test_signatures_and_exports(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    names = ("astcenc_amd_compare_blocks_device", "astcenc_amd_compare_blocks_hdr_device", "astcenc_amd_compare_image_set_device")
    for name in names:
        assert name in A.EXPORTS_AMD
        fn = getattr(lib.lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert len(lib.lib.astcenc_amd_compare_blocks_device.argtypes) == 14
    assert len(lib.lib.astcenc_amd_compare_blocks_hdr_device.argtypes) == 17
    assert len(lib.lib.astcenc_amd_compare_image_set_device.argtypes) == 7
    for method in ("compare_blocks_device", "compare_blocks_hdr_device", "compare_image_set_device"):
        assert callable(getattr(lib, method))


def test_quality_kernel_descriptors(built, A, tmp_path):
    from test_code_object import BUNDLER, READELF, kernel_descriptors
    if not (os.path.exists(BUNDLER) and os.path.exists(READELF) and shutil.which("objcopy")):
        pytest.skip("needs the ROCm LLVM tools")
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    quality = {n: d for n, d in by_short.items() if n.startswith("astc_quality_")}
    # the LDR and the HDR build of the set kernel and the finish pass
    assert len(quality) == 3 and sum(n.startswith("astc_quality_set") for n in quality) == 2 and sum(n.startswith("astc_quality_finish") for n in quality) == 1, sorted(quality)
    for name, d in quality.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["max_flat_workgroup_size"] == 64, (name, d)
    # (the decoder's scratch, the four doubles a lane hands to its block, the unorm8 table)
    for name, d in quality.items():
        if name.startswith("astc_quality_set"):
            assert d["group_segment_fixed_size"] <= 7040 + 2048 + 1024, (name, d)
    assert sum(n.startswith("astc_compare_") for n in by_short) == 3
    # the decoder's own kernels are not among the new names
    assert not any(n.startswith(("astc_decompress_blocks", "astc_decompress_set")) for n in quality)


def test_fused_routine_matches_decode_then_compare_on_the_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path / "block_quality_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"), os.path.join(ROOT, "tests", "harness", "block_quality_check.cpp"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and " 0 mismatches" in out.stdout, out.stdout + out.stderr
