# SPDX-License-Identifier: Apache-2.0
"""Image sets without a GPU (astcenc_amd_compress_images_device / astcenc_amd_decompress_images_device, csrc/image_set.h).

  * the entry lookup of the kernels, compiled by g++ from the very header the kernels include, against a linear scan;
  * the run-time build of the compression kernel takes the same kernel arguments as the library's own builds (the module
    launch in backend_hip.hip passes one argument array for both: a mismatch would hand the kernel garbage pointers);
  * the set decoder's descriptor: the limits of the single-image decoder;
  * the entry points' argument rules that need no context."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import oracle_libs as O  # (path set up by conftest.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LOOKUP_TEST = r"""
#include "image_set.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace astcd;

static unsigned int linear(const std::vector<unsigned int>& first, unsigned int item)
{
	unsigned int e = 0;
	while (e + 1 < first.size() && first[e + 1] <= item) e++;
	return e;
}

// every entry's first and last item, and (with `all`) every item, against the linear scan
static int check(const std::vector<unsigned int>& sizes, bool all)
{
	std::vector<unsigned int> first(sizes.size());
	unsigned int total = 0;
	for (size_t e = 0; e < sizes.size(); e++) { first[e] = total; total += sizes[e]; }
	const unsigned int count = (unsigned int)sizes.size();
	for (size_t e = 0; e < sizes.size(); e++)
	{
		const unsigned int lo = first[e], hi = first[e] + sizes[e] - 1;
		if (image_set_find(first.data(), count, lo) != e || image_set_find(first.data(), count, hi) != e)
		{
			printf("entry %zu of %u: first %u -> %u, last %u -> %u\n", e, count, lo, image_set_find(first.data(), count, lo), hi,
			       image_set_find(first.data(), count, hi));
			return 1;
		}
	}
	if (all)
		for (unsigned int i = 0; i < total; i++)
			if (image_set_find(first.data(), count, i) != linear(first, i)) { printf("item %u of %u entries\n", i, count); return 1; }
	return 0;
}

int main()
{
	int bad = 0;
	bad |= check({ 1 }, true);                         // one entry of one block
	bad |= check({ 29241 }, true);                     // one entry
	bad |= check(std::vector<unsigned int>(1000, 1), true);       // entries of a single block
	bad |= check({ 1, 1, 7, 1, 300, 1, 1, 2 }, true);
	for (unsigned int n = 1; n <= 70; n++)             // every count around the powers of two, uneven sizes
	{
		std::vector<unsigned int> s(n);
		for (unsigned int e = 0; e < n; e++) s[e] = 1 + (e * 7919u) % 13u;
		bad |= check(s, true);
	}
	{
		// 100 000 entries of random sizes: first / last of every entry, and a random sample against the scan
		std::vector<unsigned int> s(100000), first(100000);
		unsigned int rng = 12345u, total = 0;
		for (auto& v : s) { rng = rng * 1664525u + 1013904223u; v = 1 + ((rng >> 8) % ((rng >> 28) < 2 ? 4000u : 40u)); }
		bad |= check(s, false);
		for (size_t e = 0; e < s.size(); e++) { first[e] = total; total += s[e]; }
		for (int k = 0; k < 200000 && !bad; k++)
		{
			rng = rng * 1664525u + 1013904223u;
			const unsigned int item = (unsigned int)(((unsigned long long)rng * total) >> 32);
			unsigned int lo = 0, hi = (unsigned int)s.size() - 1;            // (the scan, by bisection on the prefix sums)
			while (lo < hi) { unsigned int mid = (lo + hi + 1) / 2; if (first[mid] <= item) lo = mid; else hi = mid - 1; }
			if (image_set_find(first.data(), (unsigned int)s.size(), item) != lo) { printf("item %u\n", item); bad = 1; }
		}
	}
	// the table layout: records 16-byte aligned after first[]
	for (unsigned int n = 1; n < 40; n++)
		if (image_set_records_offset(n) % 16 || image_set_records_offset(n) < image_set_first_offset() + 4ull * n) bad = 1;
	printf(bad ? "FAIL\n" : "OK\n");
	return bad;
}
"""


def test_lookup_header_against_linear_scan(tmp_path):
    src, exe = tmp_path / "lookup.cpp", tmp_path / "lookup"
    src.write_text(LOOKUP_TEST)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout


def _explicit_args(notes, name_prefix):
    """(offset, size, value_kind) of the explicit arguments of the kernel whose name starts with name_prefix, from the YAML of
    `llvm-readelf --notes` (one map per kernel; .args precedes the kernel's other keys)."""
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\n\s+\.name:\s+(\S+)", block).group(1)
        if not re.sub(r"^_ZN5astcd\d+", "", name).startswith(name_prefix):
            continue
        args_text = block.split(".args:", 1)[1].split(".group_segment_fixed_size", 1)[0]
        args = []
        for arg in re.split(r"\n\s+- ", args_text)[1:]:
            kind = re.search(r"\.value_kind:\s+(\S+)", arg).group(1)
            if kind.startswith("hidden_"):
                continue
            args.append((int(re.search(r"\.offset:\s+(\d+)", arg).group(1)), int(re.search(r"\.size:\s+(\d+)", arg).group(1)), kind))
        return args
    raise AssertionError("no kernel %s in the notes" % name_prefix)


def _library_notes(lib, tmp):
    """`llvm-readelf --notes` of every gfx950 code object in the library's fat binary (as tests/test_code_object.py unbundles it)."""
    from test_code_object import BUNDLER, TARGET
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    data = open(fat, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), data)] + [len(data)]
    out = []
    for n in range(len(starts) - 1):
        bundle, co = os.path.join(tmp, "b%d.bin" % n), os.path.join(tmp, "k%d.co" % n)
        open(bundle, "wb").write(data[starts[n]:starts[n + 1]])
        subprocess.run([BUNDLER, "--unbundle", "--type=o", "--input=" + bundle, "--targets=" + TARGET, "--output=" + co], check=True)
        out.append(subprocess.run([READELF, "--notes", co], capture_output=True, text=True, check=True).stdout)
    return "\n".join(out)


def test_run_time_build_takes_the_library_kernels_arguments(built, emu, A, tmp_path, monkeypatch):
    if not os.path.exists("/opt/rocm/lib/libhiprtc.so"):
        pytest.skip("no hipRTC on this box")
    if not os.path.exists(READELF):
        pytest.skip("no llvm-readelf")
    cache = str(tmp_path / "cache")
    monkeypatch.setenv("ASTCENC_AMD_CACHE_DIR", cache)
    from jit_builds import specialize_on_cpu as _specialize_on_cpu
    rc, name = _specialize_on_cpu((cache, A.PRF_LDR, (6, 6), A.PRE_THOROUGH, 0))
    assert rc == 0 and name.startswith("astc_compress_blocks_jit_"), (rc, name)
    (co,) = os.listdir(cache)
    jit = _explicit_args(subprocess.run([READELF, "--notes", os.path.join(cache, co)], capture_output=True, text=True, check=True).stdout,
                         "astc_compress_blocks_jit")
    lib = _explicit_args(_library_notes(A.LIB_PRODUCT, str(tmp_path)), "astc_compress_blocks_ldrEP")
    assert jit == lib, (jit, lib)
    # ... and the set table is among them: seven explicit arguments, the last one a pointer
    assert len(lib) == 7 and lib[-1][1] == 8 and lib[-1][2] == "global_buffer", lib


def test_set_decoder_descriptor(built, A, tmp_path):
    from test_code_object import kernel_descriptors
    k = kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    by_short = {re.sub(r"^_ZN5astcd\d+", "", n): d for n, d in k.items()}
    dec = next(d for n, d in by_short.items() if n.startswith("astc_decompress_set"))
    assert dec["private_segment_fixed_size"] == 0 and dec["vgpr_spill_count"] == 0, dec
    assert dec["group_segment_fixed_size"] <= 7040 and dec["vgpr_count"] <= 80 and dec["max_flat_workgroup_size"] == 64, dec


def test_entry_points_without_a_context(built, A):
    lib = A.Library(A.LIB_PRODUCT)
    L = lib.lib
    ms = C.c_float(-1.0)
    # no entries: nothing to do, whatever else is passed
    assert L.astcenc_amd_compress_images_device(None, None, 0, None, C.byref(ms)) == A.SUCCESS and ms.value == 0.0
    assert L.astcenc_amd_decompress_images_device(None, None, 0, None) == A.SUCCESS
    # entries without a context, a count without entries
    one = (A.ImageSetEntry * 1)(A.ImageSetEntry(None, None, 0, 1, 1, 1, A.TYPE_U8, A.Swizzle(*A.SWZ_RGBA)))
    assert L.astcenc_amd_compress_images_device(None, one, 1, None, None) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_decompress_images_device(None, one, 1, None) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_compress_images_device(None, None, 3, None, None) == A.ERR_BAD_PARAM
    assert L.astcenc_amd_decompress_images_device(None, None, 3, None) == A.ERR_BAD_PARAM
    # the ctypes structure is the C one: 24 bytes of pointers and length, three dimensions, the type, four swizzle words
    assert C.sizeof(A.ImageSetEntry) == 56
