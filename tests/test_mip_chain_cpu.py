# SPDX-License-Identifier: Apache-2.0
"""Mip chains without a GPU (astcenc_amd_mip_chain_layout, csrc/mip_filter.h).

  * the layout of a chain: level count, dimensions, 256-byte aligned texel offsets, block offsets and totals, for several
    footprints (3D ones on 2D images too) and all three data types; a level_count beyond the full chain, overflow, a null layout;
  * the filter header compiled with g++, bit for bit against the numpy model (tests/mip_model.py): every odd / even size up to
    9 x 9, strips, U8 linear and sRGB, F16, F32 at extreme magnitudes and of mixed sign;
  * the argument checks that need no device: a null context on every entry point."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

FILTER_MAIN = r"""
#include "mip_filter.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace astcd;

// stdin: "type srgb w h levels\n" then level 0 (RGBA rows of U8 = 0 / F16 = 1 / F32 = 2); stdout: levels 1 .. levels-1
int main()
{
	unsigned int type, srgb, w, h, levels;
	if (scanf("%u %u %u %u %u", &type, &srgb, &w, &h, &levels) != 5) return 2;
	getchar();
	const size_t tb = type == 0 ? 4 : type == 1 ? 8 : 16;
	std::vector<unsigned char> src((size_t)w * h * tb);
	if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
	double tables[MIP_SRGB_TABLE_DOUBLES];
	mip_srgb_tables_build(tables, [](double x, double y) { return std::pow(x, y); });
	for (unsigned int l = 1; l < levels; l++)
	{
		const unsigned int dx = mip_level_dim(w, 1), dy = mip_level_dim(h, 1);
		std::vector<unsigned char> dst((size_t)dx * dy * tb);
		for (unsigned int y = 0; y < dy; y++)
			for (unsigned int x = 0; x < dx; x++)
			{
				const MipTaps tx = mip_axis_taps(w, x), ty = mip_axis_taps(h, y);
				const size_t o = ((size_t)y * dx + x) * tb;
				if (type == 0)
				{
					const unsigned int v = mip_texel_u8(tx, ty, [&](unsigned int sx, unsigned int sy) {
						unsigned int p; memcpy(&p, &src[((size_t)sy * w + sx) * 4], 4); return p; }, srgb ? tables : nullptr, tables + 256);
					memcpy(&dst[o], &v, 4);
				}
				else
				{
					float out[4];
					mip_texel_float(tx, ty, [&](unsigned int sx, unsigned int sy, float v[4]) {
						const size_t i = ((size_t)sy * w + sx) * tb;
						for (int c = 0; c < 4; c++)
						{
							if (type == 1) { unsigned short hv; memcpy(&hv, &src[i + 2 * c], 2); v[c] = mip_float_from_half(hv); }
							else memcpy(&v[c], &src[i + 4 * c], 4);
						}
					}, out);
					for (int c = 0; c < 4; c++)
					{
						if (type == 1) { const unsigned short hv = mip_half_from_float(out[c]); memcpy(&dst[o + 2 * c], &hv, 2); }
						else memcpy(&dst[o + 4 * c], &out[c], 4);
					}
				}
			}
		fwrite(dst.data(), 1, dst.size(), stdout);
		src.swap(dst); w = dx; h = dy;
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def filter_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mipfilter")
    src, exe = d / "filter.cpp", d / "filter"
    src.write_text(FILTER_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _run_filter(exe, img, srgb=False, levels=0):
    """The header's chain of img ([H, W, 4]): [img, level 1, ...]."""
    h, w = img.shape[0], img.shape[1]
    n = M.full_levels(w, h) if levels == 0 else levels
    t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[img.dtype]
    inp = ("%d %d %d %d %d\n" % (t, int(srgb), w, h, n)).encode() + np.ascontiguousarray(img).tobytes()
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, at = [img], 0
    for lw, lh in M.level_dims(w, h, n)[1:]:
        size = lw * lh * 4 * img.dtype.itemsize
        out.append(np.frombuffer(r.stdout, dtype=img.dtype, count=lw * lh * 4, offset=at).reshape(lh, lw, 4))
        at += size
    assert at == len(r.stdout)
    return out


def _random(rng, w, h, kind):
    if kind == "u8":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "f16":
        return (rng.standard_normal((h, w, 4)) * 4).astype(np.float16)
    if kind == "f32-extreme":
        mag = np.float32(10.0) ** rng.integers(-45, 39, (h, w, 4)).astype(np.float32)
        sign = np.where(rng.integers(0, 2, (h, w, 4)) == 1, np.float32(-1), np.float32(1))
        v = (rng.random((h, w, 4)).astype(np.float32) + np.float32(0.5)) * mag * sign
        v[rng.random((h, w, 4)) < 0.05] = np.float32(3.4028235e38)
        v[rng.random((h, w, 4)) < 0.05] = np.float32(-0.0)
        return v.astype(np.float32)
    return (rng.standard_normal((h, w, 4)) * 100).astype(np.float32)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,srgb", [("u8", False), ("u8", True), ("f16", False), ("f32", False), ("f32-extreme", False)])
def test_filter_header_matches_numpy_model(filter_exe, kind, srgb):
    rng = np.random.default_rng(7 + len(kind) + srgb)
    sizes = [(w, h) for w in range(1, 10) for h in range(1, 10)] + [(1, 37), (45, 1), (1, 1000), (33, 17)]
    for w, h in sizes:
        img = _random(rng, w, h, kind)
        got = _run_filter(filter_exe, img, srgb)
        want = M.chain(img, srgb=srgb)
        assert len(got) == len(want) == M.full_levels(w, h)
        for i, (g, m) in enumerate(zip(got, want)):
            assert _same(g, m), (kind, srgb, (w, h), "level %d" % i)


def test_filter_rounding_cases(filter_exe):
    """Ties of the U8 mean round up; sRGB codes round trip through a constant image; F16 rounds its float32 to nearest even."""
    # 2 x 2 of (0, 1, 1, 1): mean 0.75 -> 1; (0, 0, 1, 1): 0.5 -> 1 (tie up); (0, 0, 0, 1): 0.25 -> 0
    img = np.zeros((2, 2, 4), np.uint8)
    img[0, 1, 0] = img[1, 0, 0] = img[1, 1, 0] = 1
    img[1, :, 1] = 1
    img[1, 1, 2] = 1
    got = _run_filter(filter_exe, img)[1]
    assert list(got[0, 0]) == [1, 1, 0, 0]
    assert _same(got, M.chain(img)[1])
    for c in range(256):
        img = np.full((3, 5, 4), c, np.uint8)
        for srgb in (False, True):
            assert np.all(_run_filter(filter_exe, img, srgb, 2)[1] == c), (c, srgb)
    f = np.zeros((1, 2, 4), np.float16)
    f[0, 0] = np.float16(1.0)
    f[0, 1] = np.float16(1.0009765625)          # one ulp above 1: the mean lies half way between two halves -> even
    got = _run_filter(filter_exe, f)[1]
    assert got[0, 0, 0] == np.float16(1.0) and _same(got, M.chain(f)[1])


def test_half_conversion_every_value(tmp_path):
    """mip_half_from_float / mip_float_from_half against numpy on every half and on float32 values around every half boundary."""
    src = tmp_path / "half.cpp"
    src.write_text(r"""
#include "mip_filter.h"
#include <cstdio>
#include <cstring>
#include <vector>
int main()
{
	unsigned int n;
	if (fread(&n, 4, 1, stdin) != 1) return 2;
	std::vector<float> f(n);
	if (fread(f.data(), 4, n, stdin) != n) return 3;
	for (unsigned int i = 0; i < n; i++) { unsigned short h = astcd::mip_half_from_float(f[i]); fwrite(&h, 2, 1, stdout); }
	for (unsigned int h = 0; h < 65536; h++) { float v = astcd::mip_float_from_half((unsigned short)h); fwrite(&v, 4, 1, stdout); }
	return 0;
}
""")
    exe = tmp_path / "half"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    finite = halves[np.isfinite(halves)].astype(np.float32)
    bits = finite.view(np.uint32)
    probes = np.concatenate([finite, (bits + 1).view(np.float32), (bits - 1).view(np.float32), (bits + 4096).view(np.float32),
                             (bits + 8191).view(np.float32), np.array([65519.996, 65520.0, 7e4, 1e-8, 2.0 ** -25, 2.0 ** -24 * 1.5],
                                                                      np.float32)])
    probes = probes[np.isfinite(probes)]
    inp = np.array([probes.size], np.uint32).tobytes() + probes.astype(np.float32).tobytes()
    r = subprocess.run([str(exe)], input=inp, capture_output=True, timeout=120)
    assert r.returncode == 0
    got_h = np.frombuffer(r.stdout, np.uint16, count=probes.size)
    with np.errstate(over="ignore"):
        assert np.array_equal(got_h, probes.astype(np.float16).view(np.uint16))
    got_f = np.frombuffer(r.stdout, np.float32, offset=2 * probes.size)
    fin = np.isfinite(halves)
    assert np.array_equal(got_f[fin].view(np.uint32), halves[fin].astype(np.float32).view(np.uint32))


LAYOUT_SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (255, 190), (4096, 17), (8192, 8192), (65535, 3), (0xFFFFFFFF, 1)]


@pytest.mark.parametrize("block", [(4, 4), (6, 6), (8, 5), (12, 12), (4, 4, 4), (6, 5, 5)])
def test_layout(product, A, block):
    bz = block[2] if len(block) > 2 else 1
    err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], bz, A.PRE_MEDIUM, 0)
    assert err == A.SUCCESS
    for w, h in LAYOUT_SIZES:
        for dtype, tb in ((A.TYPE_U8, 4), (A.TYPE_F16, 8), (A.TYPE_F32, 16)):
            full = M.full_levels(w, h)
            for levels in (0, 1, min(3, full), full):
                err, lay = product.mip_chain_layout(cfg, w, h, dtype, levels)
                assert err == A.SUCCESS, (w, h, levels)
                dims = M.level_dims(w, h, levels)
                assert lay.level_count == len(dims) == (full if levels == 0 else levels)
                texels = blocks = 0
                for i, (lw, lh) in enumerate(dims):
                    assert (lay.dim_x[i], lay.dim_y[i]) == (lw, lh)
                    assert lay.blocks_offset[i] == blocks
                    blocks += -(-lw // block[0]) * -(-lh // block[1]) * 16
                    if i == 0:
                        assert lay.texels_offset[0] == 0
                        continue
                    texels = (texels + 255) // 256 * 256
                    assert lay.texels_offset[i] == texels and texels % 256 == 0
                    texels += lw * lh * tb
                assert lay.texels_len == texels and lay.blocks_len == blocks
                for i in range(len(dims), A.MAX_MIP_LEVELS):
                    assert lay.dim_x[i] == 0 and lay.texels_offset[i] == 0
            assert product.mip_chain_layout(cfg, w, h, dtype, M.full_levels(w, h) + 1)[0] == A.ERR_BAD_PARAM
    # the full chain of the widest image has 32 levels; the dimensions that make no image, an unknown type, bytes beyond size_t,
    # a null layout
    assert product.mip_chain_layout(cfg, 0xFFFFFFFF, 1, A.TYPE_U8, 0)[1].level_count == 32
    assert M.full_levels(8192, 8192) == 14 and M.full_levels(1, 1) == 1 and M.full_levels(255, 190) == 8
    for w, h, t in ((0, 5, A.TYPE_U8), (5, 0, A.TYPE_U8), (5, 5, 3), (5, 5, -1), (0xFFFFFFFF, 0xFFFFFFFF, A.TYPE_F32)):
        assert product.mip_chain_layout(cfg, w, h, t, 0)[0] == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_mip_chain_layout(C.byref(cfg), 5, 5, A.TYPE_U8, 0, None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_mip_chain_layout(None, 5, 5, A.TYPE_U8, 0, C.byref(A.MipChainLayout())) == A.ERR_BAD_PARAM


def test_null_context(product, A):
    swz = A.Swizzle(*A.SWZ_RGBA)
    assert product.lib.astcenc_amd_generate_mip_chain_device(None, 0x1000, 64, 64, A.TYPE_U8, 0, 0x2000, 1 << 20, None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_compress_mip_chain_device(None, 0x1000, 64, 64, A.TYPE_U8, C.byref(swz), 0, 0x2000, 1 << 20, 0x3000,
                                                             1 << 20, None, None) == A.ERR_BAD_PARAM


def test_downsample_kernels_use_no_scratch(tmp_path, A):
    """The generation kernels in the shipped library: no scratch memory, no spills, the tail's LDS within a CU's share."""
    import shutil
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF) and shutil.which("objcopy")):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    mips = {n: d for n, d in k.items() if "astc_downsample_" in n}
    assert len(mips) == 12, sorted(mips)              # even / level / tail x U8, U8 sRGB, F16, F32
    for n, d in mips.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
        assert d["group_segment_fixed_size"] <= 64 * 1024, (n, d)
