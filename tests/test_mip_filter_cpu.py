# SPDX-License-Identifier: Apache-2.0
"""Windowed mip filters without a GPU (csrc/mip_resample.h, include/astcenc_amd.h):

  * the header's taps compiled with g++ -ffp-contract=off, bit for bit against the numpy model (tests/mip_filter_model.py):
    every source size 1 .. 300 and a sample of large odd and even ones, all kinds, both edges; the weights sum to 1 within a few
    ulp and are exactly symmetric on even sources; a tile of 16 destination rows touches at most the kernel's 48 source rows;
  * the header's per-texel routine against the model on random images: U8, U8 sRGB, F16, F32 with inf; 2D, ARRAY and VOLUME;
    widths 1, 2, 3 and odd; a constant U8 image stays constant on every level;
  * a null context on both new entry points (a bad kind or edge: tests/test_mip_filter.py, which has a device);
  * the astc_mipfilter_* kernels of the shipped library use no scratch memory, spill nothing and stay within 64 KiB of LDS."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_filter_model as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

RESAMPLE_MAIN = r"""
#include "mip_resample.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace astcd;

static double csin(double x) { return sin(x); }
static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const char* mode = argv[1];
	if (!strcmp(mode, "taps") && argc == 4)        // argv: kind s; stdin: n, n destination indices; stdout per index: first,
	{                                              // count, 0, 17 weights (zero padded)
		const int kind = atoi(argv[2]);
		const unsigned int s = (unsigned int)strtoul(argv[3], nullptr, 10);
		unsigned int n;
		if (fread(&n, 4, 1, stdin) != 1) return 3;
		std::vector<unsigned int> js(n);
		if (fread(js.data(), 4, n, stdin) != n) return 3;
		for (unsigned int j : js)
		{
			long long first = 0;
			double w[MIP_RESAMPLE_MAX_TAPS] = {};
			const unsigned int count = mip_resample_taps(kind, s, j, csin, &first, w), zero = 0;
			put(&first, 8); put(&count, 4); put(&zero, 4); put(w, sizeof(w));
		}
		return 0;
	}
	if (!strcmp(mode, "source") && argc == 4)      // argv: s edge; stdin: n, n int64 tap indices; stdout: n source texels
	{
		const unsigned int s = (unsigned int)strtoul(argv[2], nullptr, 10), edge = (unsigned int)atoi(argv[3]);
		unsigned int n;
		if (fread(&n, 4, 1, stdin) != 1) return 3;
		std::vector<long long> is(n);
		if (fread(is.data(), 8, n, stdin) != n) return 3;
		for (long long i : is) { const unsigned int v = mip_resample_source(i, s, edge); put(&v, 4); }
		return 0;
	}
	if (!strcmp(mode, "level"))                    // stdin: "kind edge type srgb array w h z\n", the level; stdout: the next level
	{
		unsigned int kind, edge, type, srgb, array, w, h, z;
		if (scanf("%u %u %u %u %u %u %u %u", &kind, &edge, &type, &srgb, &array, &w, &h, &z) != 8) return 2;
		getchar();
		const size_t tb = type == 0 ? 4 : type == 1 ? 8 : 16;
		std::vector<unsigned char> src((size_t)w * h * z * tb);
		if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
		double tables[MIP_SRGB_TABLE_DOUBLES];
		mip_srgb_tables_build(tables, [](double x, double y) { return std::pow(x, y); });
		const unsigned int dx = mip_level_dim(w, 1), dy = mip_level_dim(h, 1), dz = array ? z : mip_level_dim(z, 1);
		std::vector<unsigned char> dst((size_t)dx * dy * dz * tb);
		double wx[MIP_RESAMPLE_MAX_TAPS], wy[MIP_RESAMPLE_MAX_TAPS], wz[MIP_RESAMPLE_MAX_TAPS];
		for (unsigned int oz = 0; oz < dz; oz++)
			for (unsigned int oy = 0; oy < dy; oy++)
				for (unsigned int ox = 0; ox < dx; ox++)
				{
					MipResampleTaps tx, ty, tz;
					tx.s = w; tx.edge = edge; tx.w = wx; tx.count = mip_resample_taps((int)kind, w, ox, csin, &tx.first, wx);
					ty.s = h; ty.edge = edge; ty.w = wy; ty.count = mip_resample_taps((int)kind, h, oy, csin, &ty.first, wy);
					if (array) { tz.s = z; tz.edge = edge; tz.w = wz; tz.count = 1; tz.first = oz; wz[0] = 1.0; }
					else { tz.s = z; tz.edge = edge; tz.w = wz; tz.count = mip_resample_taps((int)kind, z, oz, csin, &tz.first, wz); }
					double vol[4];
					mip_resample_texel(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz, double v[4]) {
						const size_t i = (((size_t)sz * h + sy) * w + sx) * tb;
						if (type == 0) { unsigned int p; memcpy(&p, &src[i], 4); mip_resample_load_u8(p, srgb ? tables : nullptr, v); }
						else
						{
							float f[4];
							for (int c = 0; c < 4; c++)
							{
								if (type == 1) { unsigned short hv; memcpy(&hv, &src[i + 2 * c], 2); f[c] = mip_float_from_half(hv); }
								else memcpy(&f[c], &src[i + 4 * c], 4);
							}
							mip_resample_load_float(f, v);
						}
					}, vol);
					const size_t o = (((size_t)oz * dy + oy) * dx + ox) * tb;
					if (type == 0) { const unsigned int p = mip_resample_out_u8(vol, srgb ? tables + 256 : nullptr); memcpy(&dst[o], &p, 4); }
					else
					{
						float f[4];
						mip_resample_out_float(vol, f);
						for (int c = 0; c < 4; c++)
						{
							if (type == 1) { const unsigned short hv = mip_half_from_float(f[c]); memcpy(&dst[o + 2 * c], &hv, 2); }
							else memcpy(&dst[o + 4 * c], &f[c], 4);
						}
					}
				}
		put(dst.data(), dst.size());
		return 0;
	}
	return 2;
}
"""


@pytest.fixture(scope="module")
def resample_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mipresample")
    src, exe = d / "resample.cpp", d / "resample"
    src.write_text(RESAMPLE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _run(exe, args, data=b""):
    r = subprocess.run([exe] + [str(a) for a in args], input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return r.stdout


ROW = np.dtype([("first", "<i8"), ("count", "<u4"), ("zero", "<u4"), ("w", "<f8", (17,))])
LARGE = [4097, 8191, 16384, 65535]


def _header_taps(exe, kind, s, js):
    js = np.asarray(js, np.uint32)
    raw = _run(exe, ["taps", kind, s], np.array([len(js)], np.uint32).tobytes() + js.tobytes())
    return np.frombuffer(raw, dtype=ROW)


def _sample(d, rng):
    if d <= 300:
        return list(range(d))
    return sorted(set(list(range(40)) + list(range(d - 40, d)) + [int(j) for j in rng.integers(0, d, 200)]))


@pytest.mark.parametrize("kind", F.KINDS)
def test_taps_equal_the_model(resample_exe, kind):
    rng = np.random.default_rng(kind)
    for s in list(range(1, 301)) + LARGE:
        d = max(1, s >> 1)
        js = _sample(d, rng)
        got = _header_taps(resample_exe, kind, s, js)
        for j, g in zip(js, got):
            first, w = F.taps(kind, s, j)
            n = int(g["count"])
            assert (int(g["first"]), n) == (first, len(w)), (kind, s, j)
            assert g["w"][:n].tobytes() == np.array(w, np.float64).tobytes(), (kind, s, j)
            assert not g["w"][n:].any()
            assert n <= 17
            if s % 2 == 0:
                assert n == (8 if kind == F.MITCHELL else 12), (kind, s, j, n)
                # exactly symmetric, and every destination has the taps of j = 0 moved by 2j (the kernels' one row per even axis)
                f0, w0 = F.taps(kind, s, 0)
                assert w == w[::-1] and w == w0 and first == f0 + 2 * j
            # the weights sum to 1 within a few ulp
            total = 0.0
            for v in w:
                total += v
            assert abs(total - 1.0) < 8 * np.finfo(np.float64).eps, (kind, s, j, total)


def test_tile_rows_fit_the_kernel():
    """The kernel stages the row sums of the source rows a tile's 16 destination rows touch: at most 48 of them."""
    for kind in F.KINDS:
        for s in list(range(2, 301)) + LARGE:
            d = s >> 1
            rows = [F.taps(kind, s, j) for j in range(min(d, 64))] if s % 2 else None
            for y0 in range(0, min(d, 48), 16):
                y1 = min(y0 + 16, d) - 1
                if rows is None:
                    lo, (hf, hw) = F.taps(kind, s, y0)[0], F.taps(kind, s, y1)
                else:
                    lo, (hf, hw) = rows[y0][0], rows[y1]
                assert hf + len(hw) - lo <= 48, (kind, s, y0)


def test_source_indices(resample_exe):
    for s in (1, 2, 3, 5, 8, 17, 300, 16385):
        i = np.arange(-12, s + 12, dtype=np.int64) if s < 400 else np.concatenate([np.arange(-12, 12), np.arange(s - 12, s + 12)]).astype(np.int64)
        for edge in (F.CLAMP, F.WRAP):
            got = np.frombuffer(_run(resample_exe, ["source", s, edge], np.array([len(i)], np.uint32).tobytes() + i.tobytes()), np.uint32)
            assert [int(g) for g in got] == [F.source(int(k), s, edge) for k in i], (s, edge)


def _level(exe, kind, edge, img, mip_kind, srgb=False):
    z, h, w = img.shape[:3]
    t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[img.dtype]
    head = b"%d %d %d %d %d %d %d %d\n" % (kind, edge, t, int(srgb), int(mip_kind == F.ARRAY), w, h, z)
    raw = _run(exe, ["level"], head + np.ascontiguousarray(img).tobytes())
    dz = z if mip_kind == F.ARRAY else max(1, z >> 1)
    return np.frombuffer(raw, dtype=img.dtype).reshape(dz, max(1, h >> 1), max(1, w >> 1), 4)


def _random(dtype, shape, rng, inf=False):
    if dtype == np.uint8:
        return rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    v = (rng.standard_normal(shape + (4,)) * 4.0).astype(dtype)
    if inf:
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, size=max(1, flat.size // 50), replace=False)
        flat[pos] = np.where(rng.random(pos.size) < 0.5, np.inf, -np.inf).astype(dtype)
    return v


def _same(g, m):
    if g.shape != m.shape:
        return False
    if g.dtype == np.uint8:
        return g.tobytes() == m.tobytes()
    bits = np.uint16 if g.dtype == np.float16 else np.uint32
    return bool(((g.view(bits) == m.view(bits)) | (np.isnan(g) & np.isnan(m))).all())


SHAPES = [(F.VOLUME, (1, 1, 1)), (F.VOLUME, (1, 37, 1)), (F.VOLUME, (1, 1, 2)), (F.VOLUME, (1, 5, 3)), (F.VOLUME, (1, 19, 45)),
          (F.VOLUME, (1, 16, 32)), (F.ARRAY, (3, 9, 7)), (F.ARRAY, (6, 8, 8)), (F.VOLUME, (9, 17, 13)), (F.VOLUME, (4, 6, 3)),
          (F.VOLUME, (3, 1, 1))]


@pytest.mark.parametrize("dtype,srgb", [(np.uint8, False), (np.uint8, True), (np.float16, False), (np.float32, False)])
def test_texels_equal_the_model(resample_exe, dtype, srgb):
    rng = np.random.default_rng(3 + int(srgb) + np.dtype(dtype).itemsize)
    for kind in F.KINDS:
        for edge in (F.CLAMP, F.WRAP):
            for mip_kind, shape in SHAPES:
                img = _random(dtype, shape, rng, inf=dtype != np.uint8 and shape[1] > 8)
                got = _level(resample_exe, kind, edge, img, mip_kind, srgb)
                want = F.downsample(img, kind, edge, mip_kind, srgb)
                assert _same(got, want), (kind, edge, mip_kind, shape, dtype, srgb)


def test_constant_u8_stays_constant():
    for kind in F.KINDS:
        for edge in (F.CLAMP, F.WRAP):
            for mip_kind, shape in [(F.VOLUME, (1, 37, 23)), (F.ARRAY, (2, 12, 33)), (F.VOLUME, (5, 9, 11))]:
                img = np.empty(shape + (4,), np.uint8)
                img[...] = (7, 128, 250, 0)
                for lv in F.chain(img, mip_kind, kind, edge):
                    assert (lv == img.reshape(-1, 4)[0]).all(), (kind, edge, mip_kind, shape)


def test_null_context(product, A):
    swz = A.Swizzle(*A.SWZ_RGBA)
    flt = A.MipFilter(A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP)
    assert product.lib.astcenc_amd_generate_mip_chain_filtered_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, 0, None, C.byref(flt),
                                                                      0x2000, 1 << 20, None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_compress_mip_chain_filtered_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, C.byref(swz), 0, None,
                                                                      C.byref(flt), 0x2000, 1 << 20, 0x3000, 1 << 20, None,
                                                                      None) == A.ERR_BAD_PARAM


def test_filter_kernels_use_no_scratch(tmp_path, A):
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF)):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    mine = {n: d for n, d in k.items() if "astc_mipfilter_" in n}
    # level and tail for U8, U8 sRGB, F16 and F32
    assert len(mine) == 8, sorted(mine)
    for n, d in mine.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
        assert d["group_segment_fixed_size"] <= 65536, (n, d)
