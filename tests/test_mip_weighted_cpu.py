# SPDX-License-Identifier: Apache-2.0
"""Alpha-weighted mip filtering without a GPU (csrc/mip_weighted.h, include/astcenc_amd.h):

  * the header compiled with g++ -ffp-contract=off, bit for bit against the numpy model (tests/mip_weighted_model.py): every
    source size x, y, z in 1 .. 7 as a VOLUME and as an ARRAY, U8, U8 sRGB, F16 and F32, the box and the three windowed
    filters with both edges, on inputs with alpha 0 in whole regions, alpha 0 in whole footprints, random alpha, and for floats
    negative and infinite alpha;
  * properties of the model itself: channel 3 is the plain model's; WEIGHT_NONE is the plain model; a constant colour under
    random alpha stays that colour; an opaque red disc on transparent green keeps R = 255, G = 0 wherever alpha > 0, for every
    filter, and texels without alpha weight equal the plain chain's;
  * the astc_mipw_* kernels of the shipped library use no scratch memory, spill nothing and stay within 64 KiB of LDS;
  * both entry points are exported, declared, and refuse a null context."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_filter_model as F  # noqa: E402
import mip_weighted_model as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

WEIGHTED_MAIN = r"""
#include "mip_weighted.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace astcd;

static double csin(double x) { return sin(x); }

// stdin: any number of "filter edge type srgb array w h z\n" + the level; stdout: the next level of each, weighted by alpha
int main()
{
	double tables[MIP_SRGB_TABLE_DOUBLES];
	mip_srgb_tables_build(tables, [](double x, double y) { return std::pow(x, y); });
	unsigned int kind, edge, type, srgb, array, w, h, z;
	while (scanf("%u %u %u %u %u %u %u %u", &kind, &edge, &type, &srgb, &array, &w, &h, &z) == 8)
	{
		getchar();
		const size_t tb = type == 0 ? 4 : type == 1 ? 8 : 16;
		std::vector<unsigned char> src((size_t)w * h * z * tb);
		if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
		const unsigned int dx = mip_level_dim(w, 1), dy = mip_level_dim(h, 1), dz = array ? z : mip_level_dim(z, 1);
		std::vector<unsigned char> dst((size_t)dx * dy * dz * tb);
		auto texel_u8 = [&](unsigned int sx, unsigned int sy, unsigned int sz) {
			unsigned int p;
			memcpy(&p, &src[(((size_t)sz * h + sy) * w + sx) * 4], 4);
			return p;
		};
		auto texel_float = [&](unsigned int sx, unsigned int sy, unsigned int sz, float f[4]) {
			const size_t i = (((size_t)sz * h + sy) * w + sx) * tb;
			for (int c = 0; c < 4; c++)
			{
				if (type == 1) { unsigned short hv; memcpy(&hv, &src[i + 2 * c], 2); f[c] = mip_float_from_half(hv); }
				else memcpy(&f[c], &src[i + 4 * c], 4);
			}
		};
		auto put_float = [&](size_t o, const float f[4]) {
			for (int c = 0; c < 4; c++)
			{
				if (type == 1) { const unsigned short hv = mip_half_from_float(f[c]); memcpy(&dst[o + 2 * c], &hv, 2); }
				else memcpy(&dst[o + 4 * c], &f[c], 4);
			}
		};
		double wx[MIP_RESAMPLE_MAX_TAPS], wy[MIP_RESAMPLE_MAX_TAPS], wz[MIP_RESAMPLE_MAX_TAPS];
		for (unsigned int oz = 0; oz < dz; oz++)
			for (unsigned int oy = 0; oy < dy; oy++)
				for (unsigned int ox = 0; ox < dx; ox++)
				{
					const size_t o = (((size_t)oz * dy + oy) * dx + ox) * tb;
					if (kind == 0)
					{
						const MipTaps tx = mip_axis_taps(w, ox), ty = mip_axis_taps(h, oy), tz = array ? mip_axis_taps(1, 0) : mip_axis_taps(z, oz);
						const unsigned int z0 = array ? oz : 0;
						if (type == 0)
						{
							const unsigned int p = mip_texel_u8_3d_weighted(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz) {
								return texel_u8(sx, sy, z0 + sz); }, srgb ? tables : nullptr, srgb ? tables + 256 : nullptr);
							memcpy(&dst[o], &p, 4);
						}
						else
						{
							float f[4];
							mip_texel_float_3d_weighted(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz, float v[4]) {
								texel_float(sx, sy, z0 + sz, v); }, f);
							put_float(o, f);
						}
						continue;
					}
					MipResampleTaps tx, ty, tz;
					tx.s = w; tx.edge = edge; tx.w = wx; tx.count = mip_resample_taps((int)kind, w, ox, csin, &tx.first, wx);
					ty.s = h; ty.edge = edge; ty.w = wy; ty.count = mip_resample_taps((int)kind, h, oy, csin, &ty.first, wy);
					if (array) { tz.s = z; tz.edge = edge; tz.w = wz; tz.count = 1; tz.first = oz; wz[0] = 1.0; }
					else { tz.s = z; tz.edge = edge; tz.w = wz; tz.count = mip_resample_taps((int)kind, z, oz, csin, &tz.first, wz); }
					double vol[7];
					mip_resample_texel_weighted(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz, double v[7]) {
						if (type == 0) mip_resample_load_u8_weighted(texel_u8(sx, sy, sz), srgb ? tables : nullptr, v);
						else
						{
							float f[4];
							texel_float(sx, sy, sz, f);
							mip_resample_load_float_weighted(f, v);
						}
					}, vol);
					if (type == 0) { const unsigned int p = mip_resample_out_u8_weighted(vol, srgb ? tables + 256 : nullptr); memcpy(&dst[o], &p, 4); }
					else
					{
						float f[4];
						mip_resample_out_float_weighted(vol, f);
						put_float(o, f);
					}
				}
		fwrite(dst.data(), 1, dst.size(), stdout);
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def weighted_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mipweighted")
    src, exe = d / "weighted.cpp", d / "weighted"
    src.write_text(WEIGHTED_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _levels(exe, jobs):
    """jobs: [(filter, edge, img, mip_kind, srgb)] -> the next level of each from one run of the header's program."""
    data, shapes = [], []
    for kind, edge, img, mip_kind, srgb in jobs:
        z, h, w = img.shape[:3]
        t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[img.dtype]
        data.append(b"%d %d %d %d %d %d %d %d\n" % (kind, edge, t, int(srgb), int(mip_kind == W.ARRAY), w, h, z))
        data.append(np.ascontiguousarray(img).tobytes())
        shapes.append((img.dtype, (z if mip_kind == W.ARRAY else max(1, z >> 1), max(1, h >> 1), max(1, w >> 1), 4)))
    r = subprocess.run([exe], input=b"".join(data), capture_output=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out, at = [], 0
    for dtype, shape in shapes:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(r.stdout[at:at + n], dtype=dtype).reshape(shape))
        at += n
    assert at == len(r.stdout)
    return out


def _same(g, m):
    if g.shape != m.shape:
        return False
    if g.dtype == np.uint8:
        return g.tobytes() == m.tobytes()
    bits = np.uint16 if g.dtype == np.float16 else np.uint32
    return bool(((g.view(bits) == m.view(bits)) | (np.isnan(g) & np.isnan(m))).all())


def _input(dtype, shape, pattern, rng):
    """A [Z, H, W, 4] level: `pattern` 0 alpha 0 in whole regions (the low half of every axis that has one), 1 alpha 0 in whole
    footprints (random 3^3 cells), 2 random alpha with half of it 0, 3 (floats) negative and infinite alphas among them."""
    z, h, w = shape
    if dtype == np.uint8:
        v = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    else:
        v = (rng.random(shape + (4,)) * 1.4 - 0.1).astype(dtype)
        v[..., 3] = np.abs(v[..., 3])
    a = v[..., 3]
    if pattern == 0:
        a[:max(1, z // 2), :max(1, h // 2), :max(1, w // 2)] = 0
        if rng.random() < 0.5:
            a[:, :, : (w + 1) // 2] = 0
    elif pattern == 1:
        cells = rng.random(((z + 2) // 3, (h + 2) // 3, (w + 2) // 3)) < 0.5
        a[np.repeat(np.repeat(np.repeat(cells, 3, 0), 3, 1), 3, 2)[:z, :h, :w]] = 0
    elif pattern == 2:
        a[rng.random(shape) < 0.5] = 0
    else:
        r = rng.random(shape)
        a[r < 0.25] = 0
        a[(r >= 0.25) & (r < 0.4)] *= -1
        a[(r >= 0.4) & (r < 0.47)] = np.inf
        a[(r >= 0.47) & (r < 0.5)] = -np.inf
    return v


FILTERS = [(W.BOX, W.CLAMP)] + [(k, e) for k in F.KINDS for e in (W.CLAMP, W.WRAP)]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
@pytest.mark.parametrize("kind,edge", FILTERS, ids=["f%d-e%d" % f for f in FILTERS])
def test_texels_equal_the_model(weighted_exe, kind, edge, name, dtype, srgb):
    rng = np.random.default_rng(1000 * kind + 100 * edge + np.dtype(dtype).itemsize + int(srgb))
    jobs = []
    n = 0
    for z in range(1, 8):
        for h in range(1, 8):
            for w in range(1, 8):
                # every pattern on every size, as a VOLUME or an ARRAY in turn (a depth of 1 is both)
                for pattern in range(3 if dtype == np.uint8 else 4):
                    n += 1
                    jobs.append((kind, edge, _input(dtype, (z, h, w), pattern, rng), W.VOLUME if n % 3 else W.ARRAY, srgb))
    got = _levels(weighted_exe, jobs)
    for (_, _, img, mip_kind, _), g in zip(jobs, got):
        want = W.downsample(img, mip_kind, kind, edge, W.ALPHA, srgb)
        assert _same(g, want), (kind, edge, mip_kind, img.shape, dtype, srgb, img.tolist(), g.tolist(), want.tolist())


def _images():
    rng = np.random.default_rng(5)
    out = []
    for dtype in (np.uint8, np.float16, np.float32):
        for mip_kind, shape in [(W.VOLUME, (1, 37, 23)), (W.ARRAY, (3, 12, 20)), (W.VOLUME, (5, 9, 7))]:
            out.append((mip_kind, _input(dtype, shape, 2, rng)))
            out.append((mip_kind, _input(dtype, shape, 0, rng)))
    return out


def test_channel_3_is_the_plain_filters():
    for mip_kind, img in _images():
        for kind, edge in FILTERS:
            for srgb in ((False, True) if img.dtype == np.uint8 else (False,)):
                plain = F.chain(img, mip_kind, kind, edge, srgb=srgb)
                got = W.chain(img, mip_kind, kind, edge, W.ALPHA, srgb=srgb)
                assert len(got) == len(plain)
                for g, p in zip(got, plain):
                    assert g.shape == p.shape and g[..., 3].tobytes() == p[..., 3].tobytes(), (mip_kind, img.shape, kind, edge, srgb)


def test_weight_none_is_the_plain_model():
    for mip_kind, img in _images():
        for kind, edge in FILTERS:
            plain = F.chain(img, mip_kind, kind, edge)
            got = W.chain(img, mip_kind, kind, edge, W.NONE)
            assert [g.tobytes() for g in got] == [p.tobytes() for p in plain]


def test_constant_colour_stays_constant():
    """Box, linear U8: (2 c SA + SA) // (2 SA) = c, and a footprint without alpha keeps the plain mean of c, which is c."""
    rng = np.random.default_rng(6)
    for mip_kind, shape in [(W.VOLUME, (1, 23, 37)), (W.VOLUME, (1, 64, 64)), (W.VOLUME, (7, 9, 5))]:
        img = np.empty(shape + (4,), np.uint8)
        img[..., :3] = (7, 128, 250)
        img[..., 3] = rng.integers(0, 256, shape, dtype=np.uint8)
        img[..., 3][rng.random(shape) < 0.5] = 0
        for lv in W.chain(img, mip_kind, W.BOX, W.CLAMP, W.ALPHA):
            assert (lv[..., :3] == (7, 128, 250)).all(), (mip_kind, shape)


def _disc():
    y, x = np.mgrid[0:128, 0:128]
    inside = (x - 63.5) ** 2 + (y - 63.5) ** 2 < 50.0 ** 2
    img = np.zeros((1, 128, 128, 4), np.uint8)
    img[0, inside] = (255, 0, 0, 255)
    img[0, ~inside] = (0, 255, 0, 0)
    return img


def test_disc_has_no_fringe():
    img = _disc()
    for kind, edge in FILTERS:
        plain = F.chain(img, W.VOLUME, kind, edge)
        got = W.chain(img, W.VOLUME, kind, edge, W.ALPHA)
        fringe = sum(int(((p[..., 3] > 0) & (p[..., 1] > 0)).sum()) for p in plain[1:])
        assert fringe > 200, (kind, edge, fringe)            # what the plain chain does to this image
        for g, p in zip(got[1:], plain[1:]):
            seen = g[..., 3] > 0
            assert (g[seen][:, 0] == 255).all() and (g[seen][:, 1] == 0).all(), (kind, edge, g.shape)


def test_disc_box_texels_without_alpha_are_the_plain_filters():
    """One level at a time (both chains from the same source level): texels whose footprint has SA = 0 equal the plain ones."""
    lv, checked = _disc(), 0
    while lv.shape[1] > 1:
        nxt, plain = W.downsample(lv, W.VOLUME, W.BOX, W.CLAMP, W.ALPHA), F.chain(lv, W.VOLUME, W.BOX, W.CLAMP, 2)[1]
        a = lv[0, :, :, 3].astype(np.int64)
        sa = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
        assert (nxt[0][sa == 0] == plain[0][sa == 0]).all()
        checked += int((sa == 0).sum())
        lv = nxt
    assert checked > 1000


def test_kernels_use_no_scratch(tmp_path, A):
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF)):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    mine = {n: d for n, d in k.items() if "astc_mipw_" in n}
    # six box shapes and the two windowed ones, each for U8, U8 sRGB, F16 and F32
    assert len(mine) == 32, sorted(mine)
    for shape in ("astc_mipw_even", "astc_mipw_level", "astc_mipw_tail", "astc_mipw_even3d", "astc_mipw_level3d", "astc_mipw_tail3d",
                  "astc_mipw_filter_level", "astc_mipw_filter_tail"):
        assert sum(1 for n in mine if shape + "I" in n) == 4, (shape, sorted(mine))
    for n, d in mine.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
        assert d["group_segment_fixed_size"] <= 65536, (n, d)


def test_exported_and_declared(A):
    names = ["astcenc_amd_generate_mip_chain_weighted_device", "astcenc_amd_compress_mip_chain_weighted_device"]
    header = open(os.path.join(ROOT, "include", "astcenc_amd.h")).read()
    for n in names:
        assert n in A.EXPORTS_AMD and n + "(" in header
    assert (A.MIP_WEIGHT_NONE, A.MIP_WEIGHT_ALPHA) == (0, 1)
    assert "ASTCENC_AMD_MIP_WEIGHT_ALPHA = 1" in " ".join(header.split())
    if os.path.exists(A.LIB_PRODUCT):
        lib = C.CDLL(A.LIB_PRODUCT)
        for n in names:
            getattr(lib, n)


def test_null_context(product, A):
    swz = A.Swizzle(*A.SWZ_RGBA)
    flt = A.MipFilter(A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP)
    wt = A.MipWeighting(A.MIP_WEIGHT_ALPHA)
    assert product.lib.astcenc_amd_generate_mip_chain_weighted_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, 0, None, C.byref(flt),
                                                                      C.byref(wt), 0x2000, 1 << 20, None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_compress_mip_chain_weighted_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, C.byref(swz), 0, None,
                                                                      C.byref(flt), C.byref(wt), 0x2000, 1 << 20, 0x3000, 1 << 20, None,
                                                                      None) == A.ERR_BAD_PARAM
