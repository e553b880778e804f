# SPDX-License-Identifier: Apache-2.0
"""Seamless cube-map edges of the windowed mip filters without a GPU (ASTCENC_AMD_MIP_EDGE_CUBE; csrc/mip_resample.h,
csrc/mip_weighted.h compiled with g++ -ffp-contract=off against tests/mip_cube_model.py):

  * mip_cube_source against the model's integer rule: s = 1 .. 9 and 64, every face, every ix, iy in -10 .. s + 9;
  * its geometry, independent of that rule, with a floating-point GL direction -> (face, u, v) lookup written from the face table
    alone: a one-axis overshoot maps to the mirror image of the face's own texel at that depth through the plane of the shared
    edge and the cube's centre; at overshoot 0 the border texel and its mapped neighbour both lie 1 doubled unit from the shared
    cube edge, at the same position along it;
  * the header's per-texel routines against the model on one level of random cubes: faces 1, 2, 3, 5, 8, 9, 33 and a two-cube
    array; the three filters; U8, U8 sRGB, F16 and F32 with infinities; plain and alpha-weighted; bit for bit;
  * a constant cube stays constant on every level; the constants of the Python binding, the public header and csrc agree;
  * the astc_mipcube_* / astc_mipcubew_* kernels of the shipped library use no scratch memory and spill nothing."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_filter_model as F  # noqa: E402
import mip_cube_model as CM  # noqa: E402
from test_mip_filter_cpu import _random, _same  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

CUBE_MAIN = r"""
#include "mip_weighted.h"
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
	if (!strcmp(mode, "const")) { printf("%d\n", (int)MIP_EDGE_CUBE); return 0; }
	if (!strcmp(mode, "source") && argc == 3)      // argv: s; stdin: n, n x (int64 face, ix, iy); stdout: n x (uint32 face, x, y)
	{
		const unsigned int s = (unsigned int)strtoul(argv[2], nullptr, 10);
		unsigned int n;
		if (fread(&n, 4, 1, stdin) != 1) return 3;
		std::vector<long long> in(3 * (size_t)n);
		if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 3;
		for (unsigned int i = 0; i < n; i++)
		{
			const MipCubeTexel t = mip_cube_source((unsigned int)in[3 * i], in[3 * i + 1], in[3 * i + 2], s);
			const unsigned int out[3] = { t.face, t.x, t.y };
			put(out, 12);
		}
		return 0;
	}
	if (!strcmp(mode, "level"))                    // stdin: "kind type srgb weighted s z\n", the level; stdout: the next level
	{
		unsigned int kind, type, srgb, weighted, s, z;
		if (scanf("%u %u %u %u %u %u", &kind, &type, &srgb, &weighted, &s, &z) != 6) return 2;
		getchar();
		const size_t tb = type == 0 ? 4 : type == 1 ? 8 : 16;
		std::vector<unsigned char> src((size_t)s * s * z * tb);
		if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
		double tables[MIP_SRGB_TABLE_DOUBLES];
		mip_srgb_tables_build(tables, [](double x, double y) { return std::pow(x, y); });
		const unsigned int d = mip_level_dim(s, 1);
		std::vector<unsigned char> dst((size_t)d * d * z * tb);
		double wx[MIP_RESAMPLE_MAX_TAPS], wy[MIP_RESAMPLE_MAX_TAPS];
		for (unsigned int layer = 0; layer < z; layer++)
			for (unsigned int oy = 0; oy < d; oy++)
				for (unsigned int ox = 0; ox < d; ox++)
				{
					MipResampleTaps tx, ty;
					tx.s = s; tx.edge = MIP_EDGE_CUBE; tx.w = wx; tx.count = mip_resample_taps((int)kind, s, ox, csin, &tx.first, wx);
					ty.s = s; ty.edge = MIP_EDGE_CUBE; ty.w = wy; ty.count = mip_resample_taps((int)kind, s, oy, csin, &ty.first, wy);
					const unsigned int face = layer % 6, cube0 = layer - face;
					// the stored texel (face, x, y) of this cube as four floats or a packed RGBA8
					auto texel = [&](unsigned int f, unsigned int x, unsigned int y, unsigned int& p, float fl[4]) {
						const size_t i = (((size_t)(cube0 + f) * s + y) * s + x) * tb;
						if (type == 0) { memcpy(&p, &src[i], 4); return; }
						for (int c = 0; c < 4; c++)
						{
							if (type == 1) { unsigned short hv; memcpy(&hv, &src[i + 2 * c], 2); fl[c] = mip_float_from_half(hv); }
							else memcpy(&fl[c], &src[i + 4 * c], 4);
						}
					};
					double vol[7];
					if (weighted)
						mip_resample_texel_cube_weighted(face, tx, ty, [&](unsigned int f, unsigned int x, unsigned int y, double v[7]) {
							unsigned int p = 0; float fl[4];
							texel(f, x, y, p, fl);
							if (type == 0) mip_resample_load_u8_weighted(p, srgb ? tables : nullptr, v);
							else mip_resample_load_float_weighted(fl, v);
						}, vol);
					else
						mip_resample_texel_cube(face, tx, ty, [&](unsigned int f, unsigned int x, unsigned int y, double v[4]) {
							unsigned int p = 0; float fl[4];
							texel(f, x, y, p, fl);
							if (type == 0) mip_resample_load_u8(p, srgb ? tables : nullptr, v);
							else mip_resample_load_float(fl, v);
						}, vol);
					const size_t o = (((size_t)layer * d + oy) * d + ox) * tb;
					if (type == 0)
					{
						const double* thr = srgb ? tables + 256 : nullptr;
						const unsigned int p = weighted ? mip_resample_out_u8_weighted(vol, thr) : mip_resample_out_u8(vol, thr);
						memcpy(&dst[o], &p, 4);
					}
					else
					{
						float fl[4];
						if (weighted) mip_resample_out_float_weighted(vol, fl);
						else mip_resample_out_float(vol, fl);
						for (int c = 0; c < 4; c++)
						{
							if (type == 1) { const unsigned short hv = mip_half_from_float(fl[c]); memcpy(&dst[o + 2 * c], &hv, 2); }
							else memcpy(&dst[o + 4 * c], &fl[c], 4);
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
def cube_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mipcube")
    src, exe = d / "cube.cpp", d / "cube"
    src.write_text(CUBE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _run(exe, args, data=b""):
    r = subprocess.run([exe] + [str(a) for a in args], input=data, capture_output=True, timeout=600)
    assert r.returncode == 0, (args, r.returncode, r.stderr)
    return r.stdout


def _header_source(exe, s, taps):
    """[(face, x, y)] of the header's mip_cube_source for taps [(face, ix, iy)]."""
    q = np.asarray(taps, np.int64).reshape(-1, 3)
    raw = _run(exe, ["source", s], np.array([len(q)], np.uint32).tobytes() + q.tobytes())
    return [tuple(int(v) for v in row) for row in np.frombuffer(raw, np.uint32).reshape(-1, 3)]


SIZES = list(range(1, 10)) + [64]


def test_source_equals_the_model(cube_exe):
    for s in SIZES:
        taps = [(f, ix, iy) for f in range(6) for iy in range(-10, s + 10) for ix in range(-10, s + 10)]
        got = _header_source(cube_exe, s, taps)
        for t, g in zip(taps, got):
            assert g == CM.source(t[0], t[1], t[2], s), (s, t, g)
            assert 0 <= g[1] < s and 0 <= g[2] < s
            inside = (0 <= t[1] < s) + (0 <= t[2] < s)
            assert (g[0] != t[0]) == (inside == 1), (s, t, g)


def test_neighbours(cube_exe):
    """The faces across x < 0, x >= s, y < 0, y >= s, as include/astcenc_amd.h lists them."""
    want = {"+X": "+Z -Z +Y -Y", "-X": "-Z +Z +Y -Y", "+Y": "-X +X -Z +Z", "-Y": "-X +X +Z -Z", "+Z": "-X +X +Y -Y", "-Z": "+X -X +Y -Y"}
    s = 5
    for f, name in enumerate(CM.FACES):
        got = _header_source(cube_exe, s, [(f, -1, 2), (f, s, 2), (f, 2, -1), (f, 2, s)])
        assert " ".join(CM.FACES[g[0]] for g in got) == want[name], name


def _gl_lookup(d):
    """The GL cube-map lookup of direction d, from the face table alone: (face, u, v) with u, v in [0, 1]."""
    ax = int(np.argmax(np.abs(d)))
    f = 2 * ax + (0 if d[ax] > 0 else 1)
    ma = abs(float(d[ax]))
    sc, tc = float(np.dot(d, CM.SDIR[f])), float(np.dot(d, CM.TDIR[f]))
    return f, (sc / ma + 1.0) / 2.0, (tc / ma + 1.0) / 2.0


def test_geometry(cube_exe):
    for s in (2, 3, 4, 5, 8, 9):
        for f in range(6):
            m = np.array(CM.MAJOR[f])
            for axis_dir, along_x in ((np.array(CM.SDIR[f]), True), (np.array(CM.TDIR[f]), False)):
                for sg in (1, -1):
                    n = sg * axis_dir                              # the neighbour's major axis
                    taps, own = [], []
                    for k in range(0, s + 3):
                        for p in range(s):
                            out = s + k if sg > 0 else -1 - k
                            depth = min(k, s - 1)
                            inner = s - 1 - depth if sg > 0 else depth
                            taps.append((f, out, p) if along_x else (f, p, out))
                            own.append((inner, p) if along_x else (p, inner))
                    got = _header_source(cube_exe, s, taps)
                    for (k, (ox, oy)), g in zip(((i // s, o) for i, o in enumerate(own)), got):
                        c_own = np.array(CM.centre(f, ox, oy, s), np.float64)
                        # the mirror image through the plane that holds the shared edge and the centre: normal m - n, |m - n|^2 = 2
                        normal = (m - n).astype(np.float64)
                        mirror = c_own - np.dot(c_own, normal) * normal
                        gf, u, v = _gl_lookup(mirror)
                        assert g[0] == gf and CM.MAJOR[gf] == tuple(n), (s, f, k, g, gf)
                        assert abs(u * s - (g[1] + 0.5)) < 1e-9 and abs(v * s - (g[2] + 0.5)) < 1e-9, (s, f, k, g, u, v)
                        c_map = np.array(CM.centre(g[0], g[1], g[2], s), np.float64)
                        assert (c_map == mirror).all()
                        if k == 0:
                            # the shared cube edge is the line s m + s n + t e: distances from it, and the position along it
                            e = np.cross(m, n)
                            d_own = np.hypot(np.dot(c_own, m) - s, np.dot(c_own, n) - s)
                            d_map = np.hypot(np.dot(c_map, m) - s, np.dot(c_map, n) - s)
                            assert d_own == 1.0 and d_map == 1.0, (s, f, g, d_own, d_map)
                            assert np.dot(c_own, e) == np.dot(c_map, e)


def _level(exe, kind, img, weight, srgb=False):
    z, s = img.shape[:2]
    t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[img.dtype]
    head = b"%d %d %d %d %d %d\n" % (kind, t, int(srgb), int(weight), s, z)
    raw = _run(exe, ["level"], head + np.ascontiguousarray(img).tobytes())
    d = max(1, s >> 1)
    return np.frombuffer(raw, dtype=img.dtype).reshape(z, d, d, 4)


SHAPES = [(6, 1), (6, 2), (6, 3), (6, 5), (6, 8), (6, 9), (6, 33), (12, 5)]


@pytest.mark.parametrize("weight", [CM.NONE, CM.ALPHA])
@pytest.mark.parametrize("dtype,srgb", [(np.uint8, False), (np.uint8, True), (np.float16, False), (np.float32, False)])
def test_texels_equal_the_model(cube_exe, dtype, srgb, weight):
    rng = np.random.default_rng(11 + int(srgb) + np.dtype(dtype).itemsize + 100 * weight)
    for kind in F.KINDS:
        for z, s in SHAPES:
            img = _random(dtype, (z, s, s), rng, inf=dtype != np.uint8 and s > 8)
            got = _level(cube_exe, kind, img, weight, srgb)
            want = CM.downsample(img, kind, weight, srgb)
            assert _same(got, want), (kind, z, s, dtype, srgb, weight)
            if weight == CM.ALPHA:                         # channel 3 is the plain CUBE filter's
                assert _same(got[..., 3], CM.downsample(img, kind, CM.NONE, srgb)[..., 3])


def test_two_cubes_do_not_read_each_other(cube_exe):
    rng = np.random.default_rng(5)
    a, b = _random(np.uint8, (6, 9, 9), rng), _random(np.uint8, (6, 9, 9), rng)
    both = _level(cube_exe, F.LANCZOS3, np.concatenate([a, b]), CM.NONE)
    assert both[:6].tobytes() == _level(cube_exe, F.LANCZOS3, a, CM.NONE).tobytes()
    assert both[6:].tobytes() == _level(cube_exe, F.LANCZOS3, b, CM.NONE).tobytes()


def test_constant_cube_stays_constant(cube_exe):
    for kind in F.KINDS:
        for z, s in [(6, 37), (12, 12)]:
            img = np.empty((z, s, s, 4), np.uint8)
            img[...] = (7, 128, 250, 0)
            model = CM.chain(img, kind)
            assert len(model) == s.bit_length()
            lv = img
            for want in model[1:]:
                lv = _level(cube_exe, kind, lv, CM.NONE)
                assert lv.shape == want.shape and (lv == img[0, 0, 0]).all() and (want == img[0, 0, 0]).all(), (kind, z, s)


def test_constants_agree(cube_exe, A):
    assert int(_run(cube_exe, ["const"])) == A.MIP_EDGE_CUBE == CM.CUBE == 2
    header = open(os.path.join(ROOT, "include", "astcenc_amd.h")).read()
    assert re.search(r"ASTCENC_AMD_MIP_EDGE_CUBE\s*=\s*2\b", header)


def test_cube_kernels_use_no_scratch(tmp_path, A):
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF)):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    for stem in ("astc_mipcube_", "astc_mipcubew_"):
        mine = {n: d for n, d in k.items() if stem in n}
        # one launch per level, no tail kernel: U8, U8 sRGB, F16 and F32
        assert len(mine) == 4, (stem, sorted(mine))
        for n, d in mine.items():
            assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
            assert d["group_segment_fixed_size"] <= 65536, (n, d)
