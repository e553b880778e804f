# SPDX-License-Identifier: Apache-2.0
"""Resizing without a GPU (csrc/mip_resize.h, include/astcenc_amd.h):

  * the header compiled with g++ -ffp-contract=off against the model (tests/resize_model.py): the taps and weights of every
    filter at ratios up, down, equal and from one texel, the periods the kernels' table relies on, and whole small images for
    U8, U8 sRGB, F16 and F32, both weightings, every filter kind, both edges, as ARRAY and VOLUME;
  * the two equalities the feature rests on: at d = max(1, s >> 1) the windowed taps are mip_resample_taps' (and
    mip_filter_model.taps'), every float equal, for s = 1..399, 1000, 4097, 16385, 65535 and j in {0, 1, d/2, d-1}; and the box
    is the chain's box -- weights (1, 1) over 2, (n-j, n, j+1) over 2n+1 -- for every s = 1..599 and every j;
  * astcenc_amd_resize_dims against hand-computed cases, through the header and through the library;
  * the astc_resize_* kernels of the shipped library use no scratch memory, spill nothing and stay within 64 KiB of LDS;
  * both entry points are exported, declared, and refuse a null context or null outputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_filter_model as F  # noqa: E402
import mip_model as M  # noqa: E402
import resize_model as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

RESIZE_MAIN = r"""
#include "mip_resize.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace astcd;

static double csin(double x) { return sin(x); }

struct Job {
	unsigned int kind, edge, type, srgb, array, weight, w, h, z, dw, dh, dz;
	std::vector<unsigned char> src, dst;
	double tables[MIP_SRGB_TABLE_DOUBLES];
};

static void axis_taps(const Job& J, unsigned int s, unsigned int d, unsigned int j, bool one, MipResampleTaps& t, std::vector<double>& w,
                      unsigned int& den)
{
	t.s = s; t.edge = J.edge;
	if (one) { w.assign(1, 1.0); t.first = j; t.count = 1; den = 1; t.w = w.data(); return; }
	const unsigned long long n = mip_resize_tap_count((int)J.kind, s, d, j, &t.first, &den);
	w.resize(n);
	mip_resize_tap_weights((int)J.kind, s, d, j, csin, t.first, n, w.data());
	t.count = (unsigned int)n; t.w = w.data();
}

template <int TYPE, bool BOX, bool WEIGHTED>
static void run(Job& J)
{
	constexpr int N = WEIGHTED ? 7 : 4;
	constexpr unsigned int INTS = mip_resize_ints(TYPE, BOX, WEIGHTED);
	const size_t tb = J.type == 0 ? 4 : J.type == 1 ? 8 : 16;
	const double* lin = TYPE == MIP_RESIZE_U8_SRGB ? J.tables : nullptr;
	const double* thr = TYPE == MIP_RESIZE_U8_SRGB ? J.tables + 256 : nullptr;
	std::vector<double> wx, wy, wz;
	for (unsigned int oz = 0; oz < J.dz; oz++)
		for (unsigned int oy = 0; oy < J.dh; oy++)
			for (unsigned int ox = 0; ox < J.dw; ox++)
			{
				MipResampleTaps tx, ty, tz;
				unsigned int dx, dy, dz;
				axis_taps(J, J.w, J.dw, ox, false, tx, wx, dx);
				axis_taps(J, J.h, J.dh, oy, false, ty, wy, dy);
				axis_taps(J, J.z, J.dz, oz, J.array != 0, tz, wz, dz);
				MipResizeSlot vol[N];
				mip_resize_texel<N, INTS>(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz, MipResizeSlot v[N]) {
					const size_t i = (((size_t)sz * J.h + sy) * J.w + sx) * tb;
					if (TYPE != MIP_RESIZE_FLOAT)
					{
						unsigned int p;
						memcpy(&p, &J.src[i], 4);
						mip_resize_load_u8<N, INTS>(p, lin, v);
						return;
					}
					float f[4];
					for (int c = 0; c < 4; c++)
					{
						if (J.type == 1) { unsigned short hv; memcpy(&hv, &J.src[i + 2 * c], 2); f[c] = mip_float_from_half(hv); }
						else memcpy(&f[c], &J.src[i + 4 * c], 4);
					}
					mip_resize_load_float<N>(f, v);
				}, vol);
				const unsigned long long den = (unsigned long long)dx * dy * dz;
				const double dden = ((double)dx * (double)dy) * (double)dz;
				const size_t o = (((size_t)oz * J.dh + oy) * J.dw + ox) * tb;
				if (TYPE != MIP_RESIZE_FLOAT)
				{
					const unsigned int p = mip_resize_out_u8<N, BOX>(vol, thr, den, dden);
					memcpy(&J.dst[o], &p, 4);
					continue;
				}
				float f[4];
				mip_resize_out_float<N, BOX>(vol, dden, f);
				for (int c = 0; c < 4; c++)
				{
					if (J.type == 1) { const unsigned short hv = mip_half_from_float(f[c]); memcpy(&J.dst[o + 2 * c], &hv, 2); }
					else memcpy(&J.dst[o + 4 * c], &f[c], 4);
				}
			}
}

template <int TYPE>
static void run_type(Job& J)
{
	const bool box = J.kind == 0;
	if (J.weight) { if (box) run<TYPE, true, true>(J); else run<TYPE, false, true>(J); }
	else { if (box) run<TYPE, true, false>(J); else run<TYPE, false, false>(J); }
}

// "taps":  lines "kind s d j" -> "first count den period shift w0 w1 ..." (weights as %a)
// "chain": lines "kind s j" -> the chain's taps of mip_axis_taps (kind 0) / mip_resample_taps, same format without the period
// "dims":  lines "x y max pow2" -> "ok out_x out_y"
// "image": "kind edge type srgb array weight w h z dw dh dz\n" + the image, any number of times -> the resized images
int main(int argc, char** argv)
{
	const char* mode = argc > 1 ? argv[1] : "";
	if (!strcmp(mode, "taps"))
	{
		unsigned int kind, s, d, j;
		while (scanf("%u %u %u %u", &kind, &s, &d, &j) == 4)
		{
			long long first;
			unsigned int den, period, shift;
			const unsigned long long n = mip_resize_tap_count((int)kind, s, d, j, &first, &den);
			std::vector<double> w(n);
			mip_resize_tap_weights((int)kind, s, d, j, csin, first, n, w.data());
			mip_resize_period((int)kind, s, d, &period, &shift);
			printf("%lld %llu %u %u %u", first, n, den, period, shift);
			for (double v : w) printf(" %a", v);
			printf("\n");
		}
		return 0;
	}
	if (!strcmp(mode, "chain"))
	{
		unsigned int kind, s, j;
		while (scanf("%u %u %u", &kind, &s, &j) == 3)
		{
			if (kind == 0)
			{
				const MipTaps t = mip_axis_taps(s, j);
				printf("%u %u %u", t.first, t.count, t.den);
				for (unsigned int k = 0; k < t.count; k++) printf(" %a", (double)t.w[k]);
			}
			else
			{
				long long first;
				double w[MIP_RESAMPLE_MAX_TAPS];
				const unsigned int n = mip_resample_taps((int)kind, s, j, csin, &first, w);
				printf("%lld %u 1", first, n);
				for (unsigned int k = 0; k < n; k++) printf(" %a", w[k]);
			}
			printf("\n");
		}
		return 0;
	}
	if (!strcmp(mode, "dims"))
	{
		unsigned int x, y, m, p;
		while (scanf("%u %u %u %u", &x, &y, &m, &p) == 4)
		{
			unsigned int ox = 0, oy = 0;
			const bool ok = mip_resize_dims(x, y, m, p, &ox, &oy);
			printf("%d %u %u\n", ok ? 1 : 0, ox, oy);
		}
		return 0;
	}
	Job J;
	mip_srgb_tables_build(J.tables, [](double x, double y) { return std::pow(x, y); });
	while (scanf("%u %u %u %u %u %u %u %u %u %u %u %u", &J.kind, &J.edge, &J.type, &J.srgb, &J.array, &J.weight, &J.w, &J.h, &J.z, &J.dw,
	             &J.dh, &J.dz) == 12)
	{
		getchar();
		const size_t tb = J.type == 0 ? 4 : J.type == 1 ? 8 : 16;
		J.src.resize((size_t)J.w * J.h * J.z * tb);
		if (fread(J.src.data(), 1, J.src.size(), stdin) != J.src.size()) return 3;
		J.dst.assign((size_t)J.dw * J.dh * J.dz * tb, 0);
		if (J.type != 0) run_type<MIP_RESIZE_FLOAT>(J);
		else if (J.srgb) run_type<MIP_RESIZE_U8_SRGB>(J);
		else run_type<MIP_RESIZE_U8>(J);
		fwrite(J.dst.data(), 1, J.dst.size(), stdout);
	}
	return 0;
}
"""


@pytest.fixture(scope="module")
def resize_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("resize")
    src, exe = d / "resize.cpp", d / "resize"
    src.write_text(RESIZE_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _lines(exe, mode, rows):
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in rows)
    r = subprocess.run([exe, mode], input=text.encode(), capture_output=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out = [ln.split() for ln in r.stdout.decode().splitlines()]
    assert len(out) == len(rows)
    return out


def _parse(fields, head):
    return [int(v) for v in fields[:head]], [float.fromhex(v) for v in fields[head:]]


RATIOS = [(97, 40), (61, 77), (1000, 7), (3, 200), (5, 5), (1, 9), (9, 1), (64, 32), (33, 16), (12, 48), (7, 21), (2, 3), (400, 100),
          (255, 256), (256, 255), (30, 20)]


def test_taps_equal_the_model(resize_exe):
    rows = [(kind, s, d, j) for kind in R.FILTERS for s, d in RATIOS for j in sorted({0, 1 % d, d // 2, d - 1})]
    for (kind, s, d, j), fields in zip(rows, _lines(resize_exe, "taps", rows)):
        (first, count, den, _, _), w = _parse(fields, 5)
        m_first, m_w, m_den = R.taps(kind, s, d, j)
        assert (first, count, den) == (m_first, len(m_w), m_den), (kind, s, d, j)
        assert w == m_w, (kind, s, d, j, w, m_w)
        # the weights of a windowed kind sum to about one, the box's to its denominator exactly
        assert abs(sum(w) - (den if kind == R.BOX else 1.0)) < 1e-12


def test_periods_are_exact(resize_exe):
    """Where mip_resize_period reports a period, destination j has the taps of j mod period moved by (j / period) * shift."""
    cases = [(kind, s, d) for kind in R.FILTERS for s, d in RATIOS + [(96, 8), (8, 64), (8, 24), (90, 60)]]
    head = _lines(resize_exe, "taps", [(k, s, d, 0) for k, s, d in cases])
    seen = 0
    for (kind, s, d), fields in zip(cases, head):
        period, shift = int(fields[3]), int(fields[4])
        assert 1 <= period <= d
        if period == d:
            continue
        seen += 1
        for j in range(d):
            first, w, _ = R.taps(kind, s, d, j)
            bfirst, bw, _ = R.taps(kind, s, d, j % period)
            assert (first, w) == (bfirst + (j // period) * shift, bw), (kind, s, d, j, period, shift)
    assert seen >= 30
    # an integer ratio has one row; a windowed enlargement by three has none (its centres are not exact)
    assert [int(v) for v in _lines(resize_exe, "taps", [(R.LANCZOS3, 96, 8, 0)])[0][3:5]] == [1, 12]
    assert [int(v) for v in _lines(resize_exe, "taps", [(R.LANCZOS3, 8, 24, 0)])[0][3:5]] == [24, 0]
    assert [int(v) for v in _lines(resize_exe, "taps", [(R.BOX, 8, 24, 0)])[0][3:5]] == [3, 1]


def _halving_js(d):
    return sorted({0, 1 % d, d // 2, d - 1})


def test_halving_gives_the_chains_windowed_taps(resize_exe):
    sizes = list(range(1, 400)) + [1000, 4097, 16385, 65535]
    rows = [(kind, s, max(1, s >> 1), j) for kind in F.KINDS for s in sizes for j in _halving_js(max(1, s >> 1))]
    new = _lines(resize_exe, "taps", rows)
    old = _lines(resize_exe, "chain", [(kind, s, j) for kind, s, _, j in rows])
    for (kind, s, d, j), a, b in zip(rows, new, old):
        (first, count, _, _, _), w = _parse(a, 5)
        (ofirst, ocount, _), ow = _parse(b, 3)
        assert (first, count, w) == (ofirst, ocount, ow), (kind, s, j)
        m_first, m_w = F.taps(kind, s, j)
        assert (first, w) == (m_first, m_w), (kind, s, j)
        assert R.taps(kind, s, d, j)[:2] == (m_first, m_w), (kind, s, j)


def test_halving_gives_the_chains_box(resize_exe):
    rows = [(R.BOX, s, max(1, s >> 1), j) for s in range(1, 600) for j in range(max(1, s >> 1))]
    new = _lines(resize_exe, "taps", rows)
    old = _lines(resize_exe, "chain", [(0, s, j) for _, s, _, j in rows])
    for (_, s, d, j), a, b in zip(rows, new, old):
        (first, count, den, _, _), w = _parse(a, 5)
        (ofirst, ocount, oden), ow = _parse(b, 3)
        assert (first, count, den, w) == (ofirst, ocount, oden, ow), (s, j)
        n = s >> 1
        want = (0, [1.0], 1) if s == 1 else (2 * j, [1.0, 1.0], 2) if s % 2 == 0 else (2 * j, [float(n - j), float(n), float(j + 1)], s)
        assert (first, w, den) == want == R.taps(R.BOX, s, d, j), (s, j)
    # ... and the model's arrays are mip_model.axis_taps'
    for s in (1, 2, 7, 64, 97):
        idx, w, valid, den = R.axis(R.BOX, R.CLAMP, s, max(1, s >> 1))
        mi, mw, mden = M.axis_taps(s)
        assert den == mden and valid.all() and [r.tolist() for r in idx] == [r.tolist() for r in mi]
        assert [r.tolist() for r in w] == [r.astype(np.float64).tolist() for r in mw]


def _same(g, m):
    if g.shape != m.shape:
        return False
    if g.dtype == np.uint8:
        return g.tobytes() == m.tobytes()
    bits = np.uint16 if g.dtype == np.float16 else np.uint32
    return bool(((g.view(bits) == m.view(bits)) | (np.isnan(g) & np.isnan(m))).all())


def _input(dtype, shape, rng, special):
    if dtype == np.uint8:
        v = rng.integers(0, 256, shape + (4,), dtype=np.uint8)
        v[..., 3][rng.random(shape) < 0.4] = 0
        return v
    v = (rng.random(shape + (4,)) * 1.4 - 0.2).astype(dtype)
    v[..., 3][rng.random(shape) < 0.3] = 0
    if special:
        flat = v.reshape(-1)
        pos = rng.choice(flat.size, size=max(1, flat.size // 30), replace=False)
        flat[pos] = np.where(rng.random(pos.size) < 0.5, np.inf, -np.inf).astype(dtype)
    return v


def _resized(exe, jobs):
    """jobs: [(kind, edge, img, mip_kind, srgb, weight, size)] -> the resized image of each from one run of the header's program."""
    data, shapes = [], []
    for kind, edge, img, mip_kind, srgb, weight, size in jobs:
        z, h, w = img.shape[:3]
        ow, oh, od = (tuple(size) + (z,))[:3]
        t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[img.dtype]
        data.append(b"%d %d %d %d %d %d %d %d %d %d %d %d\n" % (kind, edge, t, int(srgb), int(mip_kind == R.ARRAY), weight, w, h, z, ow, oh, od))
        data.append(np.ascontiguousarray(img).tobytes())
        shapes.append((img.dtype, (od, oh, ow, 4)))
    r = subprocess.run([exe, "image"], input=b"".join(data), capture_output=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr)
    out, at = [], 0
    for dtype, shape in shapes:
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        out.append(np.frombuffer(r.stdout[at:at + n], dtype=dtype).reshape(shape))
        at += n
    assert at == len(r.stdout)
    return out


# (mip kind, source [Z, H, W], destination (w, h[, d])): down, up, mixed, an untouched axis, s == 1, the same size, all three axes
IMAGES = [(R.VOLUME, (1, 13, 17), (7, 20)), (R.VOLUME, (1, 9, 40), (3, 9)), (R.ARRAY, (3, 6, 5), (11, 4)), (R.VOLUME, (5, 7, 9), (4, 12, 3)),
          (R.VOLUME, (1, 1, 6), (9, 5)), (R.VOLUME, (4, 1, 1), (3, 2, 9)), (R.ARRAY, (2, 8, 8), (8, 8)), (R.VOLUME, (6, 10, 4), (2, 5, 3)),
          (R.VOLUME, (1, 3, 50), (2, 31)), (R.VOLUME, (7, 5, 3), (3, 5, 2))]
CPU_FILTERS = [(R.BOX, R.CLAMP)] + [(k, e) for k in F.KINDS for e in (R.CLAMP, R.WRAP)]
TYPES = [("u8", np.uint8, False), ("srgb", np.uint8, True), ("f16", np.float16, False), ("f32", np.float32, False)]


@pytest.mark.parametrize("name,dtype,srgb", TYPES, ids=[t[0] for t in TYPES])
@pytest.mark.parametrize("weight", [R.NONE, R.ALPHA], ids=["plain", "alpha"])
@pytest.mark.parametrize("kind,edge", CPU_FILTERS, ids=["f%d-e%d" % f for f in CPU_FILTERS])
def test_images_equal_the_model(resize_exe, kind, edge, weight, name, dtype, srgb):
    rng = np.random.default_rng(1000 * kind + 100 * edge + 10 * weight + np.dtype(dtype).itemsize + int(srgb))
    jobs = [(kind, edge, _input(dtype, shape, rng, n % 2 == 1), mip_kind, srgb, weight, size) for n, (mip_kind, shape, size) in enumerate(IMAGES)]
    for (_, _, img, mip_kind, _, _, size), g in zip(jobs, _resized(resize_exe, jobs)):
        want = R.resize(img, size, mip_kind, kind, edge, weight, srgb)
        assert _same(g, want), (kind, edge, weight, mip_kind, img.shape, size, dtype, srgb, g.tolist(), want.tolist())


def test_model_properties():
    """The same size returns the input; channel 3 of a weighted resize is the plain one's; halving is the chain's level 1."""
    import mip_weighted_model as W
    rng = np.random.default_rng(3)
    for dtype in (np.uint8, np.float16, np.float32):
        for mip_kind, shape in [(R.VOLUME, (1, 13, 18)), (R.ARRAY, (3, 6, 5)), (R.VOLUME, (5, 7, 9))]:
            img = _input(dtype, shape, rng, False)
            z, h, w = shape
            half = (max(1, w >> 1), max(1, h >> 1), max(1, z >> 1) if mip_kind == R.VOLUME else z)
            for kind, edge in CPU_FILTERS:
                for srgb in ((False, True) if dtype == np.uint8 else (False,)):
                    assert R.resize(img, (w, h, z), mip_kind, kind, edge, R.NONE, srgb).tobytes() == img.tobytes()
                    plain = R.resize(img, (w + 3, max(1, h - 2)), mip_kind, kind, edge, R.NONE, srgb)
                    alpha = R.resize(img, (w + 3, max(1, h - 2)), mip_kind, kind, edge, R.ALPHA, srgb)
                    assert plain[..., 3].tobytes() == alpha[..., 3].tobytes()
                    for weight in (R.NONE, R.ALPHA):
                        want = W.downsample(img, mip_kind, kind, edge, weight, srgb)
                        assert _same(R.resize(img, half, mip_kind, kind, edge, weight, srgb), want), (dtype, shape, kind, edge, srgb, weight)


# (x, y, max_dim, pow2) -> (out_x, out_y) or None, worked out by hand
DIMS = [((8192, 8192, 4096, R.POW2_NONE), (4096, 4096)),
        ((8192, 4096, 2048, R.POW2_NONE), (2048, 1024)),
        ((1000, 300, 0, R.POW2_NONE), (1000, 300)),
        ((1000, 300, 2000, R.POW2_NONE), (1000, 300)),
        ((1000, 3, 100, R.POW2_NONE), (100, 1)),              # (3 * 100 + 500) / 1000 = 0 -> 1
        ((1000, 15, 100, R.POW2_NONE), (100, 2)),             # (1500 + 500) / 1000 = 2: a half rounds up
        ((300, 1000, 100, R.POW2_NONE), (30, 100)),
        ((100, 100, 0, R.POW2_NEXT), (128, 128)),
        ((100, 100, 0, R.POW2_PREVIOUS), (64, 64)),
        ((64, 1, 0, R.POW2_NEXT), (64, 1)),
        ((96, 95, 0, R.POW2_NEAREST), (128, 64)),             # 96 ties between 64 and 128: up; 95 is nearer 64
        ((3, 6, 0, R.POW2_NEAREST), (4, 8)),                  # both ties
        ((97, 48, 0, R.POW2_NEAREST), (128, 64)),
        ((1500, 700, 1024, R.POW2_NEXT), (1024, 512)),        # 1024 x 478: 478 -> 512
        ((1500, 700, 1000, R.POW2_NEXT), (512, 512)),         # 1000 x 467: 1024 exceeds the cap -> PREVIOUS 512; 467 -> 512
        ((1500, 700, 1000, R.POW2_NEAREST), (512, 512)),      # 1000 -> 1024 exceeds the cap -> 512; 467 -> 512
        ((5000, 5000, 3000, R.POW2_NEAREST), (2048, 2048)),   # 3000 -> 2048 (952 < 1096)
        ((700, 700, 1000, R.POW2_NEXT), (512, 512)),          # no cap applied, but 1024 exceeds the cap that was given
        ((4294967295, 1, 0, R.POW2_NONE), None),              # above 2^31
        ((4294967295, 1, 0, R.POW2_PREVIOUS), (2147483648, 1)),
        ((4294967295, 1, 0, R.POW2_NEXT), None),
        ((2147483648, 2147483648, 0, R.POW2_NEAREST), (2147483648, 2147483648)),
        ((0, 5, 0, R.POW2_NONE), None), ((5, 0, 0, R.POW2_NONE), None), ((5, 5, 0, 4), None)]


def test_resize_dims(resize_exe, A):
    got = _lines(resize_exe, "dims", [args for args, _ in DIMS])
    for (args, want), g in zip(DIMS, got):
        assert R.resize_dims(*args) == want, args
        ok, x, y = (int(v) for v in g)
        assert (bool(ok), (x, y) if ok else None) == (want is not None, want), (args, g)
    if not os.path.exists(A.LIB_PRODUCT):
        pytest.skip("needs the built product library")
    lib = A.Library(A.LIB_PRODUCT)
    for args, want in DIMS:
        err, out = lib.resize_dims(*args)
        assert (err, out) == ((A.SUCCESS, want) if want else (A.ERR_BAD_PARAM, (0, 0))), args
    x = C.c_uint(7)
    assert lib.lib.astcenc_amd_resize_dims(8, 8, 0, 0, None, C.byref(x)) == A.ERR_BAD_PARAM
    assert lib.lib.astcenc_amd_resize_dims(8, 8, 0, 0, C.byref(x), None) == A.ERR_BAD_PARAM
    assert lib.lib.astcenc_amd_resize_dims(8, 8, 0, -1, C.byref(x), C.byref(x)) == A.ERR_BAD_PARAM and x.value == 7


def test_kernels_use_no_scratch(tmp_path, A):
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF)):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    mine = {n: d for n, d in k.items() if "astc_resize_" in n}
    # U8, U8 sRGB, F16 and F32, each plain and weighted, box and windowed
    assert len(mine) == 16, sorted(mine)
    for n, d in mine.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
        assert d["group_segment_fixed_size"] <= 65536, (n, d)


def test_exported_and_declared(A):
    names = ["astcenc_amd_resize_image_device", "astcenc_amd_resize_dims"]
    header = open(os.path.join(ROOT, "include", "astcenc_amd.h")).read()
    for n in names:
        assert n in A.EXPORTS_AMD and n + "(" in header
    flat = " ".join(header.split())
    assert "ASTCENC_AMD_POW2_NONE = 0" in flat and "ASTCENC_AMD_POW2_PREVIOUS = 3" in flat
    assert (A.POW2_NONE, A.POW2_NEAREST, A.POW2_NEXT, A.POW2_PREVIOUS) == (0, 1, 2, 3)
    if os.path.exists(A.LIB_PRODUCT):
        lib = C.CDLL(A.LIB_PRODUCT)
        for n in names:
            getattr(lib, n)


def test_null_context(product, A):
    rz = A.Resize(32, 32, 1, A.MipFilter(A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP), A.MipWeighting(A.MIP_WEIGHT_NONE))
    assert product.lib.astcenc_amd_resize_image_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, C.byref(rz), 0x2000, 1 << 20, None,
                                                       None) == A.ERR_BAD_PARAM
