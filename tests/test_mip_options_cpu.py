# SPDX-License-Identifier: Apache-2.0
"""Mip chain options without a GPU (csrc/mip_post.h, include/astcenc_amd.h):

  * the per-texel arithmetic of the header compiled with g++, bit for bit against the numpy model (tests/mip_options_model.py):
    NORMALIZE on every one of the 2^24 RGB8 triples and on random and edge F16 / F32 texels (zero, inf, NaN, subnormal);
    the U8 coverage remap for every (a, a_k, t); the float remap on values next to the cutoff; the host-derived constants
    (t, hi, lo), the exact target count and the order-preserving keys;
  * a null context on both new entry points;
  * the astc_mippost_* kernels of the shipped library use no scratch memory and spill nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_options_model as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

POST_MAIN = r"""
#include "mip_filter.h"
#include "mip_post.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace astcd;

static void put(const void* p, size_t n) { fwrite(p, 1, n, stdout); }

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	const char* mode = argv[1];
	if (!strcmp(mode, "norm_u8"))                  // every RGB triple, alpha 0x5A
	{
		std::vector<unsigned int> out(1u << 24);
		for (unsigned int i = 0; i < (1u << 24); i++) out[i] = mip_normalize_u8(i | 0x5A000000u);
		put(out.data(), out.size() * 4);
		return 0;
	}
	if (!strcmp(mode, "norm_float"))               // stdin: n, type (1 F16, 2 F32), n texels; stdout: the texels
	{
		unsigned int n, type;
		if (fread(&n, 4, 1, stdin) != 1 || fread(&type, 4, 1, stdin) != 1) return 3;
		const size_t tb = type == 1 ? 8 : 16;
		std::vector<unsigned char> buf((size_t)n * tb);
		if (fread(buf.data(), 1, buf.size(), stdin) != buf.size()) return 3;
		for (unsigned int i = 0; i < n; i++)
		{
			unsigned char* p = &buf[(size_t)i * tb];
			float x[3];
			unsigned short h[4];
			if (type == 1) { memcpy(h, p, 8); for (int c = 0; c < 3; c++) x[c] = mip_float_from_half(h[c]); }
			else memcpy(x, p, 12);
			if (!mip_normalize_float(x)) continue;
			if (type == 1) { for (int c = 0; c < 3; c++) h[c] = mip_half_from_float(x[c]); memcpy(p, h, 6); }
			else memcpy(p, x, 12);
		}
		put(buf.data(), buf.size());
		return 0;
	}
	if (!strcmp(mode, "remap_u8"))                 // every (t, ak, a): t, ak in 1..255, a in 0..255
	{
		std::vector<unsigned char> out(255u * 255u * 256u);
		size_t i = 0;
		for (unsigned int t = 1; t < 256; t++)
			for (unsigned int ak = 1; ak < 256; ak++)
				for (unsigned int a = 0; a < 256; a++) out[i++] = (unsigned char)mip_cover_remap_u8(a, ak, t);
		put(out.data(), out.size());
		return 0;
	}
	if (!strcmp(mode, "remap_float"))              // stdin: n, half, cutoff, then n (a, ak) float pairs; stdout: n floats
	{
		unsigned int n, half;
		float cutoff, hi, lo;
		if (fread(&n, 4, 1, stdin) != 1 || fread(&half, 4, 1, stdin) != 1 || fread(&cutoff, 4, 1, stdin) != 1) return 3;
		mip_cover_bounds(cutoff, half != 0, hi, lo);
		std::vector<float> in(2 * (size_t)n), out(n);
		if (fread(in.data(), 4, in.size(), stdin) != in.size()) return 3;
		for (unsigned int i = 0; i < n; i++) out[i] = mip_cover_remap_float(in[2 * i], in[2 * i + 1], cutoff, hi, lo, half != 0);
		put(out.data(), out.size() * 4);
		return 0;
	}
	if (!strcmp(mode, "constants"))                // stdin: n cutoffs; stdout: per cutoff t, hi32, lo32, hi16, lo16
	{
		unsigned int n;
		if (fread(&n, 4, 1, stdin) != 1) return 3;
		std::vector<float> c(n);
		if (fread(c.data(), 4, n, stdin) != n) return 3;
		for (unsigned int i = 0; i < n; i++)
		{
			float v[5];
			v[0] = (float)mip_cover_u8_threshold(c[i]);
			mip_cover_bounds(c[i], false, v[1], v[2]);
			mip_cover_bounds(c[i], true, v[3], v[4]);
			put(v, sizeof(v));
		}
		return 0;
	}
	if (!strcmp(mode, "target"))                   // stdin: n triples (c0, n, n0) of u64; stdout: n u64
	{
		unsigned int n;
		if (fread(&n, 4, 1, stdin) != 1) return 3;
		std::vector<unsigned long long> in(3 * (size_t)n), out(n);
		if (fread(in.data(), 8, in.size(), stdin) != in.size()) return 3;
		for (unsigned int i = 0; i < n; i++) out[i] = mip_cover_target(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
		put(out.data(), out.size() * 8);
		return 0;
	}
	if (!strcmp(mode, "keys"))                     // every half and a float sample: key, then value of the key
	{
		for (unsigned int h = 0; h < 65536; h++)
		{
			const unsigned int k = mip_key_f16((unsigned short)h);
			const float v = mip_key_f16_value(k);
			put(&k, 4); put(&v, 4);
		}
		return 0;
	}
	return 2;
}
"""


@pytest.fixture(scope="module")
def post_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mippost")
    src, exe = d / "post.cpp", d / "post"
    src.write_text(POST_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _run(exe, mode, data=b""):
    r = subprocess.run([exe, mode], input=data, capture_output=True, timeout=300)
    assert r.returncode == 0, (mode, r.returncode, r.stderr)
    return r.stdout


def test_normalize_every_u8_triple(post_exe):
    got = np.frombuffer(_run(post_exe, "norm_u8"), dtype=np.uint8).reshape(-1, 4)
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i & 0xFF), (i >> 8) & 0xFF, (i >> 16) & 0xFF], axis=-1).astype(np.uint8)
    want = P.normalize_u8(rgb)
    assert np.array_equal(got[:, :3], want), int((got[:, :3] != want).any(axis=1).sum())
    assert (got[:, 3] == 0x5A).all()
    # the result is a unit vector to within the code step
    v = got[:, :3].astype(np.float64) / 127.5 - 1.0
    assert np.abs(np.sqrt((v * v).sum(axis=1)) - 1.0).max() < 0.02


def _float_texels(dtype, rng, n):
    a = (rng.random((n, 4)) * 1.2 - 0.1).astype(dtype)
    with np.errstate(over="ignore"):
        edge = np.array([0.5, 0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, 5e-8, 0.5000001, 0.49999997, 65504.0, 1e30, 1e-45,
                         6e-5, 0.25], dtype=np.float64).astype(dtype)
    m = len(edge)
    combos = np.stack(np.meshgrid(edge, edge, edge, indexing="ij"), axis=-1).reshape(-1, 3)
    e = np.concatenate([combos, np.full((m ** 3, 1), 0.75, dtype)], axis=1).astype(dtype)
    # subnormal-sized components around the zero vector (x == 0.5 is v == 0)
    sub = np.full((64, 4), 0.5, dtype)
    sub[:, :3] += (rng.integers(-3, 4, (64, 3)) * np.finfo(dtype).eps / 4).astype(dtype)
    return np.concatenate([a, e, sub]).astype(dtype)


@pytest.mark.parametrize("dtype,type_code", [(np.float16, 1), (np.float32, 2)])
def test_normalize_float(post_exe, dtype, type_code):
    rng = np.random.default_rng(type_code)
    tex = _float_texels(dtype, rng, 200000)
    raw = _run(post_exe, "norm_float", np.array([len(tex), type_code], np.uint32).tobytes() + tex.tobytes())
    got = np.frombuffer(raw, dtype=dtype).reshape(-1, 4)
    want = P.normalize(tex)
    bits = np.uint16 if dtype == np.float16 else np.uint32
    bad = (got.view(bits) != want.view(bits)).any(axis=1)
    assert not bad.any(), (int(bad.sum()), tex[bad][:4], got[bad][:4], want[bad][:4])
    # the zero vector, inf and NaN texels are unchanged
    zero = (tex[:, :3] == 0.5).all(axis=1)
    assert zero.any() and (got[zero].view(bits) == tex[zero].view(bits)).all()


def test_u8_remap_every_case(post_exe):
    got = np.frombuffer(_run(post_exe, "remap_u8"), dtype=np.uint8).reshape(255, 255, 256)
    t = np.arange(1, 256, dtype=np.int64)[:, None, None]
    ak = np.arange(1, 256, dtype=np.int64)[None, :, None]
    a = np.arange(256, dtype=np.int64)[None, None, :]
    q = (2 * a * t + ak) // (2 * ak)
    want = np.where(a >= ak, np.minimum(255, q), np.minimum(t - 1, q))
    assert np.array_equal(got, want.astype(np.uint8))
    # covered afterwards exactly when a >= a_k
    assert np.array_equal(got >= t, np.broadcast_to(a >= ak, got.shape))
    # ... and the model's vectorised form agrees
    for tt in (1, 77, 128, 255):
        for k in (1, 3, 128, 255):
            assert np.array_equal(P.remap_u8(np.arange(256, dtype=np.uint8), k, tt), got[tt - 1, k - 1])


CUTOFFS = [0.5, 1.0, 0.1, 1.0 / 3.0, 0.75, 1e-8, 1e-45, 0.9999999, 6.1e-5, 0.0039215688, 0.9995]


def test_constants(post_exe):
    c = np.array(CUTOFFS, dtype=np.float32)
    got = np.frombuffer(_run(post_exe, "constants", np.array([len(c)], np.uint32).tobytes() + c.tobytes()), dtype=np.float32).reshape(-1, 5)
    for i, cut in enumerate(c):
        assert int(got[i, 0]) == P.u8_threshold(cut), cut
        for dtype, (hi, lo) in ((np.float32, got[i, 1:3]), (np.float16, got[i, 3:5])):
            mhi, mlo = P.bounds(cut, dtype)
            assert (hi, lo) == (mhi, mlo), (cut, dtype, hi, lo, mhi, mlo)
            assert hi >= cut > lo and np.float32(dtype(hi)) == hi and np.float32(dtype(lo)) == lo
    # t by its definition
    for cut in np.linspace(0.001, 1.0, 997, dtype=np.float32):
        t = P.u8_threshold(cut)
        assert float(t) >= float(cut) * 255.0 and (t == 1 or float(t - 1) < float(cut) * 255.0)


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("cutoff", [0.5, 1.0, 0.1, 1.0 / 3.0, 1e-8])
def test_float_remap_near_the_cutoff(post_exe, dtype, cutoff):
    rng = np.random.default_rng(int(cutoff * 1000) + (dtype == np.float16))
    c = np.float32(cutoff)
    fin = np.finfo(dtype)
    near = [np.nextafter(dtype(c), dtype(0)), dtype(c), np.nextafter(dtype(c), dtype(2)), dtype(1), dtype(0), dtype(-0.0)]
    vals = np.array(near + [np.inf, -np.inf, np.nan, fin.tiny, fin.max, -fin.max, 1e-3, 0.999, 0.5, 2.0], dtype=np.float64).astype(dtype)
    vals = np.concatenate([vals, rng.random(400).astype(dtype), (c * (1 + (rng.random(400) - 0.5) * 1e-3)).astype(dtype)])
    aks = np.concatenate([vals[:300], np.array(near[:3] + [1.0, 1e-4], np.float64).astype(dtype)])
    aks = np.unique(aks[np.isfinite(aks) & (aks > 0)])          # (a_k <= 0 or not finite: the surface is left unchanged)
    a, ak = [x.ravel() for x in np.meshgrid(vals, aks, indexing="ij")]
    pairs = np.stack([a.astype(np.float32), ak.astype(np.float32)], axis=1)
    raw = _run(post_exe, "remap_float", np.array([len(a), int(dtype == np.float16)], np.uint32).tobytes() + c.tobytes() + pairs.tobytes())
    got = np.frombuffer(raw, dtype=np.float32)
    want = np.concatenate([P.remap_float(a[ak == k], k, c, dtype) for k in aks]).astype(np.float32)
    order = np.concatenate([np.nonzero(ak == k)[0] for k in aks])
    g = got[order]
    same = (g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want))
    assert same.all(), (int((~same).sum()), a[order][~same][:4], ak[order][~same][:4], g[~same][:4], want[~same][:4])
    # covered afterwards exactly when a >= a_k (NaN never)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(g.astype(np.float64) >= float(c), a[order].astype(np.float64) >= ak[order].astype(np.float64))


def test_target_count_is_exact(post_exe):
    rng = np.random.default_rng(9)
    cases = [(0, 5, 7), (7, 1, 7), (3, 1, 7), (4, 1, 8), (1, 1, 3), ((1 << 61) - 1, (1 << 59) + 3, (1 << 61) - 1),
             ((1 << 60) + 12345, 1 << 58, (1 << 61) - 5), (1, 1, 2)]
    for _ in range(2000):
        n0 = int(rng.integers(1, 1 << 61, dtype=np.uint64))
        cases.append((int(rng.integers(0, n0 + 1, dtype=np.uint64)) if n0 < (1 << 63) else 0, int(rng.integers(1, n0 + 1, dtype=np.uint64)), n0))
    for _ in range(2000):
        n0 = int(rng.integers(1, 1 << 20))
        cases.append((int(rng.integers(0, n0 + 1)), int(rng.integers(1, n0 + 1)), n0))
    arr = np.array(cases, dtype=np.uint64)
    got = np.frombuffer(_run(post_exe, "target", np.array([len(cases)], np.uint32).tobytes() + arr.tobytes()), dtype=np.uint64)
    for (c0, n, n0), g in zip(cases, got):
        assert int(g) == P.target(c0, n, n0), (c0, n, n0)


def test_keys_order_every_half(post_exe):
    raw = np.frombuffer(_run(post_exe, "keys"), dtype=np.uint32).reshape(-1, 2)
    k, back = raw[:, 0], raw[:, 1].view(np.float32)
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    assert np.array_equal(k.astype(np.int64), P.keys(h))
    nan = np.isnan(h)
    assert (k[nan] == 0).all() and (k[~nan] > 0).all()
    # unsigned key order is numeric order, and a key gives its value back
    f = h[~nan].astype(np.float64)
    o = np.argsort(k[~nan])
    assert (np.diff(f[o]) >= 0).all()
    assert np.array_equal(back[~nan].view(np.uint32), h[~nan].astype(np.float32).view(np.uint32))


def test_model_surfaces_keep_coverage():
    """The model's own coverage property: covered afterwards exactly when a >= a_k, so >= k texels and == k for a unique a_k."""
    rng = np.random.default_rng(4)
    for dtype in (np.uint8, np.float16, np.float32):
        top = rng.integers(0, 256, (1, 64, 64, 4), dtype=np.uint8) if dtype == np.uint8 else rng.random((1, 64, 64, 4)).astype(dtype)
        chain = P.chain(top, P.VOLUME, P.ALPHA_COVERAGE, 0.5)
        c0 = int(P.covered(top[..., 3], 0.5).sum())
        for lv in chain[1:]:
            k = P.target(c0, lv[..., 3].size, top[..., 3].size)
            assert int(P.covered(lv[..., 3], 0.5).sum()) >= k


def test_null_context(product, A):
    import ctypes as C
    swz = A.Swizzle(*A.SWZ_RGBA)
    opts = A.MipOptions(A.MIP_NORMALIZE | A.MIP_ALPHA_COVERAGE, 0.5)
    assert product.lib.astcenc_amd_generate_mip_chain_ex_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, 0, C.byref(opts), 0x2000, 1 << 20,
                                                                None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_compress_mip_chain_ex_device(None, 0x1000, 64, 64, 1, 1, A.TYPE_U8, C.byref(swz), 0, C.byref(opts),
                                                                0x2000, 1 << 20, 0x3000, 1 << 20, None, None) == A.ERR_BAD_PARAM


def test_post_kernels_use_no_scratch(tmp_path, A):
    import test_code_object as T
    if not (os.path.exists(A.LIB_PRODUCT) and os.path.exists(T.BUNDLER) and os.path.exists(T.READELF)):
        pytest.skip("needs the built product library and the ROCm LLVM tools")
    k = T.kernel_descriptors(A.LIB_PRODUCT, str(tmp_path))
    post = {n: d for n, d in k.items() if "astc_mippost_" in n}
    # count, hist, select and apply for U8, F16 and F32
    assert len(post) == 12, sorted(post)
    for n, d in post.items():
        assert d["private_segment_fixed_size"] == 0 and d["vgpr_spill_count"] == 0 and d["sgpr_spill_count"] == 0, (n, d)
        assert d["group_segment_fixed_size"] <= 1024, (n, d)
