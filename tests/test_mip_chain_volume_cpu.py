# SPDX-License-Identifier: Apache-2.0
"""Mip chains of texture arrays, cube maps and volumes without a GPU (astcenc_amd_mip_chain_volume_layout, csrc/mip_filter.h).

  * the layout of both kinds: level dimensions, 256-byte aligned texel offsets, block offsets and totals for 2D and 3D
    footprints and all three data types; an ARRAY with a 3D footprint, a level_count beyond the full chain, overflow, a null
    config or layout; a VOLUME of depth 1 has the 2D layout;
  * the 3D filter functions of the header compiled with g++, bit for bit against the numpy model (tests/mip_model_3d.py) on
    every x, y, z in 1..7; the model's VOLUME of depth 1 is the 2D model's chain;
  * the KTX chain writer and reader: 2D arrays, cube maps, cube-map arrays and 3D-footprint volumes;
  * a null context on every entry point."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mip_model as M  # noqa: E402
import mip_model_3d as V  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "astc-encoder_amd", "csrc")

FILTER_MAIN = r"""
#include "mip_filter.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
using namespace astcd;

// stdin: "type srgb w h d levels\n" then level 0 (d slices of RGBA rows of U8 = 0 / F16 = 1 / F32 = 2); stdout: levels 1 ..
int main()
{
	unsigned int type, srgb, w, h, d, levels;
	if (scanf("%u %u %u %u %u %u", &type, &srgb, &w, &h, &d, &levels) != 6) return 2;
	getchar();
	const size_t tb = type == 0 ? 4 : type == 1 ? 8 : 16;
	std::vector<unsigned char> src((size_t)w * h * d * tb);
	if (fread(src.data(), 1, src.size(), stdin) != src.size()) return 3;
	double tables[MIP_SRGB_TABLE_DOUBLES];
	mip_srgb_tables_build(tables, [](double x, double y) { return std::pow(x, y); });
	for (unsigned int l = 1; l < levels; l++)
	{
		const unsigned int dx = mip_level_dim(w, 1), dy = mip_level_dim(h, 1), dz = mip_level_dim(d, 1);
		std::vector<unsigned char> dst((size_t)dx * dy * dz * tb);
		for (unsigned int z = 0; z < dz; z++)
		for (unsigned int y = 0; y < dy; y++)
			for (unsigned int x = 0; x < dx; x++)
			{
				const MipTaps tx = mip_axis_taps(w, x), ty = mip_axis_taps(h, y), tz = mip_axis_taps(d, z);
				const size_t o = (((size_t)z * dy + y) * dx + x) * tb;
				if (type == 0)
				{
					const unsigned int v = mip_texel_u8_3d(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz) {
						unsigned int p; memcpy(&p, &src[(((size_t)sz * h + sy) * w + sx) * 4], 4); return p; }, srgb ? tables : nullptr, tables + 256);
					memcpy(&dst[o], &v, 4);
				}
				else
				{
					float out[4];
					mip_texel_float_3d(tx, ty, tz, [&](unsigned int sx, unsigned int sy, unsigned int sz, float v[4]) {
						const size_t i = (((size_t)sz * h + sy) * w + sx) * tb;
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
		src.swap(dst); w = dx; h = dy; d = dz;
	}
	if (mip_full_levels_3d(5, 3, 7) != 3 || mip_full_levels_3d(1, 1, 256) != 9 || mip_full_levels_3d(9, 2, 1) != 4) return 4;
	return 0;
}
"""


@pytest.fixture(scope="module")
def filter_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("mipfilter3d")
    src, exe = d / "filter3d.cpp", d / "filter3d"
    src.write_text(FILTER_MAIN)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-I" + CSRC, "-o", str(exe), str(src)], check=True)
    return str(exe)


def _run_filter(exe, vol, srgb=False):
    """The header's full volume chain of vol ([D, H, W, 4]): [vol, level 1, ...]."""
    d, h, w = vol.shape[:3]
    dims = V.level_dims(w, h, d)
    t = {np.dtype(np.uint8): 0, np.dtype(np.float16): 1, np.dtype(np.float32): 2}[vol.dtype]
    inp = ("%d %d %d %d %d %d\n" % (t, int(srgb), w, h, d, len(dims))).encode() + np.ascontiguousarray(vol).tobytes()
    r = subprocess.run([exe], input=inp, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, at = [vol], 0
    for lw, lh, ld in dims[1:]:
        n = lw * lh * ld * 4
        out.append(np.frombuffer(r.stdout, dtype=vol.dtype, count=n, offset=at).reshape(ld, lh, lw, 4))
        at += n * vol.dtype.itemsize
    assert at == len(r.stdout)
    return out


def _random(rng, shape, kind):
    if kind == "u8":
        return rng.integers(0, 256, shape + (4,), dtype=np.uint8)
    if kind == "f16":
        return (rng.standard_normal(shape + (4,)) * 4).astype(np.float16)
    if kind == "f32-extreme":
        mag = np.float32(10.0) ** rng.integers(-45, 39, shape + (4,)).astype(np.float32)
        sign = np.where(rng.integers(0, 2, shape + (4,)) == 1, np.float32(-1), np.float32(1))
        v = (rng.random(shape + (4,)).astype(np.float32) + np.float32(0.5)) * mag * sign
        v[rng.random(shape + (4,)) < 0.05] = np.float32(3.4028235e38)
        v[rng.random(shape + (4,)) < 0.05] = np.float32(-0.0)
        return v.astype(np.float32)
    return (rng.standard_normal(shape + (4,)) * 100).astype(np.float32)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,srgb", [("u8", False), ("u8", True), ("f16", False), ("f32", False), ("f32-extreme", False)])
def test_3d_filter_header_matches_numpy_model(filter_exe, kind, srgb):
    rng = np.random.default_rng(11 + len(kind) + srgb)
    for w in range(1, 8):
        for h in range(1, 8):
            for d in range(1, 8):
                vol = _random(rng, (d, h, w), kind)
                got = _run_filter(filter_exe, vol, srgb)
                want = V.chain_volume(vol, srgb=srgb)
                assert len(got) == len(want) == V.full_levels(w, h, d)
                for i, (g, m) in enumerate(zip(got, want)):
                    assert _same(g, m), (kind, srgb, (w, h, d), "level %d" % i)


@pytest.mark.parametrize("kind,srgb", [("u8", False), ("u8", True), ("f16", False), ("f32-extreme", False)])
def test_volume_of_depth_one_is_the_2d_chain(filter_exe, kind, srgb):
    rng = np.random.default_rng(5 + srgb)
    for w, h in [(w, h) for w in range(1, 10) for h in range(1, 10)] + [(33, 17), (1, 37)]:
        img = _random(rng, (h, w), kind)
        want = M.chain(img, srgb=srgb)
        model = V.chain_volume(img[None], srgb=srgb)
        header = _run_filter(filter_exe, img[None], srgb)
        assert len(model) == len(header) == len(want)
        for i, (a, b, m) in enumerate(zip(model, header, want)):
            assert _same(a, m[None]) and _same(b, m[None]), (kind, srgb, (w, h), "level %d" % i)


def test_array_model_is_per_layer():
    rng = np.random.default_rng(3)
    layers = rng.integers(0, 256, (6, 13, 9, 4), dtype=np.uint8)
    got = V.chain_array(layers, srgb=True)
    for l in range(6):
        for i, m in enumerate(M.chain(layers[l], srgb=True)):
            assert _same(got[i][l], m)


LAYOUT_SIZES = [(1, 1, 1), (5, 3, 7), (7, 1, 6), (64, 64, 256), (255, 190, 6), (1, 1, 256), (4096, 17, 7), (130, 66, 33)]


def _expected(w, h, d, kind, block, tb, levels):
    dims = V.level_dims(w, h, d, kind, levels)
    texels, blocks, offs = 0, 0, []
    for i, (lw, lh, ld) in enumerate(dims):
        bo = blocks
        blocks += -(-lw // block[0]) * -(-lh // block[1]) * -(-ld // block[2]) * 16
        to = 0
        if i:
            texels = (texels + 255) // 256 * 256
            to = texels
            texels += lw * lh * ld * tb
        offs.append((to, bo))
    return dims, offs, texels, blocks


@pytest.mark.parametrize("block", [(4, 4, 1), (6, 6, 1), (8, 5, 1), (4, 4, 4), (6, 6, 6), (3, 3, 3), (6, 5, 5)])
@pytest.mark.parametrize("kind", [0, 1])
def test_layout(product, A, block, kind):
    err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], block[2], A.PRE_MEDIUM, 0)
    assert err == A.SUCCESS
    for w, h, d in LAYOUT_SIZES:
        for dtype, tb in ((A.TYPE_U8, 4), (A.TYPE_F16, 8), (A.TYPE_F32, 16)):
            full = V.full_levels(w, h, d, kind)
            for levels in (0, 1, min(3, full), full):
                err, lay = product.mip_chain_volume_layout(cfg, w, h, d, kind, dtype, levels)
                if kind == A.MIP_ARRAY and block[2] > 1:
                    assert err == A.ERR_BAD_PARAM and lay.level_count == 0 and lay.blocks_len == 0
                    continue
                assert err == A.SUCCESS, (w, h, d, levels)
                dims, offs, texels, blocks = _expected(w, h, d, kind, block, tb, levels)
                assert lay.level_count == len(dims) == (full if levels == 0 else levels)
                for i, ((lw, lh, ld), (to, bo)) in enumerate(zip(dims, offs)):
                    assert (lay.dim_x[i], lay.dim_y[i], lay.dim_z[i]) == (lw, lh, ld)
                    assert lay.texels_offset[i] == to and to % 256 == 0 and lay.blocks_offset[i] == bo
                assert lay.texels_len == texels and lay.blocks_len == blocks
                for i in range(len(dims), A.MAX_MIP_LEVELS):
                    assert lay.dim_x[i] == 0 and lay.dim_z[i] == 0 and lay.texels_offset[i] == 0
            assert product.mip_chain_volume_layout(cfg, w, h, d, kind, dtype, full + 1)[0] == A.ERR_BAD_PARAM


def test_layout_counts_and_rejects(product, A):
    err, cfg = product.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, 0)
    # the full chain: every axis for a volume, x and y alone for an array
    assert product.mip_chain_volume_layout(cfg, 4, 4, 256, A.MIP_VOLUME, A.TYPE_U8, 0)[1].level_count == 9
    assert product.mip_chain_volume_layout(cfg, 4, 4, 256, A.MIP_ARRAY, A.TYPE_U8, 0)[1].level_count == 3
    lay = product.mip_chain_volume_layout(cfg, 4, 4, 256, A.MIP_ARRAY, A.TYPE_U8, 0)[1]
    assert [lay.dim_z[i] for i in range(3)] == [256, 256, 256]
    # a bad dimension, type or kind
    for w, h, d, kind, t in ((0, 5, 5, 1, A.TYPE_U8), (5, 0, 5, 1, A.TYPE_U8), (5, 5, 0, 1, A.TYPE_U8), (5, 5, 0, 0, A.TYPE_U8),
                             (5, 5, 5, 2, A.TYPE_U8), (5, 5, 5, -1, A.TYPE_U8), (5, 5, 5, 1, 3), (5, 5, 5, 0, -1)):
        assert product.mip_chain_volume_layout(cfg, w, h, d, kind, t, 0)[0] == A.ERR_BAD_PARAM, (w, h, d, kind, t)
    # bytes beyond size_t: texels, then blocks (a 4x4 footprint: 1 byte per texel, less than F32 texels' 16)
    big = 0xFFFFFFFF
    assert product.mip_chain_volume_layout(cfg, big, big, big, A.MIP_VOLUME, A.TYPE_F32, 0)[0] == A.ERR_BAD_PARAM
    assert product.mip_chain_volume_layout(cfg, big, big, 2, A.MIP_ARRAY, A.TYPE_U8, 1)[0] == A.ERR_BAD_PARAM
    assert product.mip_chain_volume_layout(cfg, big, 1 << 20, 1, A.MIP_ARRAY, A.TYPE_U8, 1)[0] == A.SUCCESS
    # a null config or layout
    assert product.lib.astcenc_amd_mip_chain_volume_layout(C.byref(cfg), 5, 5, 5, 1, A.TYPE_U8, 0, None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_mip_chain_volume_layout(None, 5, 5, 5, 1, A.TYPE_U8, 0,
                                                           C.byref(A.MipChainVolumeLayout())) == A.ERR_BAD_PARAM


@pytest.mark.parametrize("block", [(4, 4, 1), (6, 6, 1), (12, 12, 1), (4, 4, 4), (6, 5, 5)])
def test_volume_of_depth_one_has_the_2d_layout(product, A, block):
    err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], block[2], A.PRE_MEDIUM, 0)
    for w, h in ((1, 1), (5, 3), (255, 190), (4096, 17), (8192, 8192), (0xFFFFFFFF, 1)):
        for dtype in (A.TYPE_U8, A.TYPE_F16, A.TYPE_F32):
            for levels in (0, 1, 2):
                e2, l2 = product.mip_chain_layout(cfg, w, h, dtype, levels)
                e3, l3 = product.mip_chain_volume_layout(cfg, w, h, 1, A.MIP_VOLUME, dtype, levels)
                assert e2 == e3 == (A.SUCCESS if levels <= M.full_levels(w, h) else A.ERR_BAD_PARAM), (w, h, levels)
                assert l2.level_count == l3.level_count
                for i in range(A.MAX_MIP_LEVELS):
                    assert (l2.dim_x[i], l2.dim_y[i], l2.texels_offset[i], l2.blocks_offset[i]) == \
                           (l3.dim_x[i], l3.dim_y[i], l3.texels_offset[i], l3.blocks_offset[i])
                    assert l3.dim_z[i] == (1 if i < l3.level_count else 0)
                assert (l2.texels_len, l2.blocks_len) == (l3.texels_len, l3.blocks_len)


def test_null_context(product, A):
    swz = A.Swizzle(*A.SWZ_RGBA)
    assert product.lib.astcenc_amd_generate_mip_chain_volume_device(None, 0x1000, 64, 64, 8, 1, A.TYPE_U8, 0, 0x2000, 1 << 20,
                                                                    None) == A.ERR_BAD_PARAM
    assert product.lib.astcenc_amd_compress_mip_chain_volume_device(None, 0x1000, 64, 64, 8, 1, A.TYPE_U8, C.byref(swz), 0, 0x2000, 1 << 20,
                                                                    0x3000, 1 << 20, None, None) == A.ERR_BAD_PARAM


def _blocks(rng, w, h, d, layers, faces, block, levels):
    bz = block[2] if len(block) > 2 else 1
    out = []
    for i in range(levels):
        lw, lh, ld = max(1, w >> i), max(1, h >> i), max(1, d >> i)
        n = -(-lw // block[0]) * -(-lh // block[1]) * -(-ld // bz) * max(layers, 1) * faces
        out.append(rng.integers(0, 256, n * 16, dtype=np.uint8))
    return out


@pytest.mark.parametrize("what,w,h,depth,layers,faces,block,levels", [
    ("2d array", 100, 60, 1, 5, 1, (6, 6), 7),
    ("cube map", 64, 64, 1, 0, 6, (4, 4), 7),
    ("cube map array", 32, 32, 1, 3, 6, (8, 8), 6),
    ("volume", 40, 24, 20, 0, 1, (4, 4, 4), 6),
    ("2d", 33, 17, 1, 0, 1, (5, 4), 6),
])
def test_ktx_chain_round_trip(A, tmp_path, what, w, h, depth, layers, faces, block, levels):
    rng = np.random.default_rng(len(what))
    data = _blocks(rng, w, h, depth, layers, faces, block, levels)
    path = str(tmp_path / "chain.ktx")
    A.write_ktx_chain(path, data, w, h, block, depth=depth, layers=layers, faces=faces, srgb=what == "cube map")
    got = A.read_ktx_chain(path)
    bz = block[2] if len(block) > 2 else 1
    assert (got["w"], got["h"], got["depth"], got["layers"], got["faces"]) == (w, h, depth, layers, faces), what
    assert got["block"] == (block[0], block[1], bz) and got["srgb"] == (what == "cube map")
    assert len(got["levels"]) == levels
    for g, b in zip(got["levels"], data):
        assert np.array_equal(g, b)
    # the header fields and every level's imageSize
    raw = open(path, "rb").read()
    fields = struct.unpack_from("<13I", raw, 12)
    assert fields[0] == 0x04030201 and fields[4] == A.ktx_gl_format(block, what == "cube map")
    assert fields[6:13] == (w, h, depth if depth > 1 else 0, layers, faces, levels, 0)
    at = 64
    for b in data:
        n = struct.unpack_from("<I", raw, at)[0]
        assert n == (b.size // 6 if (faces == 6 and layers == 0) else b.size), what
        at += 4 + b.size
    assert at == len(raw)
    # a single-level reader sees the first level (or face)
    first = A.read_ktx(path)
    assert (first[1], first[2], first[3]) == (w, h, depth)


def test_ktx_chain_errors(A, tmp_path):
    path = str(tmp_path / "bad.ktx")
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="3D footprint"):
        A.write_ktx_chain(path, _blocks(rng, 16, 16, 8, 0, 1, (4, 4), 1), 16, 16, (4, 4), depth=8)
    with pytest.raises(ValueError, match="square"):
        A.write_ktx_chain(path, _blocks(rng, 16, 8, 1, 0, 6, (4, 4), 1), 16, 8, (4, 4), faces=6)
    with pytest.raises(ValueError, match="level 0"):
        A.write_ktx_chain(path, [np.zeros(32, np.uint8)], 16, 16, (4, 4), layers=2)
    # a truncated file and a wrong imageSize are refused
    A.write_ktx_chain(path, _blocks(rng, 16, 16, 1, 2, 1, (4, 4), 3), 16, 16, (4, 4), layers=2)
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-16])
    with pytest.raises(ValueError):
        A.read_ktx_chain(path)
    open(path, "wb").write(raw[:64] + struct.pack("<I", 16) + raw[68:])
    with pytest.raises(ValueError, match="level 0"):
        A.read_ktx_chain(path)
