#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""A compressed mip chain sampled at a level of detail per point straight into a tensor (astcenc_amd_sample_lod_tensors_device)
against what a user does without that call: the levels and weights of every point computed in torch, the points split by level,
one astcenc_amd_sample_tensors_device call per level touched with a per-level coordinate buffer into a float32 intermediate, the
results scattered back, blended, scaled, shifted and converted in torch into the same tensor.  The source is the 8192^2 RGBA8
image of tools/time_decode_sample.py with its full chain (14 levels), every level compressed at 6x6 -fastest and kept in device
memory, one entry per level; the output is planar fp16 with three channels; BILINEAR, CLAMP, MIP_LINEAR.  Workloads:

  1. a 1920 x 1080 grid under a rotation by 30 degrees about the image's centre at one level-0 texel per point, lambda rising
     smoothly from 0 in the first row to 4 in the last;
  2. the same grid with lambda = 2 everywhere (an integer: one level);
  3. 2^20 uniformly random points (a 1024 x 1024 grid) with lambda uniform over the chain;
  4. the same rotated grid over a chain of one level with lod NULL, against astcenc_amd_sample_tensors_device itself on the same
     points (in texel units), and against that call of another build of the library when --parent-lib names one (the parent commit's).

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does.  The new call's output is checked bit for bit
against the numpy model (tests/sample_lod_model.py) over the texels the library's whole-image decode writes for every level, on
three rows of every grid; the largest absolute difference to the torch way's result is printed and is no pass criterion (its
blend is float32).  Level passes, batches and blocks decoded: counted on the host by the library's own tile routine
(csrc/decode_lod.h, through the `blocks` mode of tests/harness/decode_lod_check.cpp, which this tool compiles with g++ and which
runs the tiles over a chain of constant-colour blocks); --blocks-only does nothing else and needs no GPU, --no-blocks leaves it out.
usage: time_decode_lod.py [reps] [--size N] [--json out.json] [--parent-lib path] [--blocks-only | --no-blocks]"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
size = int(args[args.index("--size") + 1]) if "--size" in args else 8192
out_json = args[args.index("--json") + 1] if "--json" in args else None
parent_path = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
blocks_only, no_blocks = "--blocks-only" in args, "--no-blocks" in args
B = 6
TMP = tempfile.mkdtemp()
HARNESS_EXE = os.path.join(TMP, "decode_lod_check")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def chain_dims(n):
    dims = []
    while True:
        dims.append(max(1, n >> len(dims)))
        if dims[-1] == 1:
            return dims


DIMS = chain_dims(size)
LEVELS = len(DIMS)


def rotated(w, h):
    """Normalised: one level-0 texel per point."""
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    jj, ii = np.meshgrid(np.arange(h) - (h - 1) / 2.0, np.arange(w) - (w - 1) / 2.0, indexing="ij")
    x = size / 2.0 + (c * ii - s * jj)
    y = size / 2.0 + (s * ii + c * jj)
    return (np.stack([x, y], axis=-1) / size).astype(np.float32)


rng = np.random.default_rng(1)
grid = rotated(1920, 1080)
ramp = np.repeat((4.0 * np.arange(1080) / 1079.0).astype(np.float32)[:, None], 1920, axis=1)
# (name, levels of the chain, coords, lod or None)
workloads = (("1920x1080 rotated by 30 degrees, lambda ramping 0..4", LEVELS, grid, ramp),
             ("1920x1080 rotated by 30 degrees, lambda = 2", LEVELS, grid, np.full((1080, 1920), 2.0, dtype=np.float32)),
             ("2^20 uniformly random points, lambda uniform over the chain", LEVELS, rng.uniform(0.0, 1.0, size=(1024, 1024, 2)).astype(np.float32),
              rng.uniform(0.0, LEVELS - 1.0, size=(1024, 1024)).astype(np.float32)),
             ("1920x1080 rotated by 30 degrees, one level, lod NULL", 1, grid, None))


def blocks_decoded(levels, coords, lod):
    """By the library's own tile routine: the `blocks` mode of tests/harness/decode_lod_check.cpp runs decode_lod_tile over every
    tile decode_lod_build makes of the grid and sums the passes, batches and blocks it reports."""
    if not os.path.exists(HARNESS_EXE):
        subprocess.run(["g++", "-std=c++17", "-O2", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"),
                        os.path.join(ROOT, "tests", "harness", "decode_lod_check.cpp"), "-o", HARNESS_EXE], check=True)
    cpath, lpath = os.path.join(TMP, "coords.f32"), os.path.join(TMP, "lod.f32")
    coords.astype(np.float32).tofile(cpath)
    if lod is not None:
        lod.astype(np.float32).tofile(lpath)
    h, w = coords.shape[:2]
    res = subprocess.run([HARNESS_EXE, "blocks", "1", "0", "0", "1", str(B), str(B), str(size), str(size), str(levels), str(w), str(h), cpath,
                          lpath if lod is not None else "-"], capture_output=True, text=True, check=True)
    f = res.stdout.split()
    n = {"tiles": int(f[1]), "passes": int(f[3]), "batches": int(f[5]), "decoded": int(f[7]), "points": int(f[9])}
    return dict(n, passes_per_tile=round(n["passes"] / n["tiles"], 3), batches_per_tile=round(n["batches"] / n["tiles"], 3),
                decoded_per_point=round(n["decoded"] / n["points"], 4))


if blocks_only:
    rows = []
    for name, levels, coords, lod in workloads:
        row = {"workload": name, "blocks": blocks_decoded(levels, coords, lod)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    sys.exit(0)

import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import sample_lod_model as L  # noqa: E402
import tensor_model as M  # noqa: E402

assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
parent = A.Library(parent_path) if parent_path else None
stream = torch.cuda.current_stream()

# the streams: level 0 is a quarter of the image compressed and tiled (the decoder's time depends on the kinds of block, not on
# where they are); every other level is the synthetic image of its own size, compressed
streams = []
for l, n in enumerate(DIMS):
    if l == 0 and size >= 2 * B:
        tile = size // 2
        part = lib.compress(A.synthetic_image(tile, tile), (B, B), A.PRE_FASTEST).reshape(-(-tile // B), -(-tile // B), 16)
        nb = -(-size // B)
        data = np.tile(part, (2, 2, 1))[:nb, :nb].copy().reshape(-1)
    else:
        data = lib.compress(A.synthetic_image(n, n, seed=l + 1), (B, B), A.PRE_FASTEST).reshape(-1)
    streams.append(torch.from_numpy(np.ascontiguousarray(data)).cuda())


def make_context(library):
    err, cfg = library.config_init(A.PRF_LDR, B, B, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, ctx = library.context_alloc(cfg, 1)
    assert err == 0
    return ctx


ctx = make_context(lib)
parent_ctx = make_context(parent) if parent else None
entries = [A.compressed_entry(s, (n, n), A.TYPE_U8) for s, n in zip(streams, DIMS)]
entry_arr = (A.ImageSetEntry * LEVELS)(*entries)
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
plain32 = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 3)                 # the per-level intermediate of the torch way
scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
lod_sampler = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
sampler = A.Sampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP)
scale_t = torch.tensor(scale32[:3], device="cuda").view(3, 1)
bias_t = torch.tensor(bias32[:3], device="cuda").view(3, 1)
dims_t = torch.tensor(DIMS, dtype=torch.float32, device="cuda")


def decode_level(l):
    n = DIMS[l]
    scratch = torch.zeros((n, n, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
    e = lib.lib.astcenc_amd_decompress_image_device(ctx, C.c_void_p(streams[l].data_ptr()), streams[l].numel(), C.c_void_p(scratch.data_ptr()), n, n, 1,
                                                    A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), stream.cuda_stream)
    assert e == 0, e
    torch.cuda.synchronize()
    return scratch.cpu().numpy()


def sample_lod(prepared):
    e = lib.lib.astcenc_amd_sample_lod_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(lod_sampler), prepared, 1, stream.cuda_stream)
    assert e == 0, e


def sample_one(library, context, prepared):
    e = library.lib.astcenc_amd_sample_tensors_device(context, entry_arr, LEVELS, C.byref(fmt), C.byref(sampler), prepared, 1, stream.cuda_stream)
    assert e == 0, e


def per_level(levels, uv, lod, out):
    """What a user does today: levels and weights in torch, a sample call per level touched, gather, blend, scale, shift, fp16."""
    h, w = uv.shape[:2]
    flat = uv.reshape(-1, 2)
    lam = torch.zeros(h * w, device="cuda") if lod is None else lod.reshape(-1)
    lc = lam.clamp(0.0, float(levels - 1))
    l0 = lc.floor()
    g = lc - l0
    l0 = l0.long()
    l1 = torch.where(g != 0, l0 + 1, torch.full_like(l0, -1))
    s0 = torch.zeros((3, h * w), dtype=torch.float32, device="cuda")
    s1 = torch.zeros((3, h * w), dtype=torch.float32, device="cuda")
    touched = torch.unique(torch.cat([l0, l1[l1 >= 0]])).tolist()           # (the host learns the levels: a synchronisation)
    for l in touched:
        first, second = (l0 == l).nonzero().squeeze(1), (l1 == l).nonzero().squeeze(1)
        idx = torch.cat([first, second])
        # (a grid is at most 65535 points across: the list is folded into rows of 32768, the last one padded with point 0)
        n, cols = idx.numel(), min(idx.numel(), 32768)
        rows_l = -(-n // cols)
        padded = torch.cat([idx, idx.new_zeros(rows_l * cols - n)])
        xy = (flat[padded] * dims_t[l]).contiguous().view(rows_l, cols, 2)  # per-level coordinate buffer, in texel units
        part = torch.empty((3, rows_l, cols), dtype=torch.float32, device="cuda")
        e = lib.sample_tensors_device(ctx, entries, plain32, sampler, [(l, 0, xy, part)], stream=stream.cuda_stream)
        assert e == 0, e
        part = part.view(3, -1)
        s0[:, first] = part[:, :first.numel()]
        s1[:, second] = part[:, first.numel():n]
    s = torch.where((l1 >= 0)[None], (1.0 - g)[None] * s0 + g[None] * s1, s0)
    out.copy_((s * scale_t + bias_t).half().view(3, h, w))


def timed_ms(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn(*a)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = sorted(t)
    return {"best_ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4)}


whole = [decode_level(l) for l in range(LEVELS)]
rows = []
for name, levels, coords, lod in workloads:
    h, w = coords.shape[:2]
    duv = torch.from_numpy(coords).cuda()
    dlod = torch.from_numpy(lod).cuda() if lod is not None else None
    out = {k: torch.zeros((3, h, w), dtype=torch.float16, device="cuda") for k in ("lod", "other", "parent")}
    prepared = (A.LodGrid * 1)(A.lod_grid(0, levels, 0, duv, dlod, out["lod"], type=A.TENSOR_F16))
    ways = {"lod": lambda: sample_lod(prepared)}
    if levels == 1:
        # (8192 is a power of two: u W is a binary32, so the sample call at (u W, v H) writes the same bytes)
        dxy = (duv * float(DIMS[0])).contiguous()
        one = (A.SampleGrid * 1)(A.sample_grid(0, 0, dxy, out["other"], type=A.TENSOR_F16))
        ways["sample_call"] = lambda: sample_one(lib, ctx, one)
        if parent:
            one_parent = (A.SampleGrid * 1)(A.sample_grid(0, 0, dxy, out["parent"], type=A.TENSOR_F16))
            ways["sample_call_of_parent_build"] = lambda: sample_one(parent, parent_ctx, one_parent)
    else:
        ways["sample_call_per_level_and_torch"] = lambda: per_level(levels, duv, dlod, out["other"])
    torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
    for fn in ways.values():                                               # warm-up of every way
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(reps):                                                  # alternating
        for k, fn in ways.items():
            t[k].append(timed_ms(fn))
    rows_checked = sorted({0, h // 2, h - 1})
    want = L.tensor([x for x in whole[:levels]], L.S.BILINEAR, L.S.CLAMP, L.S.CLAMP, L.MIP_LINEAR, coords[rows_checked], None if lod is None else lod[rows_checked], 0.0,
                    M.F16, M.PLANAR, 3, scale32, bias32)
    got = out["lod"][:, rows_checked].view(torch.int16).cpu().numpy().view(np.uint16)
    points = h * w
    row = {"workload": name, "points": points, "levels": levels, "reps": reps, "model_points": len(rows_checked) * w, "model_differences": int((got != want).sum())}
    for k in ways:
        row[k] = dict(stats(t[k]), mpoints_per_s=round(points / min(t[k]) / 1e3, 1))
        if k != "lod":
            row[k + "_over_lod_best"] = round(min(t[k]) / min(t["lod"]), 3)
            row[k + "_over_lod_median"] = round(sorted(t[k])[reps // 2] / sorted(t["lod"])[reps // 2], 3)
    if levels == 1:
        row["bytes_equal_to_sample_call"] = bool(torch.equal(out["lod"].view(torch.int16), out["other"].view(torch.int16)))
        if parent:
            row["bytes_equal_to_parent_sample_call"] = bool(torch.equal(out["lod"].view(torch.int16), out["parent"].view(torch.int16)))
    else:
        row["max_abs_difference_to_torch_way"] = float((out["lod"].float() - out["other"].float()).abs().max())
    if not no_blocks:
        row["blocks"] = blocks_decoded(levels, coords, lod)
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"rows": rows, "model_exact": all(r["model_differences"] == 0 for r in rows)}
print(json.dumps({"model_exact": summary["model_exact"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
