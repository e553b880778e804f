#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""A compressed image sampled at a buffer of coordinates straight into a tensor (astcenc_amd_sample_tensors_device) against what
a user does without that call: astcenc_amd_decompress_image_device into a scratch RGBA8 image of the whole size, then the torch
chain around grid_sample -- convert, permute, grid_sample(mode="bilinear", padding_mode="border", align_corners=False), scale,
shift, convert -- into the same tensor.  The chain is timed both with and without the whole-image decode in it (without: the
decoded image is resident, which costs its bytes in HBM).  The source is the 8192^2 RGBA8 image of tools/time_decode_tensors.py,
compressed at 6x6 -fastest and kept in device memory; the output is planar fp16 with three channels.  Three workloads:

  1. a 1920 x 1080 grid under a rotation by 30 degrees about the image's centre at one texel per point;
  2. the same at four texels per point (its corners leave the image: clamped by both ways);
  3. 2^20 uniformly random points (a 1024 x 1024 grid).

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does (every buffer is allocated once, outside the timed
window).  The new call's output is checked bit for bit against the numpy model (tests/sample_model.py) over the texels the
library's whole-image decode writes; the largest absolute difference to torch's float32 result is printed and is no pass
criterion: torch's float32 weights are another, inexact definition.  Blocks decoded per point: counted on the host by the
library's own tile routine (csrc/decode_sample.h, through the `blocks` mode of tests/harness/decode_sample_check.cpp, which this
tool compiles with g++ and which runs the tiles over an image of constant-colour blocks).
usage: time_decode_sample.py [reps] [--size N] [--json out.json]"""
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
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import sample_model as S  # noqa: E402
import tensor_model as M  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
size = int(args[args.index("--size") + 1]) if "--size" in args else 8192
out_json = args[args.index("--json") + 1] if "--json" in args else None
B = 6
TMP = tempfile.mkdtemp()
HARNESS_EXE = os.path.join(TMP, "decode_sample_check")
subprocess.run(["g++", "-std=c++17", "-O2", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"),
                os.path.join(ROOT, "tests", "harness", "decode_sample_check.cpp"), "-o", HARNESS_EXE], check=True)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()

# the stream: a quarter of the image is compressed and tiled (the decoder's time depends on the kinds of block, not on where they are)
tile = size // 2
part = lib.compress(A.synthetic_image(tile, tile), (B, B), A.PRE_FASTEST).reshape(-(-tile // B), -(-tile // B), 16)
nb = -(-size // B)
blocks = torch.from_numpy(np.tile(part, (2, 2, 1))[:nb, :nb].copy().reshape(-1)).cuda()
err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
entry = A.compressed_entry(blocks, (size, size), A.TYPE_U8)
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
sampler = A.Sampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP)
scale_t = torch.tensor(scale32[:3], device="cuda").view(1, 3, 1, 1)
bias_t = torch.tensor(bias32[:3], device="cuda").view(1, 3, 1, 1)
scratch = torch.zeros((size, size, 4), dtype=torch.uint8, device="cuda")      # the whole image, decoded: what the chain keeps resident


def decode_whole():
    e = lib.lib.astcenc_amd_decompress_image_device(ctx, C.c_void_p(blocks.data_ptr()), blocks.numel(), C.c_void_p(scratch.data_ptr()), size, size, 1,
                                                    A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), stream.cuda_stream)
    assert e == 0, e


def sample(prepared):
    e = lib.lib.astcenc_amd_sample_tensors_device(ctx, C.byref(entry), 1, C.byref(fmt), C.byref(sampler), prepared, 1, stream.cuda_stream)
    assert e == 0, e


def chain(norm_grid, out, with_decode):
    """What a user does today (codes 0 .. 255 as float32, channels first, grid_sample, scale, shift, fp16)."""
    if with_decode:
        decode_whole()
    src = scratch[..., :3].permute(2, 0, 1)[None].float()
    got = torch.nn.functional.grid_sample(src, norm_grid, mode="bilinear", padding_mode="border", align_corners=False)
    out.copy_((got * scale_t + bias_t)[0].half())


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


def blocks_decoded(coords):
    """By the library's own tile routine: the `blocks` mode of tests/harness/decode_sample_check.cpp runs decode_sample_tile over
    every tile decode_sample_build makes of the grid and sums the batches and blocks it reports."""
    path = os.path.join(TMP, "coords.f32")
    coords.astype(np.float32).tofile(path)
    h, w = coords.shape[:2]
    res = subprocess.run([HARNESS_EXE, "blocks", "1", "0", "0", str(B), str(B), str(size), str(size), str(w), str(h), path], capture_output=True, text=True, check=True)
    f = res.stdout.split()
    return {"tiles": int(f[1]), "batches": int(f[3]), "decoded": int(f[5]), "points": int(f[7])}


def rotated(w, h, texels_per_point):
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    jj, ii = np.meshgrid(np.arange(h) - (h - 1) / 2.0, np.arange(w) - (w - 1) / 2.0, indexing="ij")
    x = size / 2.0 + texels_per_point * (c * ii - s * jj)
    y = size / 2.0 + texels_per_point * (s * ii + c * jj)
    return np.stack([x, y], axis=-1).astype(np.float32)


rng = np.random.default_rng(1)
workloads = (("1920x1080 rotated by 30 degrees, 1 texel per point", rotated(1920, 1080, 1.0)),
             ("1920x1080 rotated by 30 degrees, 4 texels per point", rotated(1920, 1080, 4.0)),
             ("2^20 uniformly random points", rng.uniform(0.0, size, size=(1024, 1024, 2)).astype(np.float32)))
decode_whole()
torch.cuda.synchronize()
whole = scratch.cpu().numpy()
rows = []
for name, coords in workloads:
    h, w = coords.shape[:2]
    # (the corners of the second workload lie outside the image: ADDRESS_CLAMP there, as padding_mode="border" for the chain)
    dcoords = torch.from_numpy(coords).cuda()
    norm_grid = (dcoords * (2.0 / size) - 1.0)[None]                       # torch's mapping for align_corners=False: x = (g + 1) * W / 2
    out = {k: torch.zeros((3, h, w), dtype=torch.float16, device="cuda") for k in ("sample", "chain")}
    prepared = (A.SampleGrid * 1)(A.sample_grid(0, 0, dcoords, out["sample"], type=A.TENSOR_F16))
    sample(prepared)                                                       # warm-up of every way
    chain(norm_grid, out["chain"], True)
    chain(norm_grid, out["chain"], False)
    torch.cuda.synchronize()
    t = {"sample": [], "chain_with_decode": [], "chain_resident": []}
    for _ in range(reps):                                                  # alternating
        t["sample"].append(timed_ms(sample, prepared))
        t["chain_with_decode"].append(timed_ms(chain, norm_grid, out["chain"], True))
        t["chain_resident"].append(timed_ms(chain, norm_grid, out["chain"], False))
    # the model over a band of rows of the grid (the whole of it is minutes of numpy at these sizes)
    rows_checked = sorted({0, h // 2, h - 1})
    want = S.tensor(whole, S.BILINEAR, S.CLAMP, S.CLAMP, coords[rows_checked], M.F16, M.PLANAR, 3, scale32, bias32)
    got = out["sample"][:, rows_checked].view(torch.int16).cpu().numpy().view(np.uint16)
    points = h * w
    row = {"workload": name, "points": points, "reps": reps,
           "sample": dict(stats(t["sample"]), mpoints_per_s=round(points / min(t["sample"]) / 1e3, 1)),
           "chain_with_whole_image_decode": stats(t["chain_with_decode"]), "chain_on_a_resident_decoded_image": stats(t["chain_resident"]),
           "chain_with_decode_over_sample_best": round(min(t["chain_with_decode"]) / min(t["sample"]), 3),
           "chain_resident_over_sample_best": round(min(t["chain_resident"]) / min(t["sample"]), 3),
           "model_points": len(rows_checked) * w, "model_differences": int((got != want).sum()),
           "max_abs_difference_to_torch": float((out["sample"].float() - out["chain"].float()).abs().max()),
           "resident_bytes": {"sample": int(blocks.numel()), "chain": int(blocks.numel() + scratch.numel()), "chain_transient_float32": int(3 * 4 * size * size)}}
    counted = blocks_decoded(coords)
    row["blocks"] = dict(counted, decoded_per_point=round(counted["decoded"] / counted["points"], 4), batches_per_tile=round(counted["batches"] / counted["tiles"], 3))
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"rows": rows, "model_exact": all(r["model_differences"] == 0 for r in rows)}
print(json.dumps({"model_exact": summary["model_exact"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
