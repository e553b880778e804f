#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The gradients of the level-of-detail sampler (astcenc_amd_sample_lod_grad_device) timed against the forward call and against
what a trainer does without it.  The source is the 8192^2 RGBA8 image of tools/time_decode_lod.py with its full chain (14 levels),
every level compressed at 6x6 -fastest and kept in device memory; the grid is that tool's first workload: 1920 x 1080 points under a
rotation by 30 degrees at one level-0 texel per point, lambda rising smoothly from 0 in the first row to 4 in the last (levels 0 to
4 are touched); planar fp16 with three channels; BILINEAR, CLAMP, MIP_LINEAR.  Three ways, in this process on the same stream,
alternating, after a warm-up pass of each; per way the best and the median of `reps` passes, timed with events on the stream:

  grad     the new call: grad_coords and grad_lod from an fp16 upstream gradient;
  forward  astcenc_amd_sample_lod_tensors_device on the same grid;
  torch    the route the call replaces: the five levels decoded to RGBA8 (astcenc_amd_decompress_image_device), made float,
           torch.nn.functional.grid_sample per level (bilinear, border padding, align_corners=False) with requires_grad on the
           coordinates, the levels blended in torch with weights max(0, 1 - |lambda - l|), scaled, and .backward() -- the whole
           backward pass of a trainer that has no compressed sampler; its forward half is part of it.

The new call's output is checked bit for bit against the numpy model (tests/sample_lod_grad_model.py) over the texels the
library's whole-image decode writes, on three rows of the grid; the largest difference to the torch way's gradients is printed and
is no pass criterion (torch's arithmetic is float32 and it has no right-hand rule at texel centres or at an integer lambda, so the
first and the last row are left out of that figure).
usage: time_decode_lod_grad.py [reps] [--size N] [--json out.json]"""
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import sample_lod_grad_model as G  # noqa: E402
import sample_lod_model as L  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
size = int(args[args.index("--size") + 1]) if "--size" in args else 8192
out_json = args[args.index("--json") + 1] if "--json" in args else None
B = 6
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
W, H, TOP = 1920, 1080, 4


def chain_dims(n):
    dims = []
    while True:
        dims.append(max(1, n >> len(dims)))
        if dims[-1] == 1:
            return dims


DIMS = chain_dims(size)
LEVELS = len(DIMS)
assert LEVELS > TOP


def rotated(w, h):
    """Normalised: one level-0 texel per point."""
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    jj, ii = np.meshgrid(np.arange(h) - (h - 1) / 2.0, np.arange(w) - (w - 1) / 2.0, indexing="ij")
    x = size / 2.0 + (c * ii - s * jj)
    y = size / 2.0 + (s * ii + c * jj)
    return (np.stack([x, y], axis=-1) / size).astype(np.float32)


assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()

# the streams, as tools/time_decode_lod.py makes them
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

err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
entries = [A.compressed_entry(s, (n, n), A.TYPE_U8) for s, n in zip(streams, DIMS)]
entry_arr = (A.ImageSetEntry * LEVELS)(*entries)
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
scale32 = [float(v) for v in fmt.scale]
sampler = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
scale_t = torch.tensor(scale32[:3], device="cuda").view(3, 1, 1)

coords = rotated(W, H)
lod = np.repeat((float(TOP) * np.arange(H) / (H - 1.0)).astype(np.float32)[:, None], W, axis=1)
upstream = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float16)
duv, dlod, dup = torch.from_numpy(coords).cuda(), torch.from_numpy(lod).cuda(), torch.from_numpy(upstream).cuda()
out = torch.zeros((3, H, W), dtype=torch.float16, device="cuda")
grad_coords, grad_lod = torch.zeros_like(duv), torch.zeros_like(dlod)
forward_grid = (A.LodGrid * 1)(A.lod_grid(0, LEVELS, 0, duv, dlod, out, type=A.TENSOR_F16))
grad_grid = (A.LodGradGrid * 1)(A.lod_grad_grid(0, LEVELS, 0, duv, dlod, dup, grad_coords, grad_lod, type=A.TENSOR_F16))
# (level TOP + 1 is read by the new call alone: the right derivative along lambda in the last row, where lambda is TOP itself)
scratch = [torch.zeros((DIMS[l], DIMS[l], 4), dtype=torch.uint8, device="cuda") for l in range(TOP + 2)]
torch_grads = {}


def decode_level(l):
    n = DIMS[l]
    e = lib.lib.astcenc_amd_decompress_image_device(ctx, C.c_void_p(streams[l].data_ptr()), streams[l].numel(), C.c_void_p(scratch[l].data_ptr()), n, n, 1,
                                                    A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), stream.cuda_stream)
    assert e == 0, e


def way_grad():
    e = lib.lib.astcenc_amd_sample_lod_grad_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(sampler), grad_grid, 1, stream.cuda_stream)
    assert e == 0, e


def way_forward():
    e = lib.lib.astcenc_amd_sample_lod_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(sampler), forward_grid, 1, stream.cuda_stream)
    assert e == 0, e


def way_torch():
    uv = duv.clone().requires_grad_(True)
    lam = dlod.clone().requires_grad_(True)
    g = (uv * 2.0 - 1.0).unsqueeze(0)                                      # align_corners=False: x = (g + 1) W / 2 = u W
    lc = lam.clamp(0.0, float(LEVELS - 1))
    total = None
    for l in range(TOP + 1):
        decode_level(l)
        img = scratch[l][..., :3].permute(2, 0, 1).unsqueeze(0).float()
        s = torch.nn.functional.grid_sample(img, g, mode="bilinear", padding_mode="border", align_corners=False)[0]
        term = (1.0 - (lc - float(l)).abs()).clamp(min=0.0).unsqueeze(0) * s
        total = term if total is None else total + term
    (total * scale_t).backward(dup.float())
    torch_grads["coords"], torch_grads["lod"] = uv.grad, lam.grad


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(t):
    t = sorted(t)
    return {"best_ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4)}


ways = {"grad": way_grad, "forward": way_forward, "torch": way_torch}
torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
for fn in ways.values():                                                   # warm-up of every way
    fn()
torch.cuda.synchronize()
t = {k: [] for k in ways}
for _ in range(reps):                                                      # alternating
    for k, fn in ways.items():
        t[k].append(timed_ms(fn))

# the model, on three rows, over what the library's whole-image decode writes
for l in range(TOP + 2):
    decode_level(l)
torch.cuda.synchronize()
whole = [scratch[l].cpu().numpy() for l in range(TOP + 2)] + [np.zeros((n, n, 4), dtype=np.uint8) for n in DIMS[TOP + 2:]]
rows_checked = sorted({0, H // 2, H - 1})
a = G.upstream(np.moveaxis(upstream[:, rows_checked], 0, -1), scale32)
want_gc, want_gl = G.grad(whole, L.S.BILINEAR, L.S.CLAMP, L.S.CLAMP, L.MIP_LINEAR, coords[rows_checked], lod[rows_checked], 0.0, a)
got_gc, got_gl = grad_coords[rows_checked].cpu().numpy(), grad_lod[rows_checked].cpu().numpy()
differences = int((got_gc.view(np.uint32) != want_gc.view(np.uint32)).sum() + (got_gl.view(np.uint32) != want_gl.view(np.uint32)).sum())

row = {"workload": "1920x1080 rotated by 30 degrees, lambda ramping 0..4", "points": W * H, "levels": LEVELS, "levels_touched": TOP + 1, "reps": reps,
       "model_points": len(rows_checked) * W, "model_differences": differences}
for k in ways:
    row[k] = dict(stats(t[k]), mpoints_per_s=round(W * H / min(t[k]) / 1e3, 1))
row["grad_over_forward_best"] = round(min(t["grad"]) / min(t["forward"]), 3)
row["grad_over_forward_median"] = round(sorted(t["grad"])[reps // 2] / sorted(t["forward"])[reps // 2], 3)
row["torch_over_grad_best"] = round(min(t["torch"]) / min(t["grad"]), 3)
row["torch_over_grad_median"] = round(sorted(t["torch"])[reps // 2] / sorted(t["grad"])[reps // 2], 3)
# (rows 0 and H - 1 have an integer lambda, where torch's |x| has the derivative 0 and this call the right derivative: left out)
row["max_abs_difference_to_torch_grad_coords"] = float((grad_coords - torch_grads["coords"])[1:-1].abs().max())
row["max_abs_grad_coords"] = float(grad_coords.abs().max())
row["max_abs_difference_to_torch_grad_lod"] = float((grad_lod - torch_grads["lod"])[1:-1].abs().max())
row["max_abs_grad_lod"] = float(grad_lod.abs().max())
print(json.dumps(row), flush=True)
lib.context_free(ctx)
summary = {"rows": [row], "model_exact": differences == 0}
print(json.dumps({"model_exact": summary["model_exact"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
