#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The gradients of the volume sampler (astcenc_amd_sample_volume_grad_device) timed against the forward call and against what a
trainer does without it.  The source is the 256^3 RGBA8 volume of tools/time_decode_volume.py with its full chain (9 levels), every
level kept compressed in device memory, once at 6x6 over slices and once at 4x4x4; the grid is that tool's first workload: a
1920 x 1080 grid of ray-march samples on a wavy surface that cuts the volume at a slant, lambda rising smoothly from 0 in the
first row to 4 in the last (levels 0 to 4 are touched); planar fp16 with three channels; BILINEAR on all three axes, CLAMP,
MIP_LINEAR.  Three ways per footprint, in this process on the same stream, alternating, after a warm-up pass of each; per way the
best and the median of `reps` passes, timed with events on the stream:

  grad     the new call: grad_coords and grad_lod from an fp16 upstream gradient;
  forward  astcenc_amd_sample_volume_tensors_device on the same grid;
  torch    the route the call replaces: the five levels decoded to float32 [C, D, H, W] (astcenc_amd_decompress_tensors_device),
           torch.nn.functional.grid_sample per level (5D, trilinear, border padding, align_corners=False) with requires_grad on the
           coordinates, the levels blended in torch with weights max(0, 1 - |lambda - l|), scaled, and .backward() -- the whole
           backward pass of a trainer that has no compressed sampler; its forward half is part of it.

Before any timing the new call's output must equal, bit for bit, the numpy model (tests/sample_volume_grad_model.py) over the
texels the library's whole-level decode writes, on three rows of the grid: the tool exits with 1 otherwise.  The largest
difference to the torch way's gradients is printed and is no pass criterion (torch's arithmetic is float32 and it has no
right-hand rule at texel centres or at an integer lambda, so the first and the last row are left out of that figure).
usage: time_decode_volume_grad.py [reps] [--json out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import sample_lod_model as L  # noqa: E402
import sample_model as S  # noqa: E402
import sample_volume_grad_model as G  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
out_json = args[args.index("--json") + 1] if "--json" in args else None
SIDE = 256
DIMS = [SIDE >> l for l in range(9)]
LEVELS = len(DIMS)
W, H, TOP = 1920, 1080, 4
SLAB = 16
FOOTPRINTS = [(6, 6, 1), (4, 4, 4)]
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def ray_march_field():
    """tools/time_decode_volume.py's: one sample per pixel, (u, v) sweep a little more than the volume, w follows a slanted, wavy
    surface through it."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u = (ii + 0.5) / W * 1.1 - 0.05
    v = (jj + 0.5) / H * 1.1 - 0.05
    w = 0.15 + 0.6 * (ii + 0.5) / W + 0.1 * np.sin(ii / 97.0) * np.cos(jj / 71.0)
    return np.stack([u, v, w], axis=-1).astype(np.float32)


def name_of(footprint):
    return "x".join(str(v) for v in (footprint if footprint[2] > 1 else footprint[:2]))


assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
plain32 = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 3)
scale32 = [float(v) for v in fmt.scale]
sampler = A.VolumeSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
scale_t = torch.tensor(scale32[:3], device="cuda").view(3, 1, 1)

coords = ray_march_field()
lod = np.repeat((float(TOP) * np.arange(H) / (H - 1.0)).astype(np.float32)[:, None], W, axis=1)
upstream = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float16)
dcoords, dlod, dup = torch.from_numpy(coords).cuda(), torch.from_numpy(lod).cuda(), torch.from_numpy(upstream).cuda()
out = torch.zeros((3, H, W), dtype=torch.float16, device="cuda")
grad_coords, grad_lod = torch.zeros_like(dcoords), torch.zeros_like(dlod)
forward_grid = (A.VolumeGrid * 1)(A.volume_grid(0, LEVELS, dcoords, dlod, out, type=A.TENSOR_F16))
grad_grid = (A.VolumeGradGrid * 1)(A.volume_grad_grid(0, LEVELS, dcoords, dlod, dup, grad_coords, grad_lod, type=A.TENSOR_F16))
vols32 = [torch.empty((3, DIMS[l], DIMS[l], DIMS[l]), dtype=torch.float32, device="cuda") for l in range(TOP + 1)]


def level_stream(footprint, l):
    """The stream of level l: a slab of min(depth, SLAB) slices compressed, repeated along z (tools/time_decode_volume.py)."""
    n = DIMS[l]
    slab = min(n, SLAB)
    img = np.stack([A.synthetic_image(n, n, seed=31 * l + z + 1) for z in range(slab)])
    if footprint[2] == 1:
        data = np.concatenate([lib.compress(img[z], footprint[:2], A.PRE_FASTEST).reshape(-1) for z in range(slab)])
    else:
        data = lib.compress(img, footprint, A.PRE_FASTEST).reshape(-1)
        assert slab % footprint[2] == 0 or slab == n
    return torch.from_numpy(np.ascontiguousarray(np.tile(data, n // slab))).cuda()


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


rows = []
for footprint in FOOTPRINTS:
    streams = [level_stream(footprint, l) for l in range(LEVELS)]
    err, cfg = lib.config_init(A.PRF_LDR, footprint[0], footprint[1], footprint[2], A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    entries = [A.compressed_entry(s, (n, n, n), A.TYPE_U8) for s, n in zip(streams, DIMS)]
    entry_arr = (A.ImageSetEntry * LEVELS)(*entries)
    torch_grads = {}

    def whole_level(l):
        n = DIMS[l]
        held = torch.zeros((n, n, n, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e = lib.decompress_tensors_device(ctx, entries, A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4), [(l, (0, 0, 0), (n, n, n), held)], stream=stream.cuda_stream)
        assert e == 0, e
        torch.cuda.synchronize()
        return held.cpu().numpy().astype(np.uint8)

    def way_grad():
        e = lib.lib.astcenc_amd_sample_volume_grad_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(sampler), grad_grid, 1, stream.cuda_stream)
        assert e == 0, e

    def way_forward():
        e = lib.lib.astcenc_amd_sample_volume_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(sampler), forward_grid, 1, stream.cuda_stream)
        assert e == 0, e

    def way_torch():
        e = lib.decompress_tensors_device(ctx, entries, plain32, [(l, (0, 0, 0), (DIMS[l],) * 3, vols32[l]) for l in range(TOP + 1)], stream=stream.cuda_stream)
        assert e == 0, e
        uvw = dcoords.clone().requires_grad_(True)
        lam = dlod.clone().requires_grad_(True)
        g = (uvw * 2.0 - 1.0).view(1, 1, H, W, 3)                               # align_corners=False: x = (g + 1) W / 2 = u W
        lc = lam.clamp(0.0, float(LEVELS - 1))
        total = None
        for l in range(TOP + 1):
            s = torch.nn.functional.grid_sample(vols32[l][None], g, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0]
            term = (1.0 - (lc - float(l)).abs()).clamp(min=0.0).unsqueeze(0) * s
            total = term if total is None else total + term
        (total * scale_t).backward(dup.float())
        torch_grads["coords"], torch_grads["lod"] = uvw.grad, lam.grad

    ways = {"grad": way_grad, "forward": way_forward, "torch": way_torch}
    torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
    for fn in ways.values():                                               # warm-up of every way, and the results the check reads
        fn()
    torch.cuda.synchronize()

    # ---- bit equality with the model first, on three rows, over what the library's whole-level decode writes ----
    # (level TOP + 1 is read by the new call alone: the right derivative along lambda in the last row, where lambda is TOP itself)
    whole = [whole_level(l) for l in range(TOP + 2)] + [np.zeros((n, n, n, 4), dtype=np.uint8) for n in DIMS[TOP + 2:]]
    rows_checked = sorted({0, H // 2, H - 1})
    a = G.upstream(np.moveaxis(upstream[:, rows_checked], 0, -1), scale32)
    want_gc, want_gl = G.grad(whole, S.BILINEAR, (S.CLAMP,) * 3, L.MIP_LINEAR, coords[rows_checked], lod[rows_checked], 0.0, a)
    got_gc, got_gl = grad_coords[rows_checked].cpu().numpy(), grad_lod[rows_checked].cpu().numpy()
    differences = int((got_gc.view(np.uint32) != want_gc.view(np.uint32)).sum() + (got_gl.view(np.uint32) != want_gl.view(np.uint32)).sum())
    del whole
    if differences:
        print(json.dumps({"footprint": name_of(footprint), "model_points": len(rows_checked) * W, "model_differences": differences}))
        sys.exit(1)

    # ---- then the times ----
    t = {k: [] for k in ways}
    for _ in range(reps):                                                  # alternating
        for k, fn in ways.items():
            t[k].append(timed_ms(fn))
    row = {"footprint": name_of(footprint), "workload": "1920x1080 ray-march samples, lambda ramping 0..4", "points": W * H, "levels": LEVELS, "levels_touched": TOP + 1,
           "reps": reps, "model_points": len(rows_checked) * W, "model_differences": differences}
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
    row["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated())
    print(json.dumps(row), flush=True)
    rows.append(row)
    lib.context_free(ctx)
summary = {"rows": rows, "model_exact": all(r["model_differences"] == 0 for r in rows)}
print(json.dumps({"model_exact": summary["model_exact"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
