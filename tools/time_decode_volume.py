#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""A compressed volume sampled at (u, v, w) at a level of detail per point straight into a tensor
(astcenc_amd_sample_volume_tensors_device) against what a user does without that call: the levels the points need decoded into
float32 [C, D, H, W] tensors with astcenc_amd_decompress_tensors_device, then torch.nn.functional.grid_sample (5D, trilinear,
align_corners=False, border padding: CLAMP) per level, the blend, scale, shift and fp16 conversion in torch.  The source is a
256^3 RGBA8 volume with its full chain (9 levels), every level kept compressed in device memory, one entry per level, once at
6x6 over slices and once at 4x4x4 (a level's stream is a compressed slab of up to 16 slices of synthetic images repeated along z:
the mix of block modes is the compressor's, the content repeats); the output is planar fp16 with three channels; BILINEAR on all
three axes, MIP_LINEAR, CLAMP.  Workloads, per footprint:

  1. a 1920 x 1080 grid of ray-march samples -- one sample per pixel on a wavy surface that cuts the volume at a slant -- with
     lambda rising smoothly from 0 in the first row to 4 in the last;
  2. a [1, 65535, 3] list of samples anywhere in the volume with lambda anywhere in [0, 4];
  3. (6x6 only) the 1920 x 1080 grid with every sample on the centre of slice 100 of level 0, a chain of that one level: one z
     tap, against astcenc_amd_sample_lod_tensors_device on slice 100 at the same (u, v): the same four taps a point, bit for bit.

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best, the median and the
worst of `reps` passes, timed with events on the stream around everything the way does.  Before any timing the new call's output
is checked bit for bit against the numpy model (tests/sample_volume_model.py, point by point) over the texels the library's
whole-level decode writes, on 256 points spread over the grid, and the torch way's result must lie within two fp16 units in the
last place of it (its arithmetic is float32, the model's binary64).  Level passes, batches and blocks decoded: counted on the host
by the library's own tile routine (the `blocks` mode of tests/harness/decode_volume_check.cpp, which this tool compiles with
g++); --blocks-only does nothing else and needs no GPU, --no-blocks leaves it out.
usage: time_decode_volume.py [reps] [--json out.json] [--blocks-only | --no-blocks]"""
import ctypes as C
import json
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
out_json = args[args.index("--json") + 1] if "--json" in args else None
blocks_only, no_blocks = "--blocks-only" in args, "--no-blocks" in args
SIDE = 256
DIMS = [SIDE >> l for l in range(9)]
LEVELS = len(DIMS)
W, H, N = 1920, 1080, 65535
SLICE = 100
SLAB = 16
FOOTPRINTS = [(6, 6, 1), (4, 4, 4)]
TMP = tempfile.mkdtemp()
HARNESS_EXE = os.path.join(TMP, "decode_volume_check")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def ray_march_field():
    """One sample per pixel: (u, v) sweep a little more than the volume, w follows a slanted, wavy surface through it."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u = (ii + 0.5) / W * 1.1 - 0.05
    v = (jj + 0.5) / H * 1.1 - 0.05
    w = 0.15 + 0.6 * (ii + 0.5) / W + 0.1 * np.sin(ii / 97.0) * np.cos(jj / 71.0)
    return np.stack([u, v, w], axis=-1).astype(np.float32)


def slice_centres():
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    uv = np.stack([(ii + 0.5) / W, (jj + 0.5) / H], axis=-1).astype(np.float32)
    w = np.full((H, W, 1), (SLICE + 0.5) / SIDE, dtype=np.float32)
    return np.concatenate([uv, w], axis=-1), uv


rng = np.random.default_rng(5)
ramp = np.repeat((4.0 * np.arange(H) / (H - 1.0)).astype(np.float32)[:, None], W, axis=1)
centre_uvw, centre_uv = slice_centres()
# (name, coords, lod, levels of the chain, (u, v) of the lod call or None)
workloads = (("1920x1080 ray-march samples, lambda ramping 0..4", ray_march_field(), ramp, LEVELS, None),
             ("[1, 65535, 3] samples anywhere, lambda anywhere in 0..4", rng.uniform(0.0, 1.0, size=(1, N, 3)).astype(np.float32),
              rng.uniform(0.0, 4.0, size=(1, N)).astype(np.float32), LEVELS, None),
             ("1920x1080 samples on the centre of slice 100, one level", centre_uvw, None, 1, centre_uv))


def blocks_decoded(footprint, coords, lod, levels):
    if not os.path.exists(HARNESS_EXE):
        subprocess.run(["g++", "-std=c++17", "-O2", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"),
                        os.path.join(ROOT, "tests", "harness", "decode_volume_check.cpp"), "-o", HARNESS_EXE], check=True)
    cpath, lpath = os.path.join(TMP, "coords.f32"), os.path.join(TMP, "lod.f32")
    coords.astype(np.float32).tofile(cpath)
    if lod is not None:
        lod.astype(np.float32).tofile(lpath)
    oy, ox = coords.shape[:2]
    res = subprocess.run([HARNESS_EXE, "blocks"] + [str(v) for v in footprint] + ["1", "1", str(SIDE), str(SIDE), str(SIDE), str(levels), str(ox), str(oy), cpath,
                                                                                   lpath if lod is not None else "-"], capture_output=True, text=True, check=True)
    f = res.stdout.split()
    n = {"tiles": int(f[1]), "passes": int(f[3]), "batches": int(f[5]), "decoded": int(f[7]), "points": int(f[9])}
    return dict(n, passes_per_tile=round(n["passes"] / n["tiles"], 3), batches_per_tile=round(n["batches"] / n["tiles"], 3),
                decoded_per_point=round(n["decoded"] / n["points"], 4))


def name_of(footprint):
    return "x".join(str(v) for v in (footprint if footprint[2] > 1 else footprint[:2]))


if blocks_only:
    rows = []
    for footprint in FOOTPRINTS:
        for name, coords, lod, levels, uv in workloads:
            if uv is not None and footprint[2] > 1:
                continue
            row = {"footprint": name_of(footprint), "workload": name, "blocks": blocks_decoded(footprint, coords, lod, levels)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    sys.exit(0)

import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import sample_model as S  # noqa: E402
import sample_lod_model as L  # noqa: E402
import sample_volume_model as K  # noqa: E402
import tensor_model as M  # noqa: E402

assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
plain32 = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 3)
scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
volume_sampler = A.VolumeSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
lod_sampler = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
scale_t = torch.tensor(scale32[:3], device="cuda").view(3, 1)
bias_t = torch.tensor(bias32[:3], device="cuda").view(3, 1)
NEEDED = 5                                                                  # lambda in [0, 4]: levels 0 .. 4


def level_stream(footprint, l):
    """The stream of level l: a slab of min(depth, SLAB) slices compressed, repeated along z."""
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
    return {"best_ms": round(t[0], 4), "median_ms": round(t[len(t) // 2], 4), "worst_ms": round(t[-1], 4)}


rows = []
for footprint in FOOTPRINTS:
    streams = [level_stream(footprint, l) for l in range(LEVELS)]
    err, cfg = lib.config_init(A.PRF_LDR, footprint[0], footprint[1], footprint[2], A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    entries = [A.compressed_entry(s, (n, n, n), A.TYPE_U8) for s, n in zip(streams, DIMS)]
    entry_arr = (A.ImageSetEntry * LEVELS)(*entries)
    vols32 = [torch.empty((3, DIMS[l], DIMS[l], DIMS[l]), dtype=torch.float32, device="cuda") for l in range(NEEDED)]

    def whole_level(l):
        n = DIMS[l]
        out = torch.zeros((n, n, n, 4), dtype=torch.float32, device="cuda")
        # (the fill is on torch's default stream, handle 0, which as hip_stream means the context's own stream; the wrapper's
        # resolver, A.torch_stream, would synchronise for handle 0 as well -- this decode feeds the model, so it is said here too)
        torch.cuda.synchronize()
        e = lib.decompress_tensors_device(ctx, entries, A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4), [(l, (0, 0, 0), (n, n, n), out)], stream=stream.cuda_stream)
        assert e == 0, e
        torch.cuda.synchronize()
        return out.cpu().numpy().astype(np.uint8)

    whole = [whole_level(l) for l in range(LEVELS)]

    def torch_way(coords, lod, levels, out):
        need = min(NEEDED, levels)
        e = lib.decompress_tensors_device(ctx, entries, plain32, [(l, (0, 0, 0), (DIMS[l],) * 3, vols32[l]) for l in range(need)], stream=stream.cuda_stream)
        assert e == 0, e
        oy, ox = coords.shape[:2]
        grid = (coords * 2.0 - 1.0).view(1, 1, oy, ox, 3)
        lc = (lod if lod is not None else torch.zeros((oy, ox), device="cuda")).clamp(0.0, float(levels - 1))
        l0 = lc.floor()
        g = lc - l0
        l1 = torch.where(g != 0, l0 + 1, torch.full_like(l0, -1))
        s0 = torch.zeros((3, oy, ox), dtype=torch.float32, device="cuda")
        s1 = torch.zeros((3, oy, ox), dtype=torch.float32, device="cuda")
        for l in range(need):
            s = torch.nn.functional.grid_sample(vols32[l][None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0]
            s0 = torch.where((l0 == l)[None], s, s0)
            s1 = torch.where((l1 == l)[None], s, s1)
        s = torch.where((l1 >= 0)[None], (1.0 - g)[None] * s0 + g[None] * s1, s0)
        out.copy_((s * scale_t.view(3, 1, 1) + bias_t.view(3, 1, 1)).half())

    for name, coords, lod, levels, uv in workloads:
        if uv is not None and footprint[2] > 1:
            continue
        oy, ox = coords.shape[:2]
        dcoords = torch.from_numpy(coords).cuda()
        dlod = torch.from_numpy(lod).cuda() if lod is not None else None
        out = {k: torch.zeros((3, oy, ox), dtype=torch.float16, device="cuda") for k in ("volume", "torch", "lod")}
        prepared = (A.VolumeGrid * 1)(A.volume_grid(0, levels, dcoords, dlod, out["volume"], type=A.TENSOR_F16))

        def volume_call(prepared=prepared):
            e = lib.lib.astcenc_amd_sample_volume_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(volume_sampler), prepared, 1, stream.cuda_stream)
            assert e == 0, e

        ways = {"volume": volume_call, "decode_levels_and_grid_sample": lambda: torch_way(dcoords, dlod, levels, out["torch"])}
        if uv is not None:
            duv = torch.from_numpy(uv).cuda()
            lod_prepared = (A.LodGrid * 1)(A.lod_grid(0, levels, SLICE, duv, None, out["lod"], type=A.TENSOR_F16))

            def lod_call(lod_prepared=lod_prepared):
                e = lib.lib.astcenc_amd_sample_lod_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(lod_sampler), lod_prepared, 1, stream.cuda_stream)
                assert e == 0, e
            ways["lod_call_on_slice_100"] = lod_call
        torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
        for fn in ways.values():                                           # warm-up of every way, and the results the check reads
            fn()
        torch.cuda.synchronize()
        # ---- agreement first ----
        pick = np.random.default_rng(9).permutation(oy * ox)[:256]
        pj, pi = pick // ox, pick % ox
        got = out["volume"].view(torch.int16).cpu().numpy().view(np.uint16)[:, pj, pi]
        model_differences = 0
        for k, (j, i) in enumerate(zip(pj, pi)):
            s = K.sample_point(whole[:levels], S.BILINEAR, (S.CLAMP,) * 3, L.MIP_LINEAR, coords[j, i, 0], coords[j, i, 1], coords[j, i, 2], None if lod is None else lod[j, i], 0.0)
            bits = M.convert(s[None, None, None], M.F16, 3, scale32, bias32).reshape(3)
            model_differences += int((got[:, k] != bits).sum())
        diff = float((out["volume"].float() - out["torch"].float()).abs().max())
        # (outputs lie within (-4, 4): an fp16 unit in the last place is at most 2^-9 there)
        agree = model_differences == 0 and diff <= 2.0 ** -8
        row = {"footprint": name_of(footprint), "workload": name, "points": oy * ox, "levels": levels, "reps": reps, "model_points": len(pick),
               "model_differences": model_differences, "max_abs_difference_to_torch_way": diff, "agree": agree}
        if uv is not None:
            row["bytes_differing_from_lod_call"] = int((out["volume"].view(torch.int16) != out["lod"].view(torch.int16)).sum())
            row["agree"] = agree = agree and row["bytes_differing_from_lod_call"] == 0
        # ---- then the times ----
        t = {k: [] for k in ways}
        for _ in range(reps):                                              # alternating
            for k, fn in ways.items():
                t[k].append(timed_ms(fn))
        for k in ways:
            row[k] = dict(stats(t[k]), mpoints_per_s=round(oy * ox / min(t[k]) / 1e3, 1))
            if k != "volume":
                row[k + "_over_volume_best"] = round(min(t[k]) / min(t["volume"]), 3)
                row[k + "_over_volume_median"] = round(sorted(t[k])[reps // 2] / sorted(t["volume"])[reps // 2], 3)
        if not no_blocks:
            row["blocks"] = blocks_decoded(footprint, coords, lod, levels)
        print(json.dumps(row), flush=True)
        rows.append(row)
    lib.context_free(ctx)
summary = {"rows": rows, "agree": all(r["agree"] for r in rows)}
print(json.dumps({"agree": summary["agree"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
sys.exit(0 if summary["agree"] else 1)
