#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""A compressed cube map sampled by direction at a level of detail per point straight into a tensor
(astcenc_amd_sample_cube_tensors_device) against what a user does without that call: the six faces of every level the points need
decoded into float32 tensors with astcenc_amd_decompress_tensors_device, every face padded by one texel with its neighbours'
texels (a gather through index tensors made once, outside the timing), then direction -> face and face coordinates, the levels
and weights, four gathers per level, the bilinear sums, the blend, scale, shift and fp16 conversion in torch.  The source is a
cube of 512^2 faces with its full chain (10 levels), every level compressed at 6x6 -fastest and kept in device memory, one entry
per level; the output is planar fp16 with three channels; BILINEAR, MIP_LINEAR.  Workloads:

  1. a 1920 x 1080 grid of reflection vectors -- the rays of a pinhole camera reflected off a wavy surface -- with lambda rising
     smoothly from 0 in the first row to 4 in the last;
  2. a 1920 x 1080 grid of directions through an even lattice over face +Z alone with the same lambda, against
     astcenc_amd_sample_lod_tensors_device on layer 4 of the same chain at the same points under CLAMP: the same pipeline apart
     from the coordinate stage.

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does.  Before any timing the new call's output is
checked bit for bit against the numpy model (tests/sample_cube_model.py) over the texels the library's whole-image decode writes
for every level, on three rows of the grid, and the torch way's result must lie within two fp16 units in the last place of it
(its arithmetic is float32, the model's binary64: one rounding each way).  Level passes, batches and blocks decoded: counted on
the host by the library's own tile routine (the `blocks` mode of tests/harness/decode_cube_check.cpp, which this tool compiles
with g++); --blocks-only does nothing else and needs no GPU, --no-blocks leaves it out.
usage: time_decode_cube.py [reps] [--json out.json] [--blocks-only | --no-blocks]"""
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
B, FACE = 6, 512
DIMS = [FACE >> l for l in range(10)]
LEVELS = len(DIMS)
W, H = 1920, 1080
TMP = tempfile.mkdtemp()
HARNESS_EXE = os.path.join(TMP, "decode_cube_check")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def reflection_field():
    """The rays of a camera with a 90 degree horizontal field of view, turned by 30 degrees about y, reflected off a surface whose
    normal waves about the view axis."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(ii + 0.5) / W * 2.0 - 1.0, -((jj + 0.5) / H * 2.0 - 1.0) * H / W, -np.ones((H, W))], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    n = np.stack([0.35 * np.sin(ii / 97.0) + 0.2 * np.sin(jj / 41.0), 0.35 * np.cos(jj / 71.0), np.ones((H, W))], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    r = d - 2.0 * (d * n).sum(axis=-1, keepdims=True) * n
    c, s = np.cos(np.radians(30.0)), np.sin(np.radians(30.0))
    r = np.stack([c * r[..., 0] + s * r[..., 2], r[..., 1], -s * r[..., 0] + c * r[..., 2]], axis=-1)
    return r.astype(np.float32)


def one_face():
    """An even lattice over face +Z: the direction (x, -y, 1) has the face coordinates ((x + 1) / 2, (y + 1) / 2) s."""
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = (ii + 0.5) / W * 2.0 - 1.0, (jj + 0.5) / H * 2.0 - 1.0
    dirs = np.stack([x, -y, np.ones((H, W))], axis=-1).astype(np.float32)
    uv = np.stack([(dirs[..., 0].astype(np.float64) + 1.0) / 2.0, (1.0 - dirs[..., 1].astype(np.float64)) / 2.0], axis=-1).astype(np.float32)
    return dirs, uv


ramp = np.repeat((4.0 * np.arange(H) / (H - 1.0)).astype(np.float32)[:, None], W, axis=1)
face_dirs, face_uv = one_face()
workloads = (("1920x1080 reflection vectors, lambda ramping 0..4", reflection_field(), ramp, None),
             ("1920x1080 directions over face +Z, lambda ramping 0..4", face_dirs, ramp, face_uv))


def blocks_decoded(dirs, lod):
    if not os.path.exists(HARNESS_EXE):
        subprocess.run(["g++", "-std=c++17", "-O2", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"),
                        os.path.join(ROOT, "tests", "harness", "decode_cube_check.cpp"), "-o", HARNESS_EXE], check=True)
    dpath, lpath = os.path.join(TMP, "dirs.f32"), os.path.join(TMP, "lod.f32")
    dirs.astype(np.float32).tofile(dpath)
    lod.astype(np.float32).tofile(lpath)
    res = subprocess.run([HARNESS_EXE, "blocks", "1", "1", str(B), str(B), str(FACE), str(LEVELS), str(W), str(H), dpath, lpath], capture_output=True, text=True, check=True)
    f = res.stdout.split()
    n = {"tiles": int(f[1]), "passes": int(f[3]), "batches": int(f[5]), "decoded": int(f[7]), "points": int(f[9])}
    return dict(n, passes_per_tile=round(n["passes"] / n["tiles"], 3), batches_per_tile=round(n["batches"] / n["tiles"], 3),
                decoded_per_point=round(n["decoded"] / n["points"], 4))


if blocks_only:
    rows = []
    for name, dirs, lod, _ in workloads:
        row = {"workload": name, "blocks": blocks_decoded(dirs, lod)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)
    sys.exit(0)

import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402
import mip_cube_model as Q  # noqa: E402
import sample_cube_model as K  # noqa: E402
import tensor_model as M  # noqa: E402

assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()

# the streams: every level is six synthetic images of its size, compressed, back to back
streams = []
for l, n in enumerate(DIMS):
    data = np.concatenate([lib.compress(A.synthetic_image(n, n, seed=6 * l + f + 1), (B, B), A.PRE_FASTEST).reshape(-1) for f in range(6)])
    streams.append(torch.from_numpy(np.ascontiguousarray(data)).cuda())
err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
entries = [A.compressed_entry(s, (n, n, 6), A.TYPE_U8) for s, n in zip(streams, DIMS)]
entry_arr = (A.ImageSetEntry * LEVELS)(*entries)
fmt = A.tensor_format(A.TENSOR_F16, A.TENSOR_PLANAR, 3, [1.0 / (255.0 * s) for s in STD], [-m / s for m, s in zip(MEAN, STD)])
plain32 = A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 3)
scale32, bias32 = [float(v) for v in fmt.scale], [float(v) for v in fmt.bias]
cube_sampler = A.CubeSampler(A.SAMPLE_BILINEAR, A.MIP_LINEAR)
lod_sampler = A.LodSampler(A.SAMPLE_BILINEAR, A.ADDRESS_CLAMP, A.ADDRESS_CLAMP, A.MIP_LINEAR)
scale_t = torch.tensor(scale32[:3], device="cuda").view(3, 1)
bias_t = torch.tensor(bias32[:3], device="cuda").view(3, 1)
NEEDED = 5                                                                  # lambda in [0, 4]: levels 0 .. 4


def whole_level(l):
    n = DIMS[l]
    out = torch.zeros((6, n, n, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                                               # as whole_level of tools/time_decode_volume.py
    e = lib.decompress_tensors_device(ctx, entries, A.tensor_format(A.TENSOR_F32, A.TENSOR_INTERLEAVED, 4), [(l, (0, 0, 0), (n, n, 6), out)], stream=stream.cuda_stream)
    assert e == 0, e
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.uint8)


# the torch way's index tensors, made once: padded texel (iy + 1, ix + 1) of face f is the texel tap (ix, iy) reads
pad_index = []
for l in range(NEEDED):
    face, ys, xs = Q.unfold(DIMS[l])
    cut = slice(Q.PAD - 1, Q.PAD + DIMS[l] + 1)
    pad_index.append(tuple(torch.from_numpy(np.ascontiguousarray(a[:, cut, cut])).cuda() for a in (face, ys, xs)))
faces32 = [torch.empty((3, 6, DIMS[l], DIMS[l]), dtype=torch.float32, device="cuda") for l in range(NEEDED)]
SC = torch.tensor([[0, 0, -1], [0, 0, 1], [1, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], dtype=torch.float32, device="cuda")
TC = torch.tensor([[0, -1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, -1, 0]], dtype=torch.float32, device="cuda")


def torch_way(dirs, lod, out):
    e = lib.decompress_tensors_device(ctx, entries, plain32, [(l, (0, 0, 0), (DIMS[l], DIMS[l], 6), faces32[l]) for l in range(NEEDED)], stream=stream.cuda_stream)
    assert e == 0, e
    d = dirs.reshape(-1, 3)
    a = d.abs()
    axis = torch.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, torch.where(a[:, 1] >= a[:, 2], 1, 2))
    major = d.gather(1, axis[:, None]).squeeze(1)
    f = 2 * axis + (major < 0).long()
    ma = major.abs()
    p, q = (d * SC[f]).sum(1) / ma, (d * TC[f]).sum(1) / ma
    lc = lod.reshape(-1).clamp(0.0, float(LEVELS - 1))
    l0 = lc.floor()
    g = lc - l0
    l0 = l0.long()
    l1 = torch.where(g != 0, l0 + 1, torch.full_like(l0, -1))
    s0 = torch.zeros((3, d.shape[0]), dtype=torch.float32, device="cuda")
    s1 = torch.zeros((3, d.shape[0]), dtype=torch.float32, device="cuda")
    for l in range(NEEDED):
        fi, yi, xi = pad_index[l]
        padded = faces32[l][:, fi, yi, xi]                                  # [3, 6, s + 2, s + 2]
        first, second = (l0 == l).nonzero().squeeze(1), (l1 == l).nonzero().squeeze(1)
        idx = torch.cat([first, second])
        h = DIMS[l] * 0.5
        tx, ty = p[idx] * h + h - 0.5, q[idx] * h + h - 0.5
        ix, iy = tx.floor(), ty.floor()
        fx, fy = (tx - ix)[None], (ty - iy)[None]
        ix, iy, ff = ix.long() + 1, iy.long() + 1, f[idx]
        # (a second tap of weight zero may lie one past the padding: clamped, its weight is zero)
        ix1, iy1 = (ix + 1).clamp(max=DIMS[l] + 1), (iy + 1).clamp(max=DIMS[l] + 1)
        r0 = (1.0 - fx) * padded[:, ff, iy, ix] + fx * padded[:, ff, iy, ix1]
        r1 = (1.0 - fx) * padded[:, ff, iy1, ix] + fx * padded[:, ff, iy1, ix1]
        part = (1.0 - fy) * r0 + fy * r1
        s0[:, first] = part[:, :first.numel()]
        s1[:, second] = part[:, first.numel():]
    s = torch.where((l1 >= 0)[None], (1.0 - g)[None] * s0 + g[None] * s1, s0)
    out.copy_((s * scale_t + bias_t).half().view(3, H, W))


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


whole = [whole_level(l) for l in range(LEVELS)]
rows = []
for name, dirs, lod, uv in workloads:
    ddirs, dlod = torch.from_numpy(dirs).cuda(), torch.from_numpy(lod).cuda()
    out = {k: torch.zeros((3, H, W), dtype=torch.float16, device="cuda") for k in ("cube", "torch", "lod")}
    prepared = (A.CubeGrid * 1)(A.cube_grid(0, LEVELS, 0, ddirs, dlod, out["cube"], type=A.TENSOR_F16))

    def cube_call(prepared=prepared):
        e = lib.lib.astcenc_amd_sample_cube_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(cube_sampler), prepared, 1, stream.cuda_stream)
        assert e == 0, e

    ways = {"cube": cube_call, "decode_faces_and_torch": lambda: torch_way(ddirs, dlod, out["torch"])}
    if uv is not None:
        duv = torch.from_numpy(uv).cuda()
        lod_prepared = (A.LodGrid * 1)(A.lod_grid(0, LEVELS, 4, duv, dlod, out["lod"], type=A.TENSOR_F16))

        def lod_call(lod_prepared=lod_prepared):
            e = lib.lib.astcenc_amd_sample_lod_tensors_device(ctx, entry_arr, LEVELS, C.byref(fmt), C.byref(lod_sampler), lod_prepared, 1, stream.cuda_stream)
            assert e == 0, e
        ways["lod_call_on_layer_4"] = lod_call
    torch.cuda.synchronize()                                               # the fills above are on torch's default stream, which the calls' own stream does not wait for
    for fn in ways.values():                                               # warm-up of every way, and the results the check reads
        fn()
    torch.cuda.synchronize()
    # ---- agreement first ----
    rows_checked = sorted({0, H // 2, H - 1})
    bits = K.convert(whole, 0, K.BILINEAR, K.MIP_LINEAR, dirs[rows_checked], lod[rows_checked], 0.0, M.F16, 3, scale32, bias32)[0]
    got = out["cube"][:, rows_checked].view(torch.int16).cpu().numpy().view(np.uint16)
    model_differences = int((got != bits.transpose(2, 0, 1)).sum())
    diff = float((out["cube"].float() - out["torch"].float()).abs().max())
    # (outputs lie within (-4, 4): an fp16 unit in the last place is at most 2^-9 there)
    agree = model_differences == 0 and diff <= 2.0 ** -8
    row = {"workload": name, "points": H * W, "levels": LEVELS, "reps": reps, "model_points": len(rows_checked) * W, "model_differences": model_differences,
           "max_abs_difference_to_torch_way": diff, "agree": agree}
    if uv is not None:
        row["bytes_differing_from_lod_call"] = int((out["cube"].view(torch.int16) != out["lod"].view(torch.int16)).sum())
    # ---- then the times ----
    t = {k: [] for k in ways}
    for _ in range(reps):                                                  # alternating
        for k, fn in ways.items():
            t[k].append(timed_ms(fn))
    for k in ways:
        row[k] = dict(stats(t[k]), mpoints_per_s=round(H * W / min(t[k]) / 1e3, 1))
        if k != "cube":
            row[k + "_over_cube_best"] = round(min(t[k]) / min(t["cube"]), 3)
            row[k + "_over_cube_median"] = round(sorted(t[k])[reps // 2] / sorted(t["cube"])[reps // 2], 3)
    if not no_blocks:
        row["blocks"] = blocks_decoded(dirs, lod)
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"rows": rows, "agree": all(r["agree"] for r in rows)}
print(json.dumps({"agree": summary["agree"]}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
sys.exit(0 if summary["agree"] else 1)
