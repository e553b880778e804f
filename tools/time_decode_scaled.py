#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Random resized crops of a compressed image straight into a training batch (astcenc_amd_decompress_scaled_tensors_device)
against what a user does without that call: astcenc_amd_decompress_tensors_device into one tensor per sample at the window's own
size (normalised, mirrored), then one torch.nn.functional.interpolate per sample into the batch tensor.  The source is the
8192^2 RGBA8 image of tools/time_decode_tensors.py, compressed at 6x6 -fastest and kept in device memory.  Three workloads:

  1. 256 random resized crops -> [256, 3, 224, 224] fp16 planar, every other sample mirrored: each window has 8 .. 100 % of the
     area of a 500 x 375 rectangle placed at random, aspect ratio 3/4 .. 4/3 (log-uniform), fixed seed;
  2. 1024 such crops -> 64^2;
  3. the 256 ratio-1 windows of 224^2 of tools/time_decode_tensors.py: here the third way is the tensors call alone, and the
     difference is the price of the resampling machinery.

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does (every buffer is allocated once, outside the timed
window).  The new call's output is checked bit for bit against the numpy model (tests/scaled_model.py) on a subsample of the
samples; the largest absolute difference to the torch chain is printed and is no pass criterion: torch's float32 weights are
another, inexact definition.  Blocks decoded per block covered: the tiles of a region decode the blocks at their seams more than
once; counted on the host by the library's own tiling code (csrc/decode_scaled.h, through the `blocks` mode of
tests/harness/decode_scaled_check.cpp, which this tool compiles with g++).
usage: time_decode_scaled.py [reps] [--size N] [--json out.json]"""
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
import scaled_model as S  # noqa: E402
import tensor_model as M  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
size = int(args[args.index("--size") + 1]) if "--size" in args else 8192
out_json = args[args.index("--json") + 1] if "--json" in args else None
B = 6
# (host code of the library's tile arithmetic, compiled as plain sequential C++: counts blocks, runs nothing on the device)
HARNESS_EXE = os.path.join(tempfile.mkdtemp(), "decode_scaled_check")
subprocess.run(["g++", "-std=c++17", "-O1", "-DASTC_WAVE_EMU=1", "-ffp-contract=off", "-I", os.path.join(ROOT, "astc-encoder_amd", "csrc"),
                os.path.join(ROOT, "tests", "harness", "decode_scaled_check.cpp"), "-o", HARNESS_EXE], check=True)
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


def blocks_decoded_and_covered(filt, windows, out):
    """By the library's own tiling (csrc/decode_scaled.h): the `blocks` mode of tests/harness/decode_scaled_check.cpp sums
    decode_scaled_tile_blocks -- the count decode_scaled_tile returns -- over the tiles decode_scaled_build makes of each window."""
    text = "".join("%d %d %d %d\n" % w for w in windows)
    res = subprocess.run([HARNESS_EXE, "blocks", str(filt), str(B), str(B), "0", str(out), str(out)], input=text, capture_output=True, text=True, check=True)
    fields = res.stdout.split()
    return int(fields[1]), int(fields[3])


def scaled(prepared, count, filt):
    e = lib.lib.astcenc_amd_decompress_scaled_tensors_device(ctx, C.byref(entry), 1, C.byref(fmt), filt, prepared, count, stream.cuda_stream)
    assert e == 0, e


def tensors(prepared, count):
    e = lib.lib.astcenc_amd_decompress_tensors_device(ctx, C.byref(entry), 1, C.byref(fmt), prepared, count, stream.cuda_stream)
    assert e == 0, e


def tensors_then_interpolate(prepared, count, per_sample, out):
    tensors(prepared, count)
    edge = out.shape[-1]
    for i in range(count):
        out[i] = torch.nn.functional.interpolate(per_sample[i][None], size=(edge, edge), mode="bilinear", align_corners=False, antialias=False)[0]


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


def check_against_model(windows, out, filt, picks):
    """Samples `picks` of `out` against the model of the regions call's texels; returns the number of differing elements."""
    bad = 0
    for i in picks:
        x, y, sw, sh = windows[i]
        rgba = torch.zeros((sh, sw, 4), dtype=torch.uint8, device="cuda")
        assert lib.decompress_regions_device(ctx, [entry], [(0, (x, y, 0), (sw, sh, 1), rgba)]) == 0
        torch.cuda.synchronize()
        edge = out.shape[-1]
        want = S.tensor(rgba.cpu().numpy(), filt, edge, edge, M.F16, M.PLANAR, 3, scale32, bias32, M.FLIP_X if i % 2 else 0)
        bad += int((out[i].view(torch.int16).cpu().numpy().view(np.uint16) != want).sum())
    return bad


def random_resized_windows(rng, count):
    out = []
    while len(out) < count:
        rx, ry = int(rng.integers(0, size - 500 + 1)), int(rng.integers(0, size - 375 + 1))
        area = 500 * 375 * float(rng.uniform(0.08, 1.0))
        ratio = math.exp(float(rng.uniform(math.log(3 / 4), math.log(4 / 3))))
        sw, sh = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
        if 1 <= sw <= 500 and 1 <= sh <= 375:
            out.append((rx + int(rng.integers(0, 500 - sw + 1)), ry + int(rng.integers(0, 375 - sh + 1)), sw, sh))
    return out


rows = []
rng = np.random.default_rng(1)
workloads = (("256 random resized crops -> 224^2", 256, 224, True), ("1024 random resized crops -> 64^2", 1024, 64, True), ("256 ratio-1 windows of 224^2", 256, 224, False))
for name, count, edge, resized in workloads:
    if resized:
        windows = random_resized_windows(rng, count)
    else:
        windows = [(int(rng.integers(0, size - edge + 1)), int(rng.integers(0, size - edge + 1)), edge, edge) for _ in range(count)]
    out = {f: torch.zeros((count, 3, edge, edge), dtype=torch.float16, device="cuda") for f in ("bilinear", "box", "chain")}
    per_sample = [torch.zeros((3, sh, sw), dtype=torch.float16, device="cuda") for (_, _, sw, sh) in windows]
    prep = {f: (A.ScaledRegion * count)(*[A.scaled_region(0, (x, y, 0), (sw, sh), out[f][i], flip_x=i % 2 == 1) for i, (x, y, sw, sh) in enumerate(windows)])
            for f in ("bilinear", "box")}
    # the chain's first step: each window at its own size, mirrored there (mirroring commutes with both filters); ratio 1: straight into the batch
    prep_t = (A.TensorRegion * count)(*[A.tensor_region(0, (x, y, 0), (sw, sh, 1), per_sample[i] if resized else out["chain"][i], flip_x=i % 2 == 1)
                                        for i, (x, y, sw, sh) in enumerate(windows)])
    third = (lambda: tensors_then_interpolate(prep_t, count, per_sample, out["chain"])) if resized else (lambda: tensors(prep_t, count))
    scaled(prep["bilinear"], count, A.WINDOW_BILINEAR)           # warm-up of every way
    scaled(prep["box"], count, A.WINDOW_BOX)
    third()
    torch.cuda.synchronize()
    t = {"bilinear": [], "box": [], "third": []}
    for _ in range(reps):                                        # alternating
        t["bilinear"].append(timed_ms(scaled, prep["bilinear"], count, A.WINDOW_BILINEAR))
        t["box"].append(timed_ms(scaled, prep["box"], count, A.WINDOW_BOX))
        t["third"].append(timed_ms(third))
    picks = sorted({0, 1, count // 2, count - 1})
    bad = check_against_model(windows, out["bilinear"], S.BILINEAR, picks) + check_against_model(windows, out["box"], S.BOX, picks)
    ref = out["chain"].float()
    texels = count * edge * edge
    row = {"workload": name, "output_texels": texels, "source_texels": int(sum(sw * sh for _, _, sw, sh in windows)), "reps": reps,
           "scaled_bilinear": dict(stats(t["bilinear"]), gtexels_per_s=round(texels / min(t["bilinear"]) / 1e6, 2)),
           "scaled_box": dict(stats(t["box"]), gtexels_per_s=round(texels / min(t["box"]) / 1e6, 2)),
           ("tensors_then_interpolate" if resized else "tensors_alone"): stats(t["third"]),
           "third_over_bilinear_best": round(min(t["third"]) / min(t["bilinear"]), 3), "third_over_box_best": round(min(t["third"]) / min(t["box"]), 3),
           "model_samples": len(picks) * 2, "model_differences": bad,
           "max_abs_difference_to_third": {"bilinear": float((out["bilinear"].float() - ref).abs().max()), "box": float((out["box"].float() - ref).abs().max())}}
    for f, filt in (("bilinear", S.BILINEAR), ("box", S.BOX)):
        decoded, covered = blocks_decoded_and_covered(filt, windows, edge)
        row["blocks_%s" % f] = {"decoded": decoded, "covered": covered, "ratio": round(decoded / covered, 3)}
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"rows": rows, "model_exact": all(r["model_differences"] == 0 for r in rows),
           "scaled_beats_the_chain": all(r["third_over_bilinear_best"] >= 1.0 and r["third_over_box_best"] >= 1.0 for r in rows[:2])}
print(json.dumps({k: summary[k] for k in ("model_exact", "scaled_beats_the_chain")}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
