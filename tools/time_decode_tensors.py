#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Windows of a compressed image straight into a training tensor (astcenc_amd_decompress_tensors_device) against what a user does
without that call: astcenc_amd_decompress_regions_device into a [N, h, w, 4] u8 tensor, then the torch chain to [N, 3, h, w] fp16
-- slice off alpha, permute, convert, scale, shift, narrow, mirror every other sample.  The source is an 8192^2 RGBA8 image
compressed at 6x6 -fastest and kept in device memory.  Three workloads:

  1. 256 random 224^2 crops;
  2. 1024 random 64^2 crops;
  3. one 512^2 tile.

All ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does (every buffer is allocated once, outside the
timed window; the chain's intermediates are torch's own).  The two tensors must be bitwise equal.  The plain regions call is
timed alone as well: the margin the conversion costs.  One JSON line per workload, then a summary line.
usage: time_decode_tensors.py [reps] [--size N] [--json out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

args = sys.argv[1:]
reps = int(args[0]) if args and not args[0].startswith("-") else 20
size = int(args[args.index("--size") + 1]) if "--size" in args else 8192
out_json = args[args.index("--json") + 1] if "--json" in args else None
B = 6
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
# the chain multiplies and adds the very float32 values the call is given
scale_t = torch.tensor(list(fmt.scale)[:3], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)
bias_t = torch.tensor(list(fmt.bias)[:3], dtype=torch.float32, device="cuda").view(1, 3, 1, 1)


def regions(prepared, count):
    e = lib.lib.astcenc_amd_decompress_regions_device(ctx, C.byref(entry), 1, prepared, count, stream.cuda_stream)
    assert e == 0, e


def regions_then_chain(prepared, count, rgba, out):
    regions(prepared, count)
    x = rgba[..., :3].permute(0, 3, 1, 2).to(torch.float32)
    y = ((x * scale_t) + bias_t).to(torch.float16)
    out[0::2] = y[0::2]
    out[1::2] = y[1::2].flip(-1)


def tensors(prepared, count):
    e = lib.lib.astcenc_amd_decompress_tensors_device(ctx, C.byref(entry), 1, C.byref(fmt), prepared, count, stream.cuda_stream)
    assert e == 0, e


def timed_ms(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn(*a)
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
rng = np.random.default_rng(1)
for name, count, edge in (("256 random 224^2 crops", 256, 224), ("1024 random 64^2 crops", 1024, 64), ("one 512^2 tile", 1, 512)):
    edge = min(edge, size)
    at = [(int(rng.integers(0, size - edge + 1)), int(rng.integers(0, size - edge + 1))) for _ in range(count)]
    rgba = torch.zeros((count, edge, edge, 4), dtype=torch.uint8, device="cuda")
    out_a = torch.zeros((count, 3, edge, edge), dtype=torch.float16, device="cuda")
    out_b = torch.zeros_like(out_a)
    prep_r = (A.DecodeRegion * count)(*[A.decode_region(0, (x, y, 0), (edge, edge, 1), rgba[i]) for i, (x, y) in enumerate(at)])
    prep_t = (A.TensorRegion * count)(*[A.tensor_region(0, (x, y, 0), (edge, edge, 1), out_b[i], flip_x=i % 2 == 1) for i, (x, y) in enumerate(at)])
    regions_then_chain(prep_r, count, rgba, out_a)       # warm-up of every way
    tensors(prep_t, count)
    regions(prep_r, count)
    torch.cuda.synchronize()
    ta, tb, tr = [], [], []
    for _ in range(reps):                                # alternating
        ta.append(timed_ms(regions_then_chain, prep_r, count, rgba, out_a))
        tb.append(timed_ms(tensors, prep_t, count))
        tr.append(timed_ms(regions, prep_r, count))
    ta.sort()
    tb.sort()
    tr.sort()
    texels = count * edge * edge
    row = {"workload": name, "texels": texels, "reps": reps,
           "regions_then_chain": {"best_ms": round(ta[0], 4), "median_ms": round(ta[len(ta) // 2], 4)},
           "tensors": {"best_ms": round(tb[0], 4), "median_ms": round(tb[len(tb) // 2], 4), "gtexels_per_s": round(texels / tb[0] / 1e6, 2)},
           "regions_alone": {"best_ms": round(tr[0], 4), "median_ms": round(tr[len(tr) // 2], 4)},
           "speedup_best": round(ta[0] / tb[0], 2), "over_regions_alone_best": round(tb[0] / tr[0], 3),
           "identical": bool(torch.equal(out_a.view(torch.int16), out_b.view(torch.int16)))}
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"rows": rows, "all_identical": all(r["identical"] for r in rows), "tensors_never_slower": all(r["speedup_best"] >= 1.0 for r in rows)}
print(json.dumps({k: summary[k] for k in ("all_identical", "tensors_never_slower")}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
