#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Windows of a compressed image (astcenc_amd_decompress_regions_device) against what a user does without that call:
astcenc_amd_decompress_image_device of the whole image into a scratch image, then torch slicing and stacking into the same
batch tensor.  The source is an 8192^2 RGBA8 image compressed at 6x6 -fastest and kept in device memory.  Three workloads:

  1. 256 random 224^2 crops into a [256, 224, 224, 4] tensor;
  2. 1024 random 64^2 crops into a [1024, 64, 64, 4] tensor;
  3. one 512^2 tile into a [1, 512, 512, 4] tensor.

Both ways run in this process on the same stream, alternating, after a warm-up pass of each; per way the best and the median of
`reps` passes, timed with events on the stream around everything the way does (the scratch image is allocated once, outside the
timed window: decode-then-crop is given its best case).  The two batch tensors must be equal.  Also the full decoder alone, for
the texels/s next to the regions path's.  One JSON line per workload, then a summary line.
usage: time_decode_regions.py [reps] [--size N] [--json out.json]"""
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
assert torch.cuda.is_available(), "needs a HIP device: this tool measures, it does not fall back"
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
SWZ = A.Swizzle(*A.SWZ_RGBA)
stream = torch.cuda.current_stream()

# the stream: a quarter of the image is compressed and tiled (the decoder's time depends on the kinds of block, not on where they are)
tile = size // 2
part = lib.compress(A.synthetic_image(tile, tile), (B, B), A.PRE_FASTEST).reshape(-(-tile // B), -(-tile // B), 16)
nb = -(-size // B)
blocks_np = np.tile(part, (2, 2, 1))[:nb, :nb].copy()
blocks = torch.from_numpy(blocks_np.reshape(-1)).cuda()
err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, A.PRE_FASTEST, A.FLG_DECOMPRESS_ONLY)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
scratch = torch.zeros((size, size, 4), dtype=torch.uint8, device="cuda")
entry = A.compressed_entry(blocks, (size, size), A.TYPE_U8)


def decode_whole():
    e = lib.lib.astcenc_amd_decompress_image_device(ctx, blocks.data_ptr(), blocks.numel(), scratch.data_ptr(), size, size, 1, A.TYPE_U8,
                                                    C.byref(SWZ), stream.cuda_stream)
    assert e == 0, e


def decode_then_crop(at, w, h, batch):
    decode_whole()
    torch.stack([scratch[y:y + h, x:x + w] for x, y in at], out=batch)


def regions(at, w, h, batch, prepared):
    e = lib.lib.astcenc_amd_decompress_regions_device(ctx, C.byref(entry), 1, prepared, len(at), stream.cuda_stream)
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
decode_whole()
torch.cuda.synchronize()
full = sorted(timed_ms(decode_whole) for _ in range(reps))
full_row = {"workload": "full decoder, %d^2" % size, "best_ms": round(full[0], 4), "median_ms": round(full[len(full) // 2], 4),
            "gtexels_per_s": round(size * size / full[0] / 1e6, 2)}
print(json.dumps(full_row), flush=True)
for name, count, edge in (("256 random 224^2 crops", 256, 224), ("1024 random 64^2 crops", 1024, 64), ("one 512^2 tile", 1, 512)):
    edge = min(edge, size)
    at = [(int(rng.integers(0, size - edge + 1)), int(rng.integers(0, size - edge + 1))) for _ in range(count)]
    batch_a = torch.zeros((count, edge, edge, 4), dtype=torch.uint8, device="cuda")
    batch_b = torch.zeros_like(batch_a)
    prepared = (A.DecodeRegion * count)(*[A.decode_region(0, (x, y, 0), (edge, edge, 1), batch_b[i]) for i, (x, y) in enumerate(at)])
    decode_then_crop(at, edge, edge, batch_a)       # warm-up of both ways
    regions(at, edge, edge, batch_b, prepared)
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):                            # alternating
        ta.append(timed_ms(decode_then_crop, at, edge, edge, batch_a))
        tb.append(timed_ms(regions, at, edge, edge, batch_b, prepared))
    ta.sort()
    tb.sort()
    texels = count * edge * edge
    row = {"workload": name, "texels": texels, "reps": reps,
           "decode_then_crop": {"best_ms": round(ta[0], 4), "median_ms": round(ta[len(ta) // 2], 4)},
           "regions": {"best_ms": round(tb[0], 4), "median_ms": round(tb[len(tb) // 2], 4), "gtexels_per_s": round(texels / tb[0] / 1e6, 2)},
           "speedup_best": round(ta[0] / tb[0], 2), "identical": bool(torch.equal(batch_a, batch_b))}
    print(json.dumps(row), flush=True)
    rows.append(row)
lib.context_free(ctx)
summary = {"full_decoder": full_row, "rows": rows, "all_identical": all(r["identical"] for r in rows),
           "regions_never_slower": all(r["speedup_best"] >= 1.0 for r in rows)}
print(json.dumps({k: summary[k] for k in ("all_identical", "regions_never_slower")}))
if out_json:
    with open(out_json, "w") as f:
        json.dump(summary, f, indent=1)
