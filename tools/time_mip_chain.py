#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Mip chain generation and compression (astcenc_amd_generate_mip_chain_device / astcenc_amd_compress_mip_chain_device),
device-resident 8192^2 RGBA8, 6x6 -medium LDR:

  1. generation alone (13 levels below level 0): HIP events around the call on its stream, best of `reps`; then every launch of
     it timed on its own (events around a one-level call per level, which runs the same kernel on the same source), and the
     level 1 step (8192^2 -> 4096^2, 335.5 MB moved) as bytes/s;
  2. compress_mip_chain_device (kernel_ms: every launch, generation included) against torch-side generation (avg_pool2d,
     levels rounded back to uint8) followed by compress_images_device (generation timed with events, compression by kernel_ms).

Everything runs on one torch side stream (torch's default stream is the null handle, which the library reads as "the context's
own stream").  One JSON line per row.  usage: time_mip_chain.py [reps] [size] [--gen-only] [--json out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("-")]
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if out_json in args:
    args.remove(out_json)
reps = int(args[0]) if args else 5
size = int(args[1]) if len(args) > 1 else 8192
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
err, cfg = lib.config_init(A.PRF_LDR, 6, 6, 1, A.PRE_MEDIUM, 0)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
gen_only = "--gen-only" in sys.argv
rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def events_ms(fn, n=reps):
    best = None
    for _ in range(n + 1):                      # (the first pass warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(5_000_000)            # (the device is busy while the host queues the work: e0 -> the first launch is back to back)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None or ms < best else best
    return best


img = torch.from_numpy(A.synthetic_image(size, size)).cuda()
err, lay = lib.mip_chain_layout(cfg, size, size, A.TYPE_U8, 0)
store = torch.empty(lay.texels_len, dtype=torch.uint8, device="cuda")
n = lay.level_count
s = stream.cuda_stream


def generate(levels=0, src=img, w=size, h=size, dst=store, dst_len=lay.texels_len):
    e = lib.lib.astcenc_amd_generate_mip_chain_device(ctx, src.data_ptr(), w, h, A.TYPE_U8, levels, dst.data_ptr(), dst_len, s)
    assert e == 0, e


gen_ms = events_ms(generate)
emit({"row": "generate_chain", "size": size, "levels": n, "ms": gen_ms})
# per level: a two-level call on level i - 1 makes level i with the launch the chain uses for it (the tail: the rest of the chain)
levels = lib.generate_mip_chain_device(ctx, img)
torch.cuda.synchronize()
scratch = torch.empty(lay.texels_len, dtype=torch.uint8, device="cuda")
for i in range(1, n):
    src = levels[i - 1]
    w, h = src.shape[1], src.shape[0]
    tail = w * h <= 4096
    ms = events_ms(lambda: generate(0 if tail else 2, src, w, h, scratch, scratch.numel()))
    moved = (w * h + levels[i].shape[0] * levels[i].shape[1]) * 4
    emit({"row": "generate_level", "level": i, "src": [w, h], "tail_launch": tail, "ms": ms, "bytes": moved, "GB_per_s": moved / ms / 1e6})
    if tail:
        break

if gen_only:
    sys.exit(0)
# compression of the chain in one call vs torch-side generation + compress_images_device
blocks = torch.empty(lay.blocks_len, dtype=torch.uint8, device="cuda")
best = None
for _ in range(max(2, reps // 2) + 1):
    ms = C.c_float(0)
    e = lib.lib.astcenc_amd_compress_mip_chain_device(ctx, img.data_ptr(), size, size, A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), 0,
                                                      store.data_ptr(), lay.texels_len, blocks.data_ptr(), lay.blocks_len, s, C.byref(ms))
    assert e == 0
    best = ms.value if best is None or ms.value < best else best
chain_ms = best


def torch_levels():
    out = [img]
    x = img.permute(2, 0, 1).unsqueeze(0).float()
    for _ in range(1, n):
        x = torch.nn.functional.avg_pool2d(x, 2, ceil_mode=False) if min(x.shape[2:]) > 1 else \
            torch.nn.functional.avg_pool2d(x, (min(2, x.shape[2]), min(2, x.shape[3])))
        out.append(x[0].permute(1, 2, 0).round().to(torch.uint8).contiguous())
    return out


torch_gen_ms = events_ms(torch_levels)
tl = torch_levels()
ours = lib.generate_mip_chain_device(ctx, img)
outs = [torch.empty(lay.blocks_offset[i + 1] - lay.blocks_offset[i] if i + 1 < n else lay.blocks_len - lay.blocks_offset[i],
                    dtype=torch.uint8, device="cuda") for i in range(n)]


def set_ms(levels):
    best = None
    for _ in range(max(2, reps // 2) + 1):
        assert lib.compress_images_device(ctx, list(zip(levels, outs))) == 0
        best = lib.last_kernel_ms if best is None or lib.last_kernel_ms < best else best
    return best


best = set_ms(tl)
ours_set_ms = set_ms(ours)
emit({"row": "compress_chain", "size": size, "levels": n, "compress_mip_chain_ms": chain_ms, "generation_ms": gen_ms,
      "generation_share": gen_ms / chain_ms, "torch_avg_pool2d_ms": torch_gen_ms, "compress_images_ms": best,
      "torch_path_ms": torch_gen_ms + best, "compress_images_on_generated_levels_ms": ours_set_ms})
lib.context_free(ctx)
if out_json:
    json.dump(rows, open(out_json, "w"), indent=1)
