#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Image sets against one call per image (astcenc_amd_compress_images_device / astcenc_amd_decompress_images_device vs
astcenc_amd_compress_image_device / astcenc_amd_decompress_image_device), 6x6 -medium LDR, device-resident RGBA8:

  1. 1024 images of 256^2: 1024 calls, one set call;
  2. the mip chain of a 4096^2 image (13 levels): one call per level, one set call;
  3. the decompression of both sets, the same two ways.

Per row, after one warm-up pass, best of `reps` passes: kernel-only time (compression: the library's kernel_ms, summed over the
calls of a pass; decompression: HIP events on the stream around each call, summed) and wall-clock time of the pass.  The set's
blocks are checked against the per-image calls' blocks.  One JSON line per row, then a summary line.
usage: time_image_set.py [reps] [--json out.json]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 3
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
B = 6
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, A.PRE_MEDIUM, 0)
assert err == 0
err, ctx = lib.context_alloc(cfg, 1)
assert err == 0
stream = torch.cuda.current_stream()
SWZ = A.Swizzle(*A.SWZ_RGBA)


def nblocks(img):
    return -(-img.shape[1] // B) * -(-img.shape[0] // B)


def make_sets():
    imgs = []
    base = A.synthetic_image(256, 256 * 8)
    for i in range(1024):       # 1024 different 256^2 images: slices of 8 tall images, rolled
        k = i % 8
        imgs.append(torch.from_numpy(np.ascontiguousarray(np.roll(base[k * 256:(k + 1) * 256], i // 8, axis=1))).cuda())
    levels = [A.synthetic_image(4096, 4096)]
    while levels[-1].shape[0] > 1:
        a = levels[-1].astype(np.uint32)
        levels.append(((a[0::2, 0::2] + a[1::2, 0::2] + a[0::2, 1::2] + a[1::2, 1::2] + 2) // 4).astype(np.uint8))
    return {"1024 x 256^2": imgs, "4096^2 mip chain (%d levels)" % len(levels): [torch.from_numpy(lv).cuda() for lv in levels]}


def compress_each(imgs, outs):
    total = 0.0
    ms = C.c_float()
    for im, o in zip(imgs, outs):
        e = lib.lib.astcenc_amd_compress_image_device(ctx, im.data_ptr(), im.shape[1], im.shape[0], A.TYPE_U8, C.byref(SWZ),
                                                      o.data_ptr(), o.numel(), stream.cuda_stream, C.byref(ms))
        assert e == 0, e
        total += ms.value
    return total


def compress_set(imgs, outs):
    assert lib.compress_images_device(ctx, list(zip(imgs, outs)), stream) == 0
    return lib.last_kernel_ms


def decompress_each(imgs, outs):
    total = 0.0
    for im, o in zip(imgs, outs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        e = lib.lib.astcenc_amd_decompress_image_device(ctx, o.data_ptr(), o.numel(), im.data_ptr(), im.shape[1], im.shape[0], 1,
                                                        A.TYPE_U8, C.byref(SWZ), stream.cuda_stream)
        assert e == 0, e
        e1.record(stream)
        e1.synchronize()
        total += e0.elapsed_time(e1)
    return total


def decompress_set(imgs, outs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    assert lib.decompress_images_device(ctx, list(zip(imgs, outs)), stream) == 0
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, *args):
    fn(*args)                   # warm-up
    best_k, best_w = 1e30, 1e30
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = fn(*args)
        torch.cuda.synchronize()
        best_w = min(best_w, (time.perf_counter() - t0) * 1e3)
        best_k = min(best_k, k)
    return best_k, best_w


rows = []
for name, imgs in make_sets().items():
    texels = sum(im.shape[0] * im.shape[1] for im in imgs)
    blocks = sum(nblocks(im) for im in imgs)
    outs_each = [torch.zeros(nblocks(im) * 16, dtype=torch.uint8, device="cuda") for im in imgs]
    outs_set = [torch.zeros_like(o) for o in outs_each]
    for what, each, one, args_each, args_set in (
            ("compress", compress_each, compress_set, (imgs, outs_each), (imgs, outs_set)),
            ("decompress", decompress_each, decompress_set, None, None)):
        if what == "decompress":
            # decode the (identical) blocks both ways into two sets of images
            back_each = [torch.zeros_like(im) for im in imgs]
            back_set = [torch.zeros_like(im) for im in imgs]
            args_each, args_set = (back_each, outs_each), (back_set, outs_set)
        ke, we = timed(each, *args_each)
        ks, ws = timed(one, *args_set)
        if what == "compress":
            same = all(torch.equal(a, b) for a, b in zip(outs_each, outs_set))
        else:
            same = all(torch.equal(a, b) for a, b in zip(back_each, back_set))
        row = {"set": name, "op": what, "images": len(imgs), "blocks": blocks, "texels": texels,
               "per_image_calls": {"kernel_ms": round(ke, 3), "wall_ms": round(we, 3)},
               "one_set_call": {"kernel_ms": round(ks, 3), "wall_ms": round(ws, 3)},
               "speedup_kernel": round(ke / ks, 3), "speedup_wall": round(we / ws, 3),
               "set_mtexels_per_s_wall": round(texels / ws / 1e3, 1), "identical": same}
        print(json.dumps(row), flush=True)
        rows.append(row)
lib.context_free(ctx)
summary = {"rows": len(rows), "all_identical": all(r["identical"] for r in rows),
           "set_never_slower_wall": all(r["speedup_wall"] >= 1.0 for r in rows),
           "set_never_slower_kernel": all(r["speedup_kernel"] >= 1.0 for r in rows)}
print(json.dumps(summary))
if out_json:
    with open(out_json, "w") as f:
        json.dump({"rows": rows, "summary": summary}, f, indent=1)
