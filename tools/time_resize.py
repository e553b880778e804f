#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The time of astcenc_amd_resize_image_device on device-resident images:

  * the halving step both ways: 8192^2 -> 4096^2 RGBA8 LANCZOS3 CLAMP through the resize call and through
    astcenc_amd_generate_mip_chain_weighted_device with level_count = 2 (the chain's own kernel), in one process on the same
    buffers, alternating, best of `reps`; the target is at most 1.25x the chain's figure;
  * 8192^2 -> 3000^2, 8192^2 -> 1000^2 and the enlargement 2048^2 -> 4096^2, RGBA8 and F16, plain and alpha-weighted, LANCZOS3
    and the box (no target).

HIP events around the call on its stream (the upload of the taps, which the call queues on the same stream, included); the
kernel's own time as the call reports it (kernel_ms) beside it.  One JSON line per row.
usage: time_resize.py [reps] [--json out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

argv = sys.argv[1:]
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
plain = [a for i, a in enumerate(argv) if not a.startswith("-") and (i == 0 or argv[i - 1] != "--json")]
reps = int(plain[0]) if plain else 10
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
rows = []
LANCZOS = (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP)
BOX = (A.MIP_FILTER_BOX, A.MIP_EDGE_CLAMP)


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def image(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.rand(shape + (4,), device="cuda", generator=g)
    if dtype == torch.uint8:
        return (v * 255.0 + 0.5).to(torch.uint8)
    return v.to(dtype)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(5_000_000)         # (the device is busy while the host queues the work)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def context(dtype):
    err, cfg = lib.config_init(A.PRF_LDR if dtype == torch.uint8 else A.PRF_HDR, 6, 6, 1, A.PRE_FASTEST, 0)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    return ctx


def halving(img):
    """The same step through both calls, for LANCZOS3 and the box, plain and weighted."""
    ctx = context(img.dtype)
    h, w = img.shape[1], img.shape[2]
    try:
        for fname, flt in (("lanczos3", LANCZOS), ("box", BOX)):
            for weight in (A.MIP_WEIGHT_NONE, A.MIP_WEIGHT_ALPHA):
                best = {}
                for _ in range(reps + 1):                    # (the first round warms up)
                    for name, call in (("chain", lambda: lib.generate_mip_chain_weighted_device(ctx, img, A.MIP_VOLUME, 2, None, flt, stream=stream,
                                                                                                 weighting=weight)),
                                       ("resize", lambda: lib.resize_image_device(ctx, img, (w // 2, h // 2), A.MIP_VOLUME, flt, weight,
                                                                                  stream=stream))):
                        ms = timed(call)
                        best[name] = min(best.get(name, ms), ms)
                        if name == "resize":
                            best["kernel"] = min(best.get("kernel", lib.last_kernel_ms), lib.last_kernel_ms)
                emit({"case": "%d^2 -> %d^2 %s" % (w, w // 2, str(img.dtype).split(".")[1]), "filter": fname, "weighted": bool(weight),
                      "chain_ms": round(best["chain"], 4), "resize_ms": round(best["resize"], 4), "resize_kernel_ms": round(best["kernel"], 4),
                      "ratio": round(best["resize"] / best["chain"], 3)})
    finally:
        lib.context_free(ctx)


def general(img, size):
    ctx = context(img.dtype)
    try:
        for fname, flt in (("lanczos3", LANCZOS), ("box", BOX)):
            for weight in (A.MIP_WEIGHT_NONE, A.MIP_WEIGHT_ALPHA):
                best, kernel = None, None
                for _ in range(reps + 1):
                    ms = timed(lambda: lib.resize_image_device(ctx, img, size, A.MIP_VOLUME, flt, weight, stream=stream))
                    best = ms if best is None else min(best, ms)
                    kernel = lib.last_kernel_ms if kernel is None else min(kernel, lib.last_kernel_ms)
                emit({"case": "%d^2 -> %d^2 %s" % (img.shape[2], size[0], str(img.dtype).split(".")[1]), "filter": fname, "weighted": bool(weight),
                      "resize_ms": round(best, 4), "resize_kernel_ms": round(kernel, 4)})
    finally:
        lib.context_free(ctx)


for dtype in (torch.uint8, torch.float16):
    img = image((1, 8192, 8192), dtype)
    halving(img)
    general(img, (3000, 3000))
    general(img, (1000, 1000))
    del img
    torch.cuda.empty_cache()
    img = image((1, 2048, 2048), dtype)
    general(img, (4096, 4096))
    del img
    torch.cuda.empty_cache()

if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
