#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Mip chains of volumes and texture arrays (astcenc_amd_generate_mip_chain_volume_device /
astcenc_amd_compress_mip_chain_volume_device), device-resident RGBA8:

  1. the first step alone (a one-level-below call, level_count = 2), HIP events around the call on its stream, best of `reps`,
     as bytes/s: a 512^3 volume -> 256^3, and a 2048^2 x 16-layer array -> 1024^2 x 16 (the bytes of the 2D 8192^2 step);
  2. the whole chain's generation against its compression in one call (kernel_ms, generation included): the 2048^2 x 16
     array at 6x6 -medium and a 256^3 volume at 4x4x4 -medium.

Everything runs on one torch side stream (the null handle means "the context's own stream" to the library).  One JSON line
per row.  usage: time_mip_chain_volume.py [reps] [--kind array|volume] [--json out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

argv = sys.argv[1:]
out_json = argv[argv.index("--json") + 1] if "--json" in argv else None
only = argv[argv.index("--kind") + 1] if "--kind" in argv else None
plain = [a for i, a in enumerate(argv) if not a.startswith("-") and (i == 0 or argv[i - 1] not in ("--json", "--kind"))]
reps = int(plain[0]) if plain else 5
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def events_ms(fn, n=reps):
    best = None
    for _ in range(n + 1):                      # (the first pass warms up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(5_000_000)            # (the device is busy while the host queues the work)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None or ms < best else best
    return best


def context(block, quality=A.PRE_MEDIUM):
    err, cfg = lib.config_init(A.PRF_LDR, block[0], block[1], block[2], quality, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    return ctx


def case(name, kind, shape, block):
    """shape: (z, h, w).  The first step, the whole chain's generation, the chain's compression."""
    ctx = context(block)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        img = torch.randint(0, 256, shape + (4,), dtype=torch.uint8, device="cuda", generator=g)
        one = lambda: lib.generate_mip_chain_volume_device(ctx, img, kind, 2, stream)  # noqa: E731
        ms = events_ms(one)
        dst = one()[1]
        moved = img.numel() + dst.numel()
        emit({"row": "first_step", "case": name, "src": list(shape), "dst": list(dst.shape[:3]), "ms": ms, "bytes": moved,
              "GB_per_s": moved / ms / 1e6})
        gen_ms = events_ms(lambda: lib.generate_mip_chain_volume_device(ctx, img, kind, 0, stream))
        best = None
        for _ in range(max(2, reps // 2)):
            lib.compress_mip_chain_volume_device(ctx, img, kind, 0, A.SWZ_RGBA, stream)
            best = lib.last_kernel_ms if best is None or lib.last_kernel_ms < best else best
        emit({"row": "chain", "case": name, "block": "x".join(map(str, block)), "generation_ms": gen_ms, "compress_chain_ms": best,
              "generation_share": gen_ms / best})
    finally:
        lib.context_free(ctx)


if only in (None, "volume"):
    case("volume 512^3", A.MIP_VOLUME, (512, 512, 512), (4, 4, 4))
    case("volume 256^3", A.MIP_VOLUME, (256, 256, 256), (4, 4, 4))
if only in (None, "array"):
    case("array 2048^2 x 16", A.MIP_ARRAY, (16, 2048, 2048), (6, 6, 1))
if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
