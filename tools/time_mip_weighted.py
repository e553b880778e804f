#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The time of alpha-weighted mip generation (astcenc_amd_generate_mip_chain_weighted_device) against the plain filter, on the
same device-resident buffers in the same process:

  the 8192^2 -> 4096^2 RGBA8 step alone (level_count 2), the whole 8192^2 chain of RGBA8, F16 and F32, a 2048^2 x 16-layer
  RGBA8 array and a 512^3 RGBA8 volume; each with the box filter and with LANCZOS3 (CLAMP edges), plain (a null weighting) and
  with ASTCENC_AMD_MIP_WEIGHT_ALPHA; HIP events around the call on its stream, best of `reps` (alternating the variants, so
  that drift hits them alike).  Alpha is 0 in the left half of the image and random elsewhere.

One JSON line per row.  usage: time_mip_weighted.py [reps] [--json out.json]"""
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
FILTERS = [("box", None), ("lanczos3", (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP))]
VARIANTS = [(f, flt, w, wt) for f, flt in FILTERS for w, wt in (("plain", None), ("weighted", A.MIP_WEIGHT_ALPHA))]


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def image(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.rand(shape + (4,), device="cuda", generator=g)
    v[:, :, :shape[2] // 2, 3] = 0.0
    if dtype == torch.uint8:
        return (v * 255.0 + 0.5).to(torch.uint8)
    return v.to(dtype)


def run(name, img, kind, levels):
    err, cfg = lib.config_init(A.PRF_LDR if img.dtype == torch.uint8 else A.PRF_HDR, 6, 6, 1, A.PRE_FASTEST, 0)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    try:
        best = {}
        for _ in range(reps + 1):                    # (the first round warms up)
            for fname, flt, wname, wt in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(5_000_000)         # (the device is busy while the host queues the work)
                e0.record(stream)
                lib.generate_mip_chain_weighted_device(ctx, img, kind, levels, None, flt, stream=stream, weighting=wt)
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                best[fname, wname] = min(best.get((fname, wname), ms), ms)
        row = {"case": name, "level0_bytes": img.numel() * img.element_size()}
        for fname, _ in FILTERS:
            p, w = best[fname, "plain"], best[fname, "weighted"]
            row.update({fname + "_plain_ms": round(p, 4), fname + "_weighted_ms": round(w, 4), fname + "_ratio": round(w / p, 3)})
        emit(row)
    finally:
        lib.context_free(ctx)


for name, shape, dtype, kind, levels in [("8192^2 -> 4096^2 step rgba8", (1, 8192, 8192), torch.uint8, A.MIP_VOLUME, 2),
                                         ("8192^2 rgba8", (1, 8192, 8192), torch.uint8, A.MIP_VOLUME, 0),
                                         ("8192^2 f16", (1, 8192, 8192), torch.float16, A.MIP_VOLUME, 0),
                                         ("8192^2 f32", (1, 8192, 8192), torch.float32, A.MIP_VOLUME, 0),
                                         ("2048^2 x 16 array rgba8", (16, 2048, 2048), torch.uint8, A.MIP_ARRAY, 0),
                                         ("512^3 volume rgba8", (512, 512, 512), torch.uint8, A.MIP_VOLUME, 0)]:
    img = image(shape, dtype)
    run(name, img, kind, levels)
    del img
    torch.cuda.empty_cache()

if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
