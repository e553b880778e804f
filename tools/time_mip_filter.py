#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The time of the windowed mip filters (astcenc_amd_generate_mip_chain_filtered_device) on device-resident chains:

  for an 8192^2 chain of RGBA8, F16 and F32, a 2048^2 x 16-layer RGBA8 array and a 512^3 RGBA8 volume, the whole chain's
  generation with the box filter and with MITCHELL, LANCZOS3 and KAISER (CLAMP edges); HIP events around the call on its
  stream, best of `reps` (alternating the variants, so that drift hits them alike).  The extra time of a filter is its time
  minus the box's; it includes the upload of the taps, which the call queues on the same stream.

One JSON line per row.  usage: time_mip_filter.py [reps] [--json out.json]"""
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
VARIANTS = [("box", None), ("mitchell", (A.MIP_FILTER_MITCHELL, A.MIP_EDGE_CLAMP)), ("lanczos3", (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CLAMP)),
            ("kaiser", (A.MIP_FILTER_KAISER, A.MIP_EDGE_CLAMP))]


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def image(shape, dtype):
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.rand(shape + (4,), device="cuda", generator=g)
    if dtype == torch.uint8:
        return (v * 255.0 + 0.5).to(torch.uint8)
    return v.to(dtype)


def run(name, img, kind):
    err, cfg = lib.config_init(A.PRF_LDR if img.dtype == torch.uint8 else A.PRF_HDR, 6, 6, 1, A.PRE_FASTEST, 0)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    try:
        best = {}
        for _ in range(reps + 1):                    # (the first round warms up)
            for vname, flt in VARIANTS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda._sleep(5_000_000)         # (the device is busy while the host queues the work)
                e0.record(stream)
                lib.generate_mip_chain_filtered_device(ctx, img, kind, 0, None, flt, stream=stream)
                e1.record(stream)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                best[vname] = min(best.get(vname, ms), ms)
        row = {"case": name, "level0_bytes": img.numel() * img.element_size(), "box_ms": round(best["box"], 4)}
        for vname, _ in VARIANTS[1:]:
            row[vname + "_ms"] = round(best[vname], 4)
            row[vname + "_extra_ms"] = round(best[vname] - best["box"], 4)
        emit(row)
    finally:
        lib.context_free(ctx)


for name, shape, dtype, kind in [("8192^2 rgba8", (1, 8192, 8192), torch.uint8, A.MIP_VOLUME),
                                 ("8192^2 f16", (1, 8192, 8192), torch.float16, A.MIP_VOLUME),
                                 ("8192^2 f32", (1, 8192, 8192), torch.float32, A.MIP_VOLUME),
                                 ("2048^2 x 16 array rgba8", (16, 2048, 2048), torch.uint8, A.MIP_ARRAY),
                                 ("512^3 volume rgba8", (512, 512, 512), torch.uint8, A.MIP_VOLUME)]:
    img = image(shape, dtype)
    run(name, img, kind)
    del img
    torch.cuda.empty_cache()

if out_json:
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
