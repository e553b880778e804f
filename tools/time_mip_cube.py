#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The time of mip generation with seamless cube edges (ASTCENC_AMD_MIP_EDGE_CUBE) against CLAMP, on the same device-resident
buffers in the same process:

  the whole chain of a 6 x 2048^2 cube map and of 96 x 64^2 (16 small cubes: the whole chain runs in the tail kernel), RGBA8, F16
  and F32, LANCZOS3 and MITCHELL, plain and with ASTCENC_AMD_MIP_WEIGHT_ALPHA; HIP events around the call on its stream, best
  of `reps` (alternating the edges, so that drift hits them alike);

  then the 6 x 2048^2 RGBA8 LANCZOS3 CUBE chain through astcenc_amd_compress_mip_chain_filtered_device at 6x6 -medium: the
  call's kernel_ms (generation and compression) next to the generation alone.

A library that refuses CUBE (one built before the edge existed, given with --lib) is timed with CLAMP alone.

One JSON line per row.  usage: time_mip_cube.py [reps] [--json out.json] [--lib libastcenc_amd.so]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

argv = sys.argv[1:]
named = {k: argv[argv.index(k) + 1] for k in ("--json", "--lib") if k in argv}
plain_args = [a for i, a in enumerate(argv) if not a.startswith("-") and (i == 0 or argv[i - 1] not in named)]
reps = int(plain_args[0]) if plain_args else 10
torch.zeros(1, device="cuda")
lib = A.Library(named.get("--lib", A.LIB_PRODUCT))
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
rows = []
EDGES = [("clamp", A.MIP_EDGE_CLAMP), ("cube", A.MIP_EDGE_CUBE)]
FILTERS = [("lanczos3", A.MIP_FILTER_LANCZOS3), ("mitchell", A.MIP_FILTER_MITCHELL)]
WEIGHTS = [("plain", None), ("weighted", A.MIP_WEIGHT_ALPHA)]


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


def context(img, quality):
    err, cfg = lib.config_init(A.PRF_LDR if img.dtype == torch.uint8 else A.PRF_HDR, 6, 6, 1, quality, 0)
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    return ctx


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(5_000_000)                     # (the device is busy while the host queues the work)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(name, img):
    ctx = context(img, A.PRE_FASTEST)
    try:
        edges = list(EDGES)
        try:
            lib.generate_mip_chain_filtered_device(ctx, img, A.MIP_ARRAY, 0, None, (A.MIP_FILTER_MITCHELL, A.MIP_EDGE_CUBE), stream=stream)
        except A.AstcError:
            edges = EDGES[:1]
        for fname, kind in FILTERS:
            for wname, wt in WEIGHTS:
                best = {}
                for _ in range(reps + 1):            # (the first round warms up)
                    for ename, edge in edges:
                        ms = timed(lambda: lib.generate_mip_chain_weighted_device(ctx, img, A.MIP_ARRAY, 0, None, (kind, edge), stream=stream,
                                                                                  weighting=wt))
                        best[ename] = min(best.get(ename, ms), ms)
                row = {"case": name, "filter": fname, "weighting": wname, "clamp_ms": round(best["clamp"], 4)}
                if "cube" in best:
                    row.update({"cube_ms": round(best["cube"], 4), "ratio": round(best["cube"] / best["clamp"], 3)})
                emit(row)
    finally:
        lib.context_free(ctx)


def run_compress(name, img):
    ctx = context(img, A.PRE_MEDIUM)
    flt = (A.MIP_FILTER_LANCZOS3, A.MIP_EDGE_CUBE)
    try:
        try:
            gen = min(timed(lambda: lib.generate_mip_chain_filtered_device(ctx, img, A.MIP_ARRAY, 0, None, flt, stream=stream)) for _ in range(reps + 1))
        except A.AstcError:
            return
        total = []
        for _ in range(3):
            lib.compress_mip_chain_filtered_device(ctx, img, A.MIP_ARRAY, 0, None, flt, stream=stream)
            stream.synchronize()
            total.append(lib.last_kernel_ms)
        emit({"case": name + " lanczos3 cube, 6x6 -medium", "generate_ms": round(gen, 4), "generate_and_compress_kernel_ms": round(min(total), 3),
              "generate_share": round(gen / (min(total) - gen), 5)})
    finally:
        lib.context_free(ctx)


for name, shape, dtype in [("6 x 2048^2 rgba8", (6, 2048, 2048), torch.uint8), ("6 x 2048^2 f16", (6, 2048, 2048), torch.float16),
                           ("6 x 2048^2 f32", (6, 2048, 2048), torch.float32), ("96 x 64^2 rgba8", (96, 64, 64), torch.uint8),
                           ("96 x 64^2 f16", (96, 64, 64), torch.float16), ("96 x 64^2 f32", (96, 64, 64), torch.float32)]:
    img = image(shape, dtype)
    run(name, img)
    if name == "6 x 2048^2 rgba8":
        run_compress(name, img)
    del img
    torch.cuda.empty_cache()

if out_json := named.get("--json"):
    with open(out_json, "w") as f:
        json.dump(rows, f, indent=1)
