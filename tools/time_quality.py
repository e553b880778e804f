#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""The fused quality call against the two calls it replaces, in one process:

  astcenc_amd_compare_blocks_device                      (no decoded image in memory)
  astcenc_amd_decompress_image_device + astcenc_amd_compare_images_device   (a scratch image the size of the texture)

on the blocks the library compresses (-medium) from bench.py's images: 8192^2 RGBA8 at 6x6 and at 8x8, 4096^2 RGBA16F at 6x6
(HDR profile; LDR sums, and a fourth row with the HDR sums over f-stops -10..10).  Buffers are allocated through torch.  Per
call, after a warm-up: wall time of the synchronous call (launches, kernels, the host's wait, the sums' copy) and the time
between two events on the stream around it; best and worst of `reps` (default 5) passes, the passes of the two paths
interleaved.  The fused sums are checked against the two calls' (1e-12 relative).  One JSON line per row.
--config N runs row N (0-based) alone, as a counter collection wants it.
usage: time_quality.py [reps] [--per-block] [--config N] [--json out.json]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 5
per_block = "--per-block" in sys.argv
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()
SWZ = A.Swizzle(*A.SWZ_RGBA)
CONFIGS = [("8192^2 RGBA8 6x6", 8192, 6, False, None), ("8192^2 RGBA8 8x8", 8192, 8, False, None),
           ("4096^2 RGBA16F 6x6", 4096, 6, True, None), ("4096^2 RGBA16F 6x6, HDR sums -10..10", 4096, 6, True, (-10, 10))]


def timed(call):
    """(wall ms, events ms) of one synchronous call."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record(stream)
    assert call() == 0
    e1.record(stream)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def spread(samples):
    return {"best_ms": round(min(samples), 4), "worst_ms": round(max(samples), 4)}


rows = []
if "--config" in sys.argv:
    CONFIGS = [CONFIGS[int(sys.argv[sys.argv.index("--config") + 1])]]
for name, size, B, hdr_image, stops in CONFIGS:
    profile = A.PRF_HDR if hdr_image else A.PRF_LDR
    ttype = A.TYPE_F16 if hdr_image else A.TYPE_U8
    err, cfg = lib.config_init(profile, B, B, 1, A.PRE_MEDIUM, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0
    image = A.synthetic_hdr_image(size, size).astype(np.float16) if hdr_image else A.synthetic_image(size, size)
    d_img = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    nblocks = (-(-size // B)) ** 2
    d_blocks = torch.zeros(nblocks * 16, dtype=torch.uint8, device="cuda")
    ms = C.c_float()
    assert lib.lib.astcenc_amd_compress_image_device(ctx, d_img.data_ptr(), size, size, ttype, C.byref(SWZ), d_blocks.data_ptr(), d_blocks.numel(),
                                                     stream.cuda_stream, C.byref(ms)) == 0
    d_dec = torch.empty_like(d_img)              # the scratch image of the two-call path
    d_err = torch.zeros(nblocks * 4, dtype=torch.float64, device="cuda") if per_block else None
    two, fused_sums, two_h, fused_h = A.ErrorSums(), A.ErrorSums(), A.HdrErrorSums(), A.HdrErrorSums()
    decode = lambda: lib.lib.astcenc_amd_decompress_image_device(ctx, d_blocks.data_ptr(), d_blocks.numel(), d_dec.data_ptr(), size, size, 1, ttype,
                                                                C.byref(SWZ), stream.cuda_stream)
    block_args = [ctx, d_blocks.data_ptr(), d_blocks.numel(), d_img.data_ptr(), size, size, 1, ttype, ttype, C.byref(SWZ),
                  d_err.data_ptr() if per_block else None, nblocks * 32 if per_block else 0]
    if stops is None:
        compare = lambda: lib.lib.astcenc_amd_compare_images_device(ctx, d_img.data_ptr(), ttype, d_dec.data_ptr(), ttype, size, size, 1, stream.cuda_stream,
                                                                   C.byref(two))
        fused = lambda: lib.lib.astcenc_amd_compare_blocks_device(*block_args, stream.cuda_stream, C.byref(fused_sums))
    else:
        compare = lambda: lib.lib.astcenc_amd_compare_images_hdr_device(ctx, d_img.data_ptr(), ttype, d_dec.data_ptr(), ttype, size, size, 1, stops[0], stops[1],
                                                                       stream.cuda_stream, C.byref(two), C.byref(two_h))
        fused = lambda: lib.lib.astcenc_amd_compare_blocks_hdr_device(*block_args, stops[0], stops[1], stream.cuda_stream, C.byref(fused_sums), C.byref(fused_h))
    for call in (decode, compare, fused):        # warm-up (the first fused call also allocates the library's scratch)
        timed(call)
    samples = {"decode": [], "compare": [], "fused": []}
    for _ in range(reps):
        for what, call in (("decode", decode), ("compare", compare), ("fused", fused)):
            samples[what].append(timed(call))
    want = np.array(list(two.squared_error) + list(two.alpha_scaled_squared_error) + (list(two_h.log2_squared_error) + list(two_h.mpsnr_squared_error) if stops else []))
    got = np.array(list(fused_sums.squared_error) + list(fused_sums.alpha_scaled_squared_error) +
                   (list(fused_h.log2_squared_error) + list(fused_h.mpsnr_squared_error) if stops else []))
    agree = bool(np.allclose(got, want, rtol=1e-12, atol=0)) and fused_sums.rgb_peak == two.rgb_peak and fused_sums.texels == two.texels
    wall = {k: [s[0] for s in v] for k, v in samples.items()}
    events = {k: [s[1] for s in v] for k, v in samples.items()}
    two_wall = [a + b for a, b in zip(wall["decode"], wall["compare"])]
    two_events = [a + b for a, b in zip(events["decode"], events["compare"])]
    row = {"config": name, "reps": reps, "per_block_output": per_block, "blocks": nblocks, "psnr_db": round(fused_sums.psnr(), 4),
           "two_calls_wall": spread(two_wall), "fused_wall": spread(wall["fused"]),
           "two_calls_events": spread(two_events), "fused_events": spread(events["fused"]),
           "decode_events": spread(events["decode"]), "compare_events": spread(events["compare"]),
           "fused_over_two_calls_wall": round(min(wall["fused"]) / min(two_wall), 4),
           "fused_over_two_calls_events": round(min(events["fused"]) / min(two_events), 4),
           "scratch_image_bytes_saved": d_dec.numel() * d_dec.element_size(), "sums_agree": agree}
    print(json.dumps(row), flush=True)
    rows.append(row)
    lib.context_free(ctx)
    del d_img, d_dec, d_blocks, d_err
summary = {"rows": len(rows), "all_agree": all(r["sums_agree"] for r in rows),
           "fused_never_slower_wall": all(r["fused_over_two_calls_wall"] <= 1.0 for r in rows)}
print(json.dumps(summary))
if out_json:
    with open(out_json, "w") as f:
        json.dump({"rows": rows, "summary": summary}, f, indent=1)
