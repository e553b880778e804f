#!/usr/bin/env python3
# SPDX-License-Identifier: Apache-2.0
"""Adaptive effort (astcenc_amd_compress_image_adaptive_device) against its two presets alone, in one process.

Workload: 8192^2 RGBA8 at 6x6, on bench.py's synthetic image and on its photographic mosaic (the Khronos images of the corpus
tiled to 8192^2; skipped when the corpus is not there).  Base -fast, strong -thorough.

  baselines   astcenc_amd_compress_image_device with each context: kernel_ms, wall time, PSNR (astcenc_amd_compare_blocks_device)
  adaptive    thresholds that select about 10 %, 25 % and 50 % of the blocks -- quantiles of e(E0) / n over the base stream's
              records --: the stats' kernel times (base, strong, other), wall time, PSNR of the final stream, selected and
              replaced counts, and the per-block time of the listed strong launch over the per-block time of the full strong
              launch (kernel_ms_strong / selected against the -thorough baseline's kernel_ms / blocks)

After a warm-up of every call: best and worst of `reps` (default 5) passes.  One JSON line per row.

--set: the image-set driver with a block budget (astcenc_amd_compress_images_adaptive_device) on the full mip chain of the mosaic
(of the bench image when the corpus is not there), threshold 0, so that every block with an error is a candidate:
  baselines   astcenc_amd_compress_images_device with each context: kernel_ms, wall time, PSNR over the whole chain
  budgets     5, 10, 25 and 50 % of the chain's blocks: the three kernel times of the stats, wall time, dB gained over the base
              streams, selected and replaced counts
  selection   astcenc_amd_select_blocks_set_device on the base records with a budget of a third of the candidates and without
              one, against astcenc_amd_compare_image_set_device on the same set (wall time of the synchronous calls)
usage: time_adaptive.py [reps] [--size N] [--json out.json] [--set]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "astc-encoder_amd", "python"))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import astcenc_amd as A  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else 5
size = int(sys.argv[sys.argv.index("--size") + 1]) if "--size" in sys.argv else 8192
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
B = 6
FRACTIONS = (0.10, 0.25, 0.50)
torch.zeros(1, device="cuda")
lib = A.Library(A.LIB_PRODUCT)
stream = torch.cuda.current_stream()
SWZ = A.Swizzle(*A.SWZ_RGBA)


def context(quality):
    err, cfg = lib.config_init(A.PRF_LDR, B, B, 1, quality, 0)
    assert err == 0
    err, ctx = lib.context_alloc(cfg, 1)
    assert err == 0, err
    return ctx


def spread(samples):
    return {"best": round(min(samples), 4), "worst": round(max(samples), 4)}


def walled(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    result = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, result


def images():
    yield "bench image", A.synthetic_image(size, size)
    import bench
    try:
        mosaic, why = bench.khronos_mosaic(size), "the corpus images are not there"
    except ImportError as e:                     # (no PIL; any other error is a bug and surfaces)
        mosaic, why = None, repr(e)
    if mosaic is not None:
        yield "photographic mosaic", mosaic
    else:
        print(json.dumps({"image": "photographic mosaic", "skipped": why}), flush=True)


def set_mode():
    rows = []
    base, strong = context(A.PRE_FAST), context(A.PRE_THOROUGH)
    name, image = list(images())[-1]
    d_img = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    levels = lib.generate_mip_chain_weighted_device(base, d_img[None])
    counts = [(-(-t.shape[2] // B)) * (-(-t.shape[1] // B)) for t in levels]
    nblocks, texels = sum(counts), sum(t.shape[1] * t.shape[2] for t in levels)
    outs = [torch.zeros(c * 16, dtype=torch.uint8, device="cuda") for c in counts]
    entries = list(zip(levels, outs))
    d_err = torch.zeros(nblocks * 4, dtype=torch.float64, device="cuda")
    d_list = torch.zeros(nblocks, dtype=torch.int32, device="cuda")

    def full(ctx):
        assert lib.compress_images_device(ctx, entries) == 0
        return lib.last_kernel_ms

    def score(records=None):
        err, sums = lib.compare_image_set_device(base, entries, block_errors=records)
        assert err == 0
        return sums

    def psnr():
        num = sum(sum(s.squared_error[k] for k in range(4)) for s in score())
        return 999.0 if num == 0 else 10.0 * float(np.log10(texels * 4 / num))

    common = {"image": name + ", mip chain", "size": size, "block": B, "levels": len(levels), "blocks": nblocks, "reps": reps}
    psnr_of = {}
    for what, ctx in (("base -fast alone", base), ("strong -thorough alone", strong)):
        full(ctx)
        wall, kernel = zip(*[walled(lambda: full(ctx)) for _ in range(reps)])
        psnr_of[what] = psnr()
        row = dict(common, run=what, kernel_ms=spread(kernel), wall_ms=spread(wall), psnr_db=round(psnr_of[what], 4),
                   db_over_base=round(psnr_of[what] - psnr_of["base -fast alone"], 4))
        print(json.dumps(row), flush=True)
        rows.append(row)

    criterion = A.block_criterion(0.0)
    for percent in (5, 10, 25, 50):
        budget = nblocks * percent // 100

        def adaptive():
            err, stats = lib.compress_images_adaptive_device(base, strong, entries, criterion, budget, block_errors=d_err)
            assert err == 0
            return stats

        adaptive()
        wall, stats = zip(*[walled(adaptive) for _ in range(reps)])
        s = stats[0]
        total = [x.kernel_ms_base + x.kernel_ms_strong + x.kernel_ms_other for x in stats]
        row = dict(common, run="adaptive set, budget %d %% of the blocks" % percent, max_blocks=budget, candidates=s.candidates, selected=s.selected,
                   replaced=s.replaced, kernel_ms_base=spread([x.kernel_ms_base for x in stats]), kernel_ms_strong=spread([x.kernel_ms_strong for x in stats]),
                   kernel_ms_other=spread([x.kernel_ms_other for x in stats]), kernel_ms_total=spread(total), wall_ms=spread(wall))
        final = psnr()
        row.update(psnr_db=round(final, 4), db_over_base=round(final - psnr_of["base -fast alone"], 4))
        print(json.dumps(row), flush=True)
        rows.append(row)

    # the selection alone against one scoring pass of the same set
    full(base)
    score(d_err)
    dims = [(t.shape[2], t.shape[1], 1) for t in levels]
    err, candidates, _ = lib.select_blocks_set_device(base, dims, d_err, criterion, d_list)
    assert err == 0
    timings = {"scoring pass (astcenc_amd_compare_image_set_device, with records)": lambda: score(d_err),
               "selection, budget of a third of the candidates": lambda: lib.select_blocks_set_device(base, dims, d_err, criterion, d_list, candidates // 3),
               "selection, no budget": lambda: lib.select_blocks_set_device(base, dims, d_err, criterion, d_list)}
    for what, call in timings.items():
        call()
        wall, _ = zip(*[walled(call) for _ in range(max(reps, 5))])
        row = dict(common, run=what, candidates=candidates, wall_ms=spread(wall))
        print(json.dumps(row), flush=True)
        rows.append(row)
    lib.context_free(base)
    lib.context_free(strong)
    if out_json:
        with open(out_json, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if "--set" in sys.argv:
    set_mode()
    sys.exit(0)

rows = []
base, strong = context(A.PRE_FAST), context(A.PRE_THOROUGH)
nblocks = (-(-size // B)) ** 2
for name, image in images():
    d_img = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    d_out = torch.zeros(nblocks * 16, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(nblocks * 4, dtype=torch.float64, device="cuda")

    def full(ctx):
        ms = C.c_float()
        err = lib.lib.astcenc_amd_compress_image_device(ctx, d_img.data_ptr(), size, size, A.TYPE_U8, C.byref(SWZ), d_out.data_ptr(), d_out.numel(),
                                                        stream.cuda_stream, C.byref(ms))
        assert err == 0
        return ms.value

    def psnr(records=None):
        err, sums = lib.compare_blocks_device(base, d_out, d_img, block_errors=records)
        assert err == 0
        return sums.psnr()

    full_ms = {}
    for what, ctx in (("base -fast alone", base), ("strong -thorough alone", strong)):
        full(ctx)
        wall, kernel = zip(*[walled(lambda: full(ctx)) for _ in range(reps)])
        full_ms[what] = min(kernel)
        row = {"image": name, "run": what, "size": size, "block": B, "blocks": nblocks, "reps": reps, "kernel_ms": spread(kernel), "wall_ms": spread(wall),
               "mtexels_per_s": round(size * size / min(kernel) / 1e3, 2), "psnr_db": round(psnr(), 4)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    strong_per_block = full_ms["strong -thorough alone"] / nblocks

    # the thresholds: quantiles of the base stream's per-texel weighted error (equal weights)
    full(base)
    psnr(d_err)
    e0 = d_err.cpu().numpy().reshape(-1, 4)
    n = np.minimum(B, size - np.arange(-(-size // B)) * B)
    per_texel = ((e0[:, 0] + e0[:, 1]) + e0[:, 2] + e0[:, 3]) / (n[:, None] * n[None, :]).reshape(-1)
    for fraction in FRACTIONS:
        threshold = float(np.quantile(per_texel, 1.0 - fraction))
        criterion = A.block_criterion(threshold)

        def adaptive():
            err, stats = lib.compress_image_adaptive_device(base, strong, d_img, criterion, d_out, block_errors=d_err)
            assert err == 0
            return stats

        adaptive()
        wall, stats = zip(*[walled(adaptive) for _ in range(reps)])
        s = stats[0]
        strong_ms = [x.kernel_ms_strong for x in stats]
        total = [x.kernel_ms_base + x.kernel_ms_strong + x.kernel_ms_other for x in stats]
        row = {"image": name, "run": "adaptive, about %d %% selected" % round(fraction * 100), "size": size, "block": B, "blocks": nblocks, "reps": reps,
               "max_mean_squared_error": threshold, "selected": s.selected, "replaced": s.replaced,
               "kernel_ms_base": spread([x.kernel_ms_base for x in stats]), "kernel_ms_strong": spread(strong_ms),
               "kernel_ms_other": spread([x.kernel_ms_other for x in stats]), "kernel_ms_total": spread(total), "wall_ms": spread(wall),
               "mtexels_per_s": round(size * size / min(total) / 1e3, 2), "psnr_db": round(psnr(), 4),
               "listed_over_full_per_block": round(min(strong_ms) / max(s.selected, 1) / strong_per_block, 4) if s.selected else None}
        print(json.dumps(row), flush=True)
        rows.append(row)
    del d_img, d_out, d_err
lib.context_free(base)
lib.context_free(strong)
if out_json:
    with open(out_json, "w") as f:
        json.dump({"rows": rows}, f, indent=1)
