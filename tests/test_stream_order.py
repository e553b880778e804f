# SPDX-License-Identifier: Apache-2.0
"""Every call that takes a hip_stream is ordered after the work queued before it, and complete when it returns.

A NULL hip_stream is the context's own stream, which is non-blocking: it does not wait for the legacy null stream, and the
legacy null stream is torch's default stream (handle 0).  astcenc_amd.torch_stream() therefore synchronises torch's default
stream before it hands out handle 0.  Without that, a call made under torch's default stream starts while the kernels and copies
torch queued before it -- the call's inputs, fills of its outputs -- are still pending.  The suite's other tests cannot see that:
they upload from pageable memory (synchronous for the host) and their fills are over before the library's host side is.

TABLE has one row per call: every method of Library that takes a stream and the five exported calls that no such method
reaches (through ctypes).  A row names
its device inputs, says whether the caller owns the outputs, and builds the call on a small workload (a 48x48 RGBA8 image at 6x6
-fastest; a 24x24x8 volume at 4x4x4; chains of three levels; grids of 33x9 points).  Every input has two contents, A and B.

Modes: (a) torch's default stream is current, stream=None; (b) a side stream is current, stream=None; (c) the default stream is
current and stream=side is passed after side.wait_stream.

  inputs arrive in time    the buffer holds A; a sleep and a non-blocking copy of B from pinned memory are queued on the mode's
                           stream; the call must give, bit for bit, what it gives on B after torch.cuda.synchronize() -- and
                           that differs from what it gives on A
  outputs are not overwritten  a sleep and a guard fill of every output are queued; the call's results must survive the fill
  complete on return       hip_stream NULL; the outputs are read at once on a fresh stream that waits for nothing
  autograd                 Library.sample_lod under the default stream, coordinates, levels of detail and the upstream gradient
                           made by torch kernels queued behind sleeps

The arithmetic is proven elsewhere; what is compared here is a call with itself.  The delay is long enough by construction: the
queued prefix (timed with events) is at least RATIO times the host wall time of the row's synchronised call, so an unordered call
is over before its input lands and a defect fails every time.  A row that misses the ratio gets a longer sleep (SLEEP_SCALE)."""
import ctypes as C
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SLEEP = 20_000_000          # cycles, as the other ordering tests
SLEEP_SCALE = {}            # row -> multiple of SLEEP, for rows whose synchronised call is too slow for RATIO at SLEEP
RATIO = 4
GUARD = 0xA5
MODES = ("a", "b", "c")
GRID = (33, 9)              # points: x, y
LEVELS = 3


class Buf:
    """A device buffer and its two contents in pinned memory."""

    def __init__(self, a, b):
        import torch
        assert a.shape == b.shape and a.dtype == b.dtype and not np.array_equal(a, b, equal_nan=True)
        self.host = {"A": torch.from_numpy(np.ascontiguousarray(a)).pin_memory(), "B": torch.from_numpy(np.ascontiguousarray(b)).pin_memory()}
        self.t = torch.empty(a.shape, dtype=self.host["A"].dtype, device="cuda")

    def put(self, which):
        self.t.copy_(self.host[which], non_blocking=True)


class Row:
    """inputs: {name: Buf}; outputs: the device tensors the caller owns and the call writes; call(stream) makes the call and
    returns what else it gives: tensors the wrapper allocated, host results as bytes."""

    def __init__(self, inputs, outputs, call):
        self.inputs, self.outputs, self.call = inputs, outputs, call
        self.want, self.wall_ms = {}, None

    def reset(self, fill=True):
        """Every input holds A, every output the guard; nothing pending."""
        import torch
        for b in self.inputs.values():
            b.put("A")
        if fill:
            self.fill()
        torch.cuda.synchronize()

    def fill(self):
        import torch
        for o in self.outputs:
            o.view(torch.uint8).fill_(GUARD)

    def results(self, extra):
        """The outputs and `extra` as bytes, after everything has completed."""
        import torch
        torch.cuda.synchronize()
        return [bits(r) for r in list(self.outputs) + list(extra)]

    def synchronised(self, name=None):
        """What the call gives with input `name` holding B (None: every input A), made after torch.cuda.synchronize()."""
        import torch
        if name not in self.want:
            self.reset()
            if name is not None:
                self.inputs[name].put("B")
                torch.cuda.synchronize()
            self.want[name] = self.results(self.call(None))
            if name is None:
                # (the call above paid for whatever a context sets up once: this one is timed)
                self.reset()
                t0 = time.perf_counter()
                extra = self.call(None)
                self.wall_ms = (time.perf_counter() - t0) * 1e3
                assert self.results(extra) == self.want[None], "the synchronised call gives two results on the same inputs"
        return self.want[name]


def bits(r):
    import torch
    if isinstance(r, torch.Tensor):
        return r.contiguous().view(torch.uint8).cpu().numpy().tobytes()
    return bytes(r)


def rgba(A, w, h, seed, depth=None):
    if depth is None:
        return A.synthetic_image(w, h, seed)
    return np.stack([A.synthetic_image(w, h, seed + 31 * z) for z in range(depth)])


class World:
    """Contexts, images and compressed chains the rows share.  Inputs (Buf) are restored to A by every case that uses them;
    everything else is written once, here."""

    def __init__(self, product, A, shift=0):
        import torch
        self.product, self.A = product, A
        self.rng = np.random.default_rng(11)
        self.ctxs = {}
        # (contexts nothing runs on: the streams of the others are made that many contexts later, see TWINS)
        self.spare = [self.ctx((4, 4, 1), A.PRE_FASTEST, fresh=True) for _ in range(shift)]
        self.side = torch.cuda.Stream()
        self.enc, self.strong = self.ctx((6, 6, 1), A.PRE_FASTEST), self.ctx((6, 6, 1), A.PRE_FAST)
        self.dec = self.ctx((6, 6, 1), A.PRE_FASTEST, flags=A.FLG_DECOMPRESS_ONLY)
        self.hdr = self.ctx((6, 6, 1), A.PRE_FASTEST, profile=A.PRF_HDR)
        self.enc3 = self.ctx((4, 4, 4), A.PRE_FASTEST)
        self.dec3 = self.ctx((4, 4, 4), A.PRE_FASTEST, flags=A.FLG_DECOMPRESS_ONLY)
        self.images = {k: rgba(A, 48, 48, s) for k, s in (("A", 1), ("B", 2))}
        self.small = torch.from_numpy(rgba(A, 24, 24, 3)).cuda()
        self.faces = {k: rgba(A, 24, 24, s, depth=6) for k, s in (("A", 4), ("B", 5))}
        self.volumes = {k: rgba(A, 24, 24, s, depth=8) for k, s in (("A", 6), ("B", 7))}
        # compressed chains of both contents: per level (dims, {content: bytes})
        self.chain2d = self.chains(self.enc, {k: v[None] for k, v in self.images.items()}, A.MIP_VOLUME)
        self.chain_cube = self.chains(self.enc, self.faces, A.MIP_ARRAY)
        self.chain_volume = self.chains(self.enc3, self.volumes, A.MIP_VOLUME)

    def ctx(self, block, quality, profile=None, flags=0, fresh=False):
        A = self.A
        key = (block, quality, profile, flags, len(self.ctxs) if fresh else None)
        if key not in self.ctxs:
            err, cfg = self.product.config_init(A.PRF_LDR if profile is None else profile, block[0], block[1], block[2], quality, flags)
            assert err == 0, self.product.error_string(err)
            err, ctx = self.product.context_alloc(cfg, 1)
            assert err == 0, self.product.error_string(err)
            self.ctxs[key] = ctx
        return self.ctxs[key]

    def chains(self, ctx, images, kind):
        import torch
        levels = None
        for k, img in images.items():
            torch.cuda.synchronize()
            tensors, blocks = self.product.compress_mip_chain_volume_device(ctx, torch.from_numpy(img).cuda(), kind, LEVELS)
            torch.cuda.synchronize()
            assert len(blocks) == LEVELS
            if levels is None:
                levels = [((t.shape[2], t.shape[1], t.shape[0]), {}, {}) for t in tensors]
            for l in range(LEVELS):
                levels[l][1][k] = blocks[l].cpu().numpy()
                levels[l][2][k] = tensors[l].cpu().numpy()
        return levels

    # what rows are made of
    def image(self, leading=False):
        a, b = self.images["A"], self.images["B"]
        return Buf(a[None], b[None]) if leading else Buf(a, b)

    def blocks(self, chain, level=0):
        return Buf(chain[level][1]["A"], chain[level][1]["B"])

    def fixed(self, array):
        import torch
        return torch.from_numpy(np.ascontiguousarray(array)).cuda()

    def entries(self, chain, first, data_type=None):
        """(ImageSetEntry per level without an image, the tensors they point to): level 0's blocks are `first`.t."""
        A = self.A
        held = [first.t] + [self.fixed(chain[l][1]["A"]) for l in range(1, LEVELS)]
        return [A.compressed_entry(t, chain[l][0], A.TYPE_U8 if data_type is None else data_type) for l, t in enumerate(held)], held

    def points(self, n, lo, hi):
        """[9, 33, n] float32 in lo .. hi, and the same mirrored."""
        a = self.rng.uniform(lo, hi, size=(GRID[1], GRID[0], n)).astype(np.float32)
        return Buf(a, (np.float32(lo + hi) - a).astype(np.float32))

    def lods(self):
        a = self.rng.uniform(0.0, LEVELS - 0.5, size=(GRID[1], GRID[0])).astype(np.float32)
        return Buf(a, (np.float32(LEVELS - 0.5) - a).astype(np.float32))

    def records(self, blocks):
        """[blocks, 4] float64 squared errors, about half of them above the criterion of `criterion`."""
        return Buf(*[np.random.default_rng(s).uniform(0.0, 36.0 * 0.5, size=(blocks, 4)) for s in (21, 22)])

    def criterion(self):
        return self.A.block_criterion(1.0)

    def out(self, shape, dtype):
        import torch
        return torch.empty(shape, dtype=dtype, device="cuda")

    def fmt(self):
        A = self.A
        return A.tensor_format(A.TENSOR_F32, A.TENSOR_PLANAR, 3, (2.0, 0.5, 1.5), (0.25, -1.0, 0.0))


def ok(w, err):
    assert err == 0, w.product.error_string(err)


# ---- the rows: name -> (inputs, caller owns the outputs, builder).  A builder returns the Row; its inputs are those named.

def row_compress_images(w):
    import torch
    img = w.image()
    outs = [w.out(64 * 16, torch.uint8), w.out(16 * 16, torch.uint8)]

    def call(stream):
        ok(w, w.product.compress_images_device(w.enc, [(img.t, outs[0]), (w.small, outs[1])], stream))
        return []
    return Row({"image": img}, outs, call)


def row_decompress_images(w):
    import torch
    blocks, out = w.blocks(w.chain2d), w.out((48, 48, 4), torch.uint8)

    def call(stream):
        ok(w, w.product.decompress_images_device(w.dec, [(out, blocks.t)], stream))
        return []
    return Row({"blocks": blocks}, [out], call)


def row_decompress_regions(w):
    import torch
    A = w.A
    blocks, out = w.blocks(w.chain2d), w.out((20, 30, 4), torch.uint8)
    entry = A.compressed_entry(blocks.t, (48, 48), A.TYPE_U8)

    def call(stream):
        ok(w, w.product.decompress_regions_device(w.dec, [entry], [(0, (5, 7, 0), (30, 20, 1), out)], stream))
        return []
    return Row({"blocks": blocks}, [out], call)


def row_decompress_tensors(w):
    import torch
    A = w.A
    blocks, out = w.blocks(w.chain2d), w.out((3, 20, 30), torch.float32)
    entry = A.compressed_entry(blocks.t, (48, 48), A.TYPE_U8)

    def call(stream):
        ok(w, w.product.decompress_tensors_device(w.dec, [entry], w.fmt(), [(0, (5, 7, 0), (30, 20, 1), out, True)], stream))
        return []
    return Row({"blocks": blocks}, [out], call)


def row_decompress_scaled_tensors(w):
    import torch
    A = w.A
    blocks, out = w.blocks(w.chain2d), w.out((3, GRID[1], GRID[0]), torch.float32)
    entry = A.compressed_entry(blocks.t, (48, 48), A.TYPE_U8)

    def call(stream):
        ok(w, w.product.decompress_scaled_tensors_device(w.dec, [entry], w.fmt(), A.WINDOW_BILINEAR, [(0, (3, 5, 0), (30, 8), out)], stream))
        return []
    return Row({"blocks": blocks}, [out], call)


def row_sample_tensors(w):
    import torch
    A = w.A
    blocks, coords, out = w.blocks(w.chain2d), w.points(2, -4.0, 52.0), w.out((3, GRID[1], GRID[0]), torch.float32)
    entry = A.compressed_entry(blocks.t, (48, 48), A.TYPE_U8)

    def call(stream):
        ok(w, w.product.sample_tensors_device(w.dec, [entry], w.fmt(), (A.SAMPLE_BILINEAR, A.ADDRESS_REPEAT, A.ADDRESS_MIRROR), [(0, 0, coords.t, out)], stream))
        return []
    return Row({"blocks": blocks, "coords": coords}, [out], call)


LOD_SAMPLER = (1, 1, 0, 1)      # bilinear, repeat, clamp, linear between levels


def row_sample_lod_tensors(w):
    import torch
    blocks, coords, lod, out = w.blocks(w.chain2d), w.points(2, -0.25, 1.25), w.lods(), w.out((3, GRID[1], GRID[0]), torch.float32)
    entries, held = w.entries(w.chain2d, blocks)

    def call(stream, held=held):
        ok(w, w.product.sample_lod_tensors_device(w.dec, entries, w.fmt(), LOD_SAMPLER, [(0, LEVELS, 0, coords.t, lod.t, out, 0.25)], stream))
        return []
    return Row({"blocks": blocks, "coords": coords, "lod": lod}, [out], call)


def row_sample_lod_grad(w):
    import torch
    blocks, coords, lod = w.blocks(w.chain2d), w.points(2, -0.25, 1.25), w.lods()
    grad_out = Buf(*[np.random.default_rng(s).normal(0.0, 2.0, size=(3, GRID[1], GRID[0])).astype(np.float32) for s in (31, 32)])
    grad_coords, grad_lod = w.out((GRID[1], GRID[0], 2), torch.float32), w.out((GRID[1], GRID[0]), torch.float32)
    entries, held = w.entries(w.chain2d, blocks)

    def call(stream, held=held):
        ok(w, w.product.sample_lod_grad_device(w.dec, entries, w.fmt(), LOD_SAMPLER, [(0, LEVELS, 0, coords.t, lod.t, grad_out.t, grad_coords, grad_lod, 0.25)], stream))
        return []
    return Row({"blocks": blocks, "coords": coords, "lod": lod, "grad_out": grad_out}, [grad_coords, grad_lod], call)


def row_sample_cube_tensors(w):
    import torch
    A = w.A
    blocks, lod, out = w.blocks(w.chain_cube), w.lods(), w.out((3, GRID[1], GRID[0]), torch.float32)
    a = w.rng.normal(0.0, 1.0, size=(GRID[1], GRID[0], 3)).astype(np.float32)
    dirs = Buf(a, -a)
    entries, held = w.entries(w.chain_cube, blocks)

    def call(stream, held=held):
        ok(w, w.product.sample_cube_tensors_device(w.dec, entries, w.fmt(), (A.SAMPLE_BILINEAR, A.MIP_LINEAR), [(0, LEVELS, 0, dirs.t, lod.t, out, 0.25)], stream))
        return []
    return Row({"blocks": blocks, "dirs": dirs, "lod": lod}, [out], call)


def row_sample_volume_tensors(w):
    import torch
    A = w.A
    blocks, coords, lod, out = w.blocks(w.chain_volume), w.points(3, -0.25, 1.25), w.lods(), w.out((3, GRID[1], GRID[0]), torch.float32)
    entries, held = w.entries(w.chain_volume, blocks)
    sampler = (A.SAMPLE_BILINEAR, A.ADDRESS_REPEAT, A.ADDRESS_CLAMP, A.ADDRESS_MIRROR, A.MIP_LINEAR)

    def call(stream, held=held):
        ok(w, w.product.sample_volume_tensors_device(w.dec3, entries, w.fmt(), sampler, [(0, LEVELS, coords.t, lod.t, out, 0.25)], stream))
        return []
    return Row({"blocks": blocks, "coords": coords, "lod": lod}, [out], call)


def row_compare_blocks(w):
    import torch
    blocks, img, errors = w.blocks(w.chain2d), w.image(), w.out((64, 4), torch.float64)

    def call(stream):
        err, sums = w.product.compare_blocks_device(w.enc, blocks.t, img.t, block_errors=errors, stream=stream)
        ok(w, err)
        return [sums]
    return Row({"blocks": blocks, "image": img}, [errors], call)


def row_compare_blocks_hdr(w):
    import torch
    halves = [(w.images[k].astype(np.float32) / np.float32(255.0) * np.float32(3.0)).astype(np.float16) for k in ("A", "B")]
    blocks, img, errors = w.blocks(w.chain2d), Buf(*halves), w.out((64, 4), torch.float64)

    def call(stream):
        err, sums, hdr = w.product.compare_blocks_hdr_device(w.hdr, blocks.t, img.t, -2, 3, block_errors=errors, stream=stream)
        ok(w, err)
        return [sums, hdr]
    return Row({"blocks": blocks, "image": img}, [errors], call)


def row_compress_block_list(w):
    import torch
    img, out = w.image(), w.out(64 * 16, torch.uint8)
    listed = Buf(np.arange(0, 64, 2, dtype=np.int32), np.arange(1, 64, 2, dtype=np.int32))

    def call(stream):
        ok(w, w.product.compress_block_list_device(w.enc, img.t, listed.t, out, stream=stream))
        return []
    return Row({"image": img, "block_list": listed}, [out], call)


def row_select_blocks(w):
    import torch
    records, listed = w.records(64), w.out(64, torch.int32)

    def call(stream):
        err, count = w.product.select_blocks_device(w.enc, records.t, (48, 48, 1), w.criterion(), listed, stream)
        ok(w, err)
        return [b"%d" % count]
    return Row({"block_errors": records}, [listed], call)


def row_compress_image_adaptive(w):
    import torch
    A = w.A
    img, out, errors = w.image(), w.out(64 * 16, torch.uint8), w.out((64, 4), torch.float64)

    def call(stream):
        err, stats = w.product.compress_image_adaptive_device(w.enc, w.strong, img.t, A.block_criterion(0.0), out, block_errors=errors, stream=stream)
        ok(w, err)
        return [b"%d %d %d" % (stats.blocks, stats.selected, stats.replaced)]
    return Row({"image": img}, [out, errors], call)


SET_DIMS = [(48, 48, 1), (24, 24, 1), (12, 12, 1)]      # 64 + 16 + 4 blocks at 6x6


def row_select_blocks_set(w):
    import torch
    records, listed = w.records(84), w.out(84, torch.int32)

    def call(stream):
        err, candidates, count = w.product.select_blocks_set_device(w.enc, SET_DIMS, records.t, w.criterion(), listed, 40, stream)
        ok(w, err)
        return [b"%d %d" % (candidates, count)]
    return Row({"block_errors": records}, [listed], call)


def row_compress_block_list_set(w):
    import torch
    img = w.image()
    levels = [img.t] + [w.fixed(w.chain2d[l][2]["A"][0]) for l in range(1, LEVELS)]
    outs = [w.out(n * 16, torch.uint8) for n in (64, 16, 4)]
    listed = Buf(np.arange(0, 84, 2, dtype=np.int32), np.arange(1, 84, 2, dtype=np.int32))

    def call(stream):
        ok(w, w.product.compress_block_list_set_device(w.enc, list(zip(levels, outs)), listed.t, stream=stream))
        return []
    return Row({"image": img, "block_list": listed}, outs, call)


def row_compress_images_adaptive(w):
    import torch
    A = w.A
    img = w.image()
    outs, errors = [w.out(64 * 16, torch.uint8), w.out(16 * 16, torch.uint8)], w.out((80, 4), torch.float64)

    def call(stream):
        err, stats = w.product.compress_images_adaptive_device(w.enc, w.strong, [(img.t, outs[0]), (w.small, outs[1])], A.block_criterion(0.0), 24,
                                                               block_errors=errors, stream=stream)
        ok(w, err)
        return [b"%d %d %d %d" % (stats.blocks, stats.candidates, stats.selected, stats.replaced)]
    return Row({"image": img}, outs + [errors], call)


def row_compare_image_set(w):
    import torch
    img, blocks, errors = w.image(), w.blocks(w.chain2d), w.out((80, 4), torch.float64)
    small_blocks = w.fixed(w.chain2d[1][1]["A"])

    def call(stream):
        err, sums = w.product.compare_image_set_device(w.enc, [(img.t, blocks.t), (w.small, small_blocks)], errors, stream)
        ok(w, err)
        return sums
    return Row({"image": img, "blocks": blocks}, [errors], call)


def chain_row(method, volume, **options):
    """A row of a mip chain wrapper: it allocates its outputs itself and returns them."""
    def build(w):
        img = Buf(w.volumes["A"], w.volumes["B"]) if volume else w.image()
        ctx = w.enc3 if volume else w.enc

        def call(stream):
            got = getattr(w.product, method)(ctx, img.t, levels=LEVELS, stream=stream, **options)
            tensors, blocks = got if isinstance(got, tuple) else (got, [])
            assert len(tensors) == LEVELS
            return list(tensors[1:]) + list(blocks)
        return Row({"image": img}, [], call)
    return build


def row_resize_image(w):
    img = w.image(leading=True)

    def call(stream):
        return [w.product.resize_image_device(w.enc, img.t, GRID, stream=stream)]
    return Row({"image": img}, [], call)


def row_raw_compress_image(w):
    import torch
    A = w.A
    img, out = w.image(), w.out(64 * 16, torch.uint8)

    def call(stream):
        ok(w, w.product.lib.astcenc_amd_compress_image_device(w.enc, img.t.data_ptr(), 48, 48, A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                              A.torch_stream(stream), None))
        return []
    return Row({"image": img}, [out], call)


def row_raw_decompress_image(w):
    import torch
    A = w.A
    blocks, out = w.blocks(w.chain2d), w.out((48, 48, 4), torch.uint8)

    def call(stream):
        ok(w, w.product.lib.astcenc_amd_decompress_image_device(w.dec, blocks.t.data_ptr(), blocks.t.numel(), out.data_ptr(), 48, 48, 1, A.TYPE_U8,
                                                                C.byref(A.Swizzle(*A.SWZ_RGBA)), A.torch_stream(stream)))
        return []
    return Row({"blocks": blocks}, [out], call)


def row_raw_compress_volume(w):
    import torch
    A = w.A
    vol, out = Buf(w.volumes["A"], w.volumes["B"]), w.out(6 * 6 * 2 * 16, torch.uint8)

    def call(stream):
        ok(w, w.product.lib.astcenc_amd_compress_volume_device(w.enc3, vol.t.data_ptr(), 24, 24, 8, A.TYPE_U8, C.byref(A.Swizzle(*A.SWZ_RGBA)), out.data_ptr(), out.numel(),
                                                               A.torch_stream(stream), None))
        return []
    return Row({"image": vol}, [out], call)


def row_raw_compare_images_hdr(w):
    A = w.A
    halves = [(rgba(A, 48, 48, s).astype(np.float32) / np.float32(255.0) * np.float32(3.0)).astype(np.float16) for s in (1, 2, 8, 9)]
    one, two = Buf(halves[0], halves[1]), Buf(halves[2], halves[3])

    def call(stream):
        sums, hdr = A.ErrorSums(), A.HdrErrorSums()
        ok(w, w.product.lib.astcenc_amd_compare_images_hdr_device(w.hdr, one.t.data_ptr(), A.TYPE_F16, two.t.data_ptr(), A.TYPE_F16, 48, 48, 1, -2, 3,
                                                                  A.torch_stream(stream), C.byref(sums), C.byref(hdr)))
        return [sums, hdr]
    return Row({"image": one, "image2": two}, [], call)


def row_compress_mip_chain_adaptive(w):
    """The driver that composes the weighted generation and the adaptive set call: it allocates what it writes."""
    A = w.A
    img = w.image(leading=True)

    def call(stream):
        tensors, blocks, stats = w.product.compress_mip_chain_adaptive(w.enc, w.strong, img.t, A.block_criterion(0.0), 24, levels=LEVELS, stream=stream)
        assert len(tensors) == LEVELS
        return list(tensors[1:]) + list(blocks) + [b"%d %d %d %d" % (stats.blocks, stats.candidates, stats.selected, stats.replaced)]
    return Row({"image": img}, [], call)


def row_raw_compare_images(w):
    A = w.A
    one, two = w.image(), Buf(rgba(A, 48, 48, 8), rgba(A, 48, 48, 9))

    def call(stream):
        sums = A.ErrorSums()
        ok(w, w.product.lib.astcenc_amd_compare_images_device(w.enc, one.t.data_ptr(), A.TYPE_U8, two.t.data_ptr(), A.TYPE_U8, 48, 48, 1, A.torch_stream(stream), C.byref(sums)))
        return [sums]
    return Row({"image": one, "image2": two}, [], call)


# name -> (inputs, the caller owns device outputs, the call leaves device results, builder)
TABLE = {
    "compress_images_device": (("image",), True, True, row_compress_images),
    "decompress_images_device": (("blocks",), True, True, row_decompress_images),
    "decompress_regions_device": (("blocks",), True, True, row_decompress_regions),
    "decompress_tensors_device": (("blocks",), True, True, row_decompress_tensors),
    "decompress_scaled_tensors_device": (("blocks",), True, True, row_decompress_scaled_tensors),
    "sample_tensors_device": (("blocks", "coords"), True, True, row_sample_tensors),
    "sample_lod_tensors_device": (("blocks", "coords", "lod"), True, True, row_sample_lod_tensors),
    "sample_lod_grad_device": (("blocks", "coords", "lod", "grad_out"), True, True, row_sample_lod_grad),
    "sample_cube_tensors_device": (("blocks", "dirs", "lod"), True, True, row_sample_cube_tensors),
    "sample_volume_tensors_device": (("blocks", "coords", "lod"), True, True, row_sample_volume_tensors),
    "compare_blocks_device": (("blocks", "image"), True, True, row_compare_blocks),
    "compare_blocks_hdr_device": (("blocks", "image"), True, True, row_compare_blocks_hdr),
    "compress_block_list_device": (("image", "block_list"), True, True, row_compress_block_list),
    "select_blocks_device": (("block_errors",), True, True, row_select_blocks),
    "compress_image_adaptive_device": (("image",), True, True, row_compress_image_adaptive),
    "select_blocks_set_device": (("block_errors",), True, True, row_select_blocks_set),
    "compress_block_list_set_device": (("image", "block_list"), True, True, row_compress_block_list_set),
    "compress_images_adaptive_device": (("image",), True, True, row_compress_images_adaptive),
    "compare_image_set_device": (("image", "blocks"), True, True, row_compare_image_set),
    # (the mip chain and resize wrappers allocate what they write: no caller's fill can be pending on it)
    "generate_mip_chain_device": (("image",), False, True, chain_row("generate_mip_chain_device", False)),
    "compress_mip_chain_device": (("image",), False, True, chain_row("compress_mip_chain_device", False)),
    "generate_mip_chain_volume_device": (("image",), False, True, chain_row("generate_mip_chain_volume_device", True)),
    "compress_mip_chain_volume_device": (("image",), False, True, chain_row("compress_mip_chain_volume_device", True)),
    "generate_mip_chain_ex_device": (("image",), False, True, chain_row("generate_mip_chain_ex_device", True, options=(2, 0.5))),
    "compress_mip_chain_ex_device": (("image",), False, True, chain_row("compress_mip_chain_ex_device", True, options=(2, 0.5))),
    "generate_mip_chain_filtered_device": (("image",), False, True, chain_row("generate_mip_chain_filtered_device", True, mip_filter=(1, 0))),
    "compress_mip_chain_filtered_device": (("image",), False, True, chain_row("compress_mip_chain_filtered_device", True, mip_filter=(1, 0))),
    "generate_mip_chain_weighted_device": (("image",), False, True, chain_row("generate_mip_chain_weighted_device", True, mip_filter=(1, 0), weighting=1)),
    "compress_mip_chain_weighted_device": (("image",), False, True, chain_row("compress_mip_chain_weighted_device", True, mip_filter=(1, 0), weighting=1)),
    "resize_image_device": (("image",), False, True, row_resize_image),
    "compress_mip_chain_adaptive": (("image",), False, True, row_compress_mip_chain_adaptive),
    "astcenc_amd_compress_image_device": (("image",), True, True, row_raw_compress_image),
    "astcenc_amd_decompress_image_device": (("blocks",), True, True, row_raw_decompress_image),
    "astcenc_amd_compress_volume_device": (("image",), True, True, row_raw_compress_volume),
    # (their only results are the sums on the host)
    "astcenc_amd_compare_images_device": (("image", "image2"), False, False, row_raw_compare_images),
    "astcenc_amd_compare_images_hdr_device": (("image", "image2"), False, False, row_raw_compare_images_hdr),
}

# Whether a call with a NULL hip_stream overtakes torch's default stream depends on which hardware queue the runtime gave the
# context's stream: streams that share one run in order by accident (the runtime deals its few queues out in turn).  Every case
# therefore runs twice, on two sets of contexts made one context apart, and has to hold on both.
# (profiles/stream_order/parent_vs_fix.txt: what one set alone missed.  The sets are shared by all cases and live as long as the
# session does.)
TWINS = 2
_WORLDS, _ROWS = {}, {}


def world(product, A, twin):
    if twin not in _WORLDS:
        import torch
        # the premise of the whole file: torch's default stream is the legacy null stream, whose handle a NULL hip_stream equals
        assert torch.cuda.default_stream().cuda_stream == 0
        _WORLDS[twin] = World(product, A, shift=twin)
    return _WORLDS[twin]


def row_of(product, A, name, twin):
    if (name, twin) not in _ROWS:
        inputs, owns, _, build = TABLE[name]
        row = build(world(product, A, twin))
        assert tuple(row.inputs) == inputs and bool(row.outputs) == owns, name
        _ROWS[name, twin] = row
    return _ROWS[name, twin]


def test_table_has_every_device_call(A):
    """A row for every method of Library that takes a stream, and for every exported call with a hip_stream that no such method
    reaches (read from the header), through ctypes."""
    import inspect
    import os
    import re
    methods = {n for n, f in vars(A.Library).items() if inspect.isfunction(f) and "stream" in inspect.signature(f).parameters}
    assert {n for n in vars(A.Library) if n.endswith("_device")} <= methods
    raw = {n for n in TABLE if n.startswith("astcenc_amd_")}
    assert methods == set(TABLE) - raw
    header = open(os.path.join(A.REPO, "include", "astcenc_amd.h")).read()
    exported = {m.group(1) for m in re.finditer(r"ASTCENC_PUBLIC enum astcenc_error (astcenc_amd_\w+)\(([^;]*)\);", header) if "hip_stream" in m.group(2)}
    source = inspect.getsource(A.Library)
    assert raw == {n for n in exported if "self.lib." + n + "(" not in source}


def in_mode(w, mode, queue, call):
    """Queues `queue()` on the mode's stream, makes `call(stream argument)`; returns (what call gave, the queued prefix in ms)."""
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def prefix():
        start.record()
        queue()
        end.record()
    if mode == "b":
        with torch.cuda.stream(w.side):
            prefix()
            got = call(None)
    else:
        prefix()
        if mode == "c":
            w.side.wait_stream(torch.cuda.default_stream())
        got = call(w.side if mode == "c" else None)
    torch.cuda.synchronize()
    return got, start.elapsed_time(end)


def check_delay(name, prefix_ms, wall_ms):
    print("%s: queued prefix %.2f ms, synchronised call %.3f ms, ratio %.1f" % (name, prefix_ms, wall_ms, prefix_ms / wall_ms))
    assert prefix_ms >= RATIO * wall_ms, "%s: the delay of %.2f ms is not %d times the call's %.3f ms: raise SLEEP_SCALE" % (name, prefix_ms, RATIO, wall_ms)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,which", [(n, i) for n, t in TABLE.items() for i in t[0]])
def test_inputs_arrive_in_time(product, A, name, which, mode):
    import torch
    for twin in range(TWINS):
        w, row = world(product, A, twin), row_of(product, A, name, twin)
        want_a, want_b = row.synchronised(), row.synchronised(which)
        assert want_a != want_b, "the call gives the same on both contents of %s: the case proves nothing" % which
        row.reset()
        buf = row.inputs[which]

        def queue():
            torch.cuda._sleep(SLEEP * SLEEP_SCALE.get(name, 1))
            buf.put("B")
        extra, prefix_ms = in_mode(w, mode, queue, row.call)
        got = row.results(extra)
        check_delay(name, prefix_ms, row.wall_ms)
        assert got != want_a, "the call read %s before the copy queued ahead of it had landed (contexts %d)" % (which, twin)
        assert got == want_b, "neither the old nor the new content of %s (contexts %d)" % (which, twin)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n, t in TABLE.items() if t[1]])
def test_outputs_are_not_overwritten(product, A, name, mode):
    import torch
    for twin in range(TWINS):
        w, row = world(product, A, twin), row_of(product, A, name, twin)
        want = row.synchronised()
        row.reset(fill=False)
        filled = [bytes([GUARD]) * (o.numel() * o.element_size()) for o in row.outputs]
        assert all(g != f for g, f in zip(want, filled)), "an output the call does not write"

        def queue():
            torch.cuda._sleep(SLEEP * SLEEP_SCALE.get(name, 1))
            row.fill()
        extra, prefix_ms = in_mode(w, mode, queue, row.call)
        got = row.results(extra)
        check_delay(name, prefix_ms, row.wall_ms)
        assert all(g != f for g, f in zip(got, filled)), "the guard fill queued ahead of the call landed over what it wrote (contexts %d)" % twin
        assert got == want, twin


@pytest.mark.parametrize("name", [n for n, t in TABLE.items() if t[2]])
def test_complete_on_return(product, A, name):
    """hip_stream NULL: what the call wrote is there for a stream that waits for nothing."""
    import torch
    for twin in range(TWINS):
        row = row_of(product, A, name, twin)
        want = row.synchronised()
        row.reset()
        extra = row.call(None)
        device = [r for r in list(row.outputs) + list(extra) if isinstance(r, torch.Tensor)]
        assert device
        fresh = torch.cuda.Stream()
        with torch.cuda.stream(fresh):
            held = [torch.empty(r.shape, dtype=r.dtype).pin_memory().copy_(r, non_blocking=True) for r in device]
        fresh.synchronize()
        wanted = [x for x, r in zip(want, list(row.outputs) + list(extra)) if isinstance(r, torch.Tensor)]
        assert [bits(h) for h in held] == wanted, twin


def test_autograd_function_under_the_default_stream(product, A):
    """sample_lod and its backward read what torch kernels queued behind sleeps are still to write."""
    import torch
    shape = (GRID[1], GRID[0])
    for twin in range(TWINS):
        w = world(product, A, twin)
        fmt = w.fmt()
        blocks = w.blocks(w.chain2d)
        entries, held = w.entries(w.chain2d, blocks)
        blocks.put("A")
        a_coords = w.fixed(w.rng.uniform(-0.25, 1.25, size=shape + (2,)).astype(np.float32))
        a_lod = w.fixed(w.rng.uniform(0.0, 1.0, size=shape).astype(np.float32))
        a_up = w.fixed(w.rng.normal(0.0, 1.0, size=(3,) + shape).astype(np.float32))

        def produce():
            return (a_coords * -1.0 + 1.0).requires_grad_(True), (a_lod * 1.5 + 0.25).requires_grad_(True)

        def through_autograd(coords, lod, upstream):
            """On synchronised tensors: (bits of the output and both gradients, the host's time for forward and backward)."""
            coords, lod = coords.clone().requires_grad_(True), lod.clone().requires_grad_(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = product.sample_lod(w.dec, entries, fmt, LOD_SAMPLER, 0, LEVELS, 0, coords, lod, lod_bias=0.25)
            gc, gl = torch.autograd.grad(out, (coords, lod), upstream)
            wall_ms = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()
            return [bits(t) for t in (out.detach(), gc, gl)], wall_ms

        def direct(coords, lod, upstream):
            out, gc, gl = w.out((3,) + shape, torch.float32), w.out(shape + (2,), torch.float32), w.out(shape, torch.float32)
            torch.cuda.synchronize()
            ok(w, product.sample_lod_tensors_device(w.dec, entries, fmt, LOD_SAMPLER, [(0, LEVELS, 0, coords, lod, out, 0.25)]))
            ok(w, product.sample_lod_grad_device(w.dec, entries, fmt, LOD_SAMPLER, [(0, LEVELS, 0, coords, lod, upstream, gc, gl, 0.25)]))
            torch.cuda.synchronize()
            return [bits(t) for t in (out, gc, gl)]

        # on the inputs A: what a stale read would give; the first pass pays for what torch and the context set up once (the
        # Function, the engine's thread), the second is how long the host takes over forward and backward
        through_autograd(a_coords, a_lod, a_up)
        other, wall_ms = through_autograd(a_coords, a_lod, a_up)
        assert other == direct(a_coords, a_lod, a_up)
        # (the blocks the allocator hands out next hold NaNs until the queued kernels have run)
        poison = [torch.full_like(t, float("nan")) for t in (a_coords, a_lod, a_up) for _ in range(8)]
        del poison
        torch.cuda.synchronize()
        start, mid, end = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        start.record()
        torch.cuda._sleep(SLEEP)
        coords, lod = produce()
        mid.record()
        out = product.sample_lod(w.dec, entries, fmt, LOD_SAMPLER, 0, LEVELS, 0, coords, lod, lod_bias=0.25)
        torch.cuda._sleep(SLEEP)
        upstream = a_up * 2.0 - 0.5
        end.record()
        gc, gl = torch.autograd.grad(out, (coords, lod), upstream)
        torch.cuda.synchronize()
        check_delay("sample_lod", min(start.elapsed_time(mid), mid.elapsed_time(end)), wall_ms)
        # the same tensors, materialised and synchronised, through the two calls
        want = direct(coords.detach().clone(), lod.detach().clone(), upstream.clone())
        assert all(x != y for x, y in zip(want, other)), "the calls give the same on A and on B: the case proves nothing"
        assert [bits(t) for t in (out.detach(), gc, gl)] == want, twin
