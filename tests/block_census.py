# SPDX-License-Identifier: Apache-2.0
"""Which encodings a stream of ASTC blocks holds: the header fields of every block (oracle/astc_decode.c,
astc_oracle_block_info: the decoder's own parse, nothing looked up) counted as features.  The coverage tests
(tests/test_encoding_coverage*.py) use it on the reference's bytes to show which arms of the search an image drives.

Not a conftest and not a test module: a plain module, imported by name.  Run as a program it prints the census of the
reference's output over the matrices of tools/gpu_sweep.py and tools/gpu_sweep_3d.py, per kernel build class, on the CPUs:

    python tests/block_census.py sweep [SIZE [EDGE]]          (SIZE 120, EDGE 24 by default)
    python tests/block_census.py cases                        (the images of tests/encoding_cases.py)

Features, each a string:
  kind:normal | kind:void_ldr | kind:void_fp16 | kind:error
  partitions:N                      N = 1..4
  partitions:N:same | :mixed        N >= 2: the partitions' endpoint formats are of one class (format >> 2) or not
  plane2:C                          two weight planes, the second on component C = 0..3
  plane2:partitions:N               two weight planes and N partitions
  format:F                          a partition with endpoint format F (counted once per block)
  blue:F:on | blue:F:off            F in 8, 9, 12, 13: a partition whose integers select / do not select blue contraction
  wq:Q                              weight quant level 0..11
  cq:Q                              colour quant level 4..20"""
import collections
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DECODE = os.path.join(ROOT, "oracle", "_build", "libastc_decode.so")

KINDS = ("normal", "void_ldr", "void_fp16", "error")
BLUE_FORMATS = (8, 9, 12, 13)


class BlockInfo(ctypes.Structure):
    """AstcOracleBlockInfo (oracle/astc_decode.c)."""
    _fields_ = [("kind", ctypes.c_int), ("partition_count", ctypes.c_int), ("dual_plane", ctypes.c_int),
                ("plane2_component", ctypes.c_int), ("weight_x", ctypes.c_int), ("weight_y", ctypes.c_int),
                ("weight_z", ctypes.c_int), ("weight_quant", ctypes.c_int), ("color_quant", ctypes.c_int),
                ("mixed_classes", ctypes.c_int), ("partition_seed", ctypes.c_int), ("format", ctypes.c_int * 4),
                ("blue_contraction", ctypes.c_int * 4)]


_lib = None


def library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_DECODE):
            subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "decode"])
        _lib = ctypes.CDLL(LIB_DECODE)
        _lib.astc_oracle_block_info.restype = ctypes.c_int
        _lib.astc_oracle_block_info.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(BlockInfo)]
    return _lib


def _footprint(block):
    return block[0], block[1], (block[2] if len(block) > 2 else 1)


def block_infos(blocks, block):
    """One BlockInfo per 16 bytes of `blocks`; block is (x, y) or (x, y, z)."""
    lib = library()
    bx, by, bz = _footprint(block)
    data = np.ascontiguousarray(np.asarray(blocks, dtype=np.uint8)).reshape(-1, 16)
    out = []
    for row in data:
        info = BlockInfo()
        lib.astc_oracle_block_info(row.ctypes.data, bx, by, bz, ctypes.byref(info))
        out.append(info)
    return out


def features(info):
    """The features (see the module's docstring) of one block."""
    out = ["kind:" + KINDS[info.kind]]
    if info.kind != 0:
        return out
    n = info.partition_count
    out.append("partitions:%d" % n)
    if n >= 2:
        out.append("partitions:%d:%s" % (n, "mixed" if info.mixed_classes else "same"))
    if info.dual_plane:
        out.append("plane2:%d" % info.plane2_component)
        out.append("plane2:partitions:%d" % n)
    formats = [info.format[i] for i in range(n)]
    for f in sorted(set(formats)):
        out.append("format:%d" % f)
    blue = {(formats[i], info.blue_contraction[i]) for i in range(n) if formats[i] in BLUE_FORMATS}
    for f, on in sorted(blue):
        out.append("blue:%d:%s" % (f, "on" if on else "off"))
    out.append("wq:%d" % info.weight_quant)
    out.append("cq:%d" % info.color_quant)
    return out


def census(blocks, block):
    """Counter of the features of every block of the stream."""
    count = collections.Counter()
    for info in block_infos(blocks, block):
        count.update(features(info))
    return count


def blocks_with(blocks, block, feature):
    """Indices of the blocks of the stream that have `feature`."""
    return [i for i, info in enumerate(block_infos(blocks, block)) if feature in features(info)]


def _key(feature):
    return [(0, int(p), "") if p.isdigit() else (1, 0, p) for p in feature.split(":")]


def format_census(per_class):
    """Text of {class name: Counter}: one line per feature, one column per class."""
    names = list(per_class)
    feats = sorted({f for c in per_class.values() for f in c}, key=_key)
    width = max([len(f) for f in feats] + [8])
    lines = ["%-*s %s" % (width, "feature", " ".join("%9s" % n for n in names))]
    lines.append("%-*s %s" % (width, "blocks", " ".join("%9d" % sum(v for f, v in per_class[n].items() if f.startswith("kind:")) for n in names)))
    for f in feats:
        lines.append("%-*s %s" % (width, f, " ".join("%9d" % per_class[n][f] for n in names)))
    return "\n".join(lines) + "\n"


# ---- as a program: the census of the sweep tools' matrices, and of the coverage images, reference only, on the CPUs -------


def _threaded_reference():
    import threading
    import astcenc_amd as A
    import oracle_libs as O
    ref = A.Library(O.LIB_REF_AVX2)          # (byte-identical to the scalar build by the reference's invariance mode)
    threads = min(16, len(os.sched_getaffinity(0)))

    def compress(img, block, quality, profile):
        bx, by, bz = _footprint(block)
        err, cfg = ref.config_init(profile, bx, by, bz, quality, 0)
        assert err == 0
        err, ctx = ref.context_alloc(cfg, threads)
        assert err == 0
        img = np.ascontiguousarray(img)
        d = img.shape[0] if img.ndim == 4 else 1
        h, w = img.shape[-3], img.shape[-2]
        out = np.zeros(((w + bx - 1) // bx) * ((h + by - 1) // by) * ((d + bz - 1) // bz) * 16, dtype=np.uint8)
        ts = [threading.Thread(target=lambda i=i: ref.compress_raw(ctx, img, out, thread_index=i)) for i in range(threads)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        ref.context_free(ctx)
        return out
    return A, compress


def sweep_census(size=120, edge=24):
    """{class: Counter} over the matrix of tools/gpu_sweep.py at `size` and of tools/gpu_sweep_3d.py at `edge`."""
    import encoding_cases as E
    import images
    A, compress = _threaded_reference()
    per_class = {name: collections.Counter() for name in E.CLASSES}

    def add(img, block, quality, profile):
        per_class[E.build_class(profile, block, quality)].update(census(compress(img, block, quality, profile), block))

    foot = [(4, 4), (5, 4), (5, 5), (6, 5), (6, 6), (8, 5), (8, 6), (8, 8), (10, 5), (10, 6), (10, 8), (10, 10), (12, 10), (12, 12)]
    presets = [0.0, 10.0, 60.0, 98.0]
    ldr = {"noisy": images.noisy(size, size - 7, 21), "random": images.random_u8(size - 5, size, 22), "two_colour": images.two_colour(size, size, 23),
           "gray": images.grayscale(size, size), "flat": images.flat_regions(size, size), "smooth": images.smooth(size, size)}
    for block in foot:
        for q in presets:
            for name, img in ldr.items():
                for profile in ((A.PRF_LDR, A.PRF_LDR_SRGB) if name == "noisy" else (A.PRF_LDR,)):
                    add(img, block, q, profile)
        for profile in (A.PRF_HDR, A.PRF_HDR_RGB_LDR_A):
            for name, img in images.hdr_variants(96, 90).items():
                add(img.astype(np.float16), block, 60.0, profile)
    for block in ((4, 4), (6, 6), (8, 8)):
        add(images.noisy(48, 48, 31), block, 100.0, A.PRF_LDR)
    foot3 = [(3, 3, 3), (4, 3, 3), (4, 4, 3), (4, 4, 4), (5, 4, 4), (5, 5, 4), (5, 5, 5), (6, 5, 5), (6, 6, 5), (6, 6, 6)]
    vols = {k: images.volume(k, edge - 3, edge, edge + 5, seed=40 + i) for i, k in enumerate(("noise", "grad", "edges", "alpha", "flat"))}
    for block in foot3:
        for q in presets:
            for vol in vols.values():
                add(vol, block, q, A.PRF_LDR)
    return per_class


def cases_census():
    """{class: Counter} over the images of tests/encoding_cases.py."""
    import encoding_cases as E
    A, compress = _threaded_reference()
    per_class = {name: collections.Counter() for name in E.CLASSES}
    for case in E.cases():
        per_class[case.build_class].update(census(compress(case.image(), case.block, case.quality, case.profile), case.block))
    return per_class


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle")]
    what = sys.argv[1] if len(sys.argv) > 1 else "sweep"
    if what == "sweep":
        size = int(sys.argv[2]) if len(sys.argv) > 2 else 120
        edge = int(sys.argv[3]) if len(sys.argv) > 3 else 24
        sys.stdout.write("# reference output over the matrices of tools/gpu_sweep.py (size %d) and tools/gpu_sweep_3d.py (edge %d)\n" % (size, edge))
        sys.stdout.write(format_census(sweep_census(size, edge)))
    else:
        sys.stdout.write("# reference output over the images of tests/encoding_cases.py\n")
        sys.stdout.write(format_census(cases_census()))
