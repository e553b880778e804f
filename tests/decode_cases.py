# SPDX-License-Identifier: Apache-2.0
"""Shared by tests/test_decode_coverage_cpu.py and tests/test_decode_coverage.py: what the decoder is fed to show that it is
right for every legal encoding, not only for what an encoder of ours emits.

  pool(block)      a seeded pool of 128-bit blocks per footprint: the 11 mode bits from the modes the plain-C oracle
                   (oracle/astc_decode.c, astc_oracle_block_info) accepts for the footprint, the partition count uniform, the
                   format of a one-partition block balanced over 0..15, everything else random -- so the payload carries
                   trit and quint groups no encoder writes -- plus hand-steered blocks (void extents in the 2D / 3D layout,
                   reserved modes, four partitions with two planes, HDR formats) and top-ups steered at the cells and modes
                   the draw left short.  Every block keeps the oracle's BlockInfo; nothing here reads the product's tables.
  MATRIX / cells   the cells that must hold MIN_BLOCKS blocks per footprint, and every legal mode MIN_PER_MODE blocks;
                   NOT_REACHED lists the cells no block can be in, each with the format rule that forbids it.
  streams(block)   the pool laid out as images: block rows of two full runs of RUN blocks and a tail (1, 17, 31 blocks: one
                   stream each), the last block column and row clipped by the image's size.  A run is composed for one build
                   of decode_row_texels (csrc/wave_decode.h): `full` runs hold RUN payload blocks of at least FULL_MODES
                   distinct modes, `mixed` runs interleave payload, constant and error blocks.  Every stream comes shuffled too, and
                   one more stream holds the whole pool in its own order.
  run_build        which build a run selects, from oracle info alone.  It backs the coverage claim only: expected texels
                   always come from the reference decoder.

Not a conftest and not a test module: a plain module, imported by name.  As a program it prints the census files of
profiles/decode_coverage:

    python tests/decode_cases.py before        (the streams of the decode tests that were there before)
    python tests/decode_cases.py after         (the streams of this module)"""
import collections
import ctypes as C
import os
import sys

import numpy as np

import block_census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RUN = 32                # blocks a wave decodes together: DECODE_BATCH of the shipped build (csrc/wave_decode.h)
FULL_MODES = 24         # distinct (weight grid, planes, weight quant) in a full run
MIN_BLOCKS = 8          # per cell of the matrix
MIN_PER_MODE = 2        # per legal mode
CANDIDATES = 4000       # the seeded draw per footprint
SEARCH = 100000         # candidates of a directed search before a cell counts as not reached
TAILS = (1, 17, 31)

FOOTPRINTS_2D = [(4, 4), (6, 6), (8, 5), (12, 12)]                  # 4x4: the small-block hash; 12x12: 64-weight grids
FOOTPRINTS_3D = [(3, 3, 3), (4, 4, 4), (6, 6, 5), (6, 6, 6)]        # 3x3x3: the small-block hash
FOOTPRINTS = FOOTPRINTS_2D + FOOTPRINTS_3D

HDR_FORMATS = (2, 3, 7, 11, 14, 15)
NORMAL, VOID_LDR, VOID_FP16, ERROR = 0, 1, 2, 3


def block_id(block):
    return "x".join(str(v) for v in block)


def _bz(block):
    return block[2] if len(block) > 2 else 1


# ---- bits -------------------------------------------------------------------------------------------------------------------


def _put(v, off, n, x):
    mask = ((1 << n) - 1) << off
    return (v & ~mask) | ((x << off) & mask)


def _random_bits(rng):
    return int.from_bytes(rng.integers(0, 256, size=16, dtype=np.uint8).tobytes(), "little")


def _bytes(v):
    return v.to_bytes(16, "little")


def _infos(values, block):
    data = np.frombuffer(b"".join(_bytes(v) for v in values), dtype=np.uint8)
    return block_census.block_infos(data, block)


def mode_key(info):
    """What the issue calls a mode: weight grid, planes, weight quant."""
    return (info.weight_x, info.weight_y, info.weight_z, info.dual_plane, info.weight_quant)


_LEGAL = {}


def legal_modes(block):
    """{mode key: [the 11-bit mode values that decode to it]} of a footprint, by asking the oracle: one partition, format 0,
    each of the 2048 mode values."""
    block = tuple(block)
    if block not in _LEGAL:
        out = collections.OrderedDict()
        for mode, info in enumerate(_infos(list(range(2048)), block)):
            if info.kind == NORMAL:
                out.setdefault(mode_key(info), []).append(mode)
        _LEGAL[block] = out
    return _LEGAL[block]


# ---- the matrix -------------------------------------------------------------------------------------------------------------


def cells(info):
    """The matrix cells one block is in: block_census.features, with the partition count crossed with the planes and a
    format told apart by whether its block has one partition or more."""
    out = [f for f in block_census.features(info) if not f.startswith("format:") and not f.startswith("plane2:partitions:")]
    if info.kind != NORMAL:
        return out
    n = info.partition_count
    out.append("partitions:%d:planes:%d" % (n, 2 if info.dual_plane else 1))
    for f in sorted({info.format[i] for i in range(n)}):
        out.append("format:%d:%s" % (f, "single" if n == 1 else "multi"))
    return out


MATRIX = (["kind:" + k for k in block_census.KINDS] +
          ["partitions:%d:planes:%d" % (n, p) for n in (1, 2, 3, 4) for p in (1, 2)] +
          ["partitions:%d:%s" % (n, s) for n in (2, 3, 4) for s in ("same", "mixed")] +
          ["plane2:%d" % c for c in range(4)] +
          ["format:%d:%s" % (f, s) for f in range(16) for s in ("single", "multi")] +
          ["blue:%d:%s" % (f, s) for f in block_census.BLUE_FORMATS for s in ("on", "off")] +
          ["wq:%d" % q for q in range(12)] +
          ["cq:%d" % q for q in range(4, 21)])

# Cells no block is in: cell -> the format rule.  tests/test_decode_coverage_cpu.py runs the directed search of SEARCH
# candidates for each of them, per footprint, and fails when the oracle accepts one.
NOT_REACHED = {
    "partitions:4:planes:2": "four partitions with two weight planes is an illegal encoding (ASTC specification, block mode: "
                             "dual-plane mode is not available with four partitions); %d candidates with a legal two-plane mode and "
                             "partition bits 3 were all rejected by the oracle" % SEARCH,
}


_STEER_KEYS = {}


def _steer_keys(cell, block):
    """The legal modes a candidate for `cell` draws from."""
    if (cell, block) not in _STEER_KEYS:
        keys = list(legal_modes(block))
        name = cell.split(":")
        if name[0] == "partitions" and len(name) == 4:              # partitions:N:planes:P
            keys = [k for k in keys if k[3] == int(name[3]) - 1]
        elif name[0] == "wq":
            keys = [k for k in keys if k[4] == int(name[1])]
        elif name[0] == "plane2":
            keys = [k for k in keys if k[3] == 1]
        _STEER_KEYS[(cell, block)] = keys
    return _STEER_KEYS[(cell, block)]


def steer(cell, block, rng):
    """One candidate aimed at `cell`: random bits with a legal mode, and what of the cell the header states directly."""
    block = tuple(block)
    legal = legal_modes(block)
    keys = _steer_keys(cell, block)
    if not keys:
        return None
    v = _random_bits(rng)
    parts = int(rng.integers(0, 4))
    name = cell.split(":")
    if name[0] == "partitions":                                 # partitions:N:planes:P, partitions:N:same|mixed
        parts = int(name[1]) - 1
    elif name[0] == "format":
        parts = 0 if name[2] == "single" else int(rng.integers(1, 4))
    modes = legal[keys[int(rng.integers(0, len(keys)))]]
    v = _put(v, 0, 11, modes[int(rng.integers(0, len(modes)))])
    v = _put(v, 11, 2, parts)
    if name[0] == "partitions" and len(name) == 3:
        v = _put(v, 23, 2, 0 if name[2] == "same" else int(rng.integers(1, 4)))
    if name[0] == "format":
        f = int(name[1])
        if parts == 0:
            v = _put(v, 13, 4, f)
        elif rng.integers(0, 2):
            v = _put(v, 23, 6, f << 2)                          # every partition this format
        else:
            v = _put(v, 23, 2, int(rng.integers(1, 4)))
    return v


def directed_search(cell, block, want, seed=0, limit=SEARCH):
    """Up to `limit` steered candidates; returns (the first `want` blocks the oracle puts in `cell`, candidates tried)."""
    rng = np.random.default_rng([seed, FOOTPRINTS.index(tuple(block)), MATRIX.index(cell)])
    found, tried = [], 0
    while tried < limit and len(found) < want:
        batch = [steer(cell, block, rng) for _ in range(min(2000, limit - tried))]
        if batch[0] is None:
            return found, limit
        tried += len(batch)
        for v, info in zip(batch, _infos(batch, block)):
            if cell in cells(info) and len(found) < want:
                found.append((v, info))
    return found, tried


# ---- the pool ---------------------------------------------------------------------------------------------------------------

Entry = collections.namedtuple("Entry", "bits info origin")       # bits: the block's 16 bytes


def _void(block, fp16, coords, colour, reserved=3):
    """A void-extent block in the footprint's layout: 2D four 13-bit coordinates from bit 12 under two reserved bits, 3D six
    9-bit coordinates from bit 10."""
    v = 0x1FC | (0x200 if fp16 else 0)
    if _bz(block) > 1:
        for i, c in enumerate(coords[:6]):
            v = _put(v, 10 + 9 * i, 9, c)
    else:
        v = _put(v, 10, 2, reserved)
        for i, c in enumerate(coords[:4]):
            v = _put(v, 12 + 13 * i, 13, c)
    for i, c in enumerate(colour):
        v = _put(v, 64 + 16 * i, 16, int(c))
    return v


def _hand_steered(block, rng):
    """(bits, origin) of the blocks no draw is trusted with."""
    out = []
    three = _bz(block) > 1
    top = 0x1FF if three else 0x1FFF
    n = 6 if three else 4
    for fp16 in (False, True):
        tag = "void_fp16" if fp16 else "void_ldr"
        for i in range(10):
            if fp16:
                # finite halves of every size, and now and then an infinity or a NaN as the colour
                colour = [int(x) for x in rng.integers(0, 0x7C00, size=4)]
                colour[int(rng.integers(0, 4))] |= 0x8000 if i & 1 else 0
                if i >= 8:
                    colour[i - 8] = (0x7C00, 0x7E01)[i - 8]
            else:
                colour = [int(x) for x in rng.integers(0, 65536, size=4)]
            lo = [int(x) for x in rng.integers(0, top - 1, size=n // 2)]
            hi = [int(rng.integers(l + 1, top + 1)) for l in lo]
            ordered = [c for pair in zip(lo, hi) for c in pair]
            out.append((_void(block, fp16, ordered, colour), tag + ":ordered"))
            out.append((_void(block, fp16, [top] * n, colour), tag + ":all_ones"))
            axis = i % (n // 2)
            bad = list(ordered)
            bad[2 * axis + 1] = bad[2 * axis] - (i & 1) if bad[2 * axis] > 0 else 0          # max < min, and max == min
            bad[2 * axis] = max(bad[2 * axis], bad[2 * axis + 1])
            out.append((_void(block, fp16, bad, colour), tag + ":min_ge_max"))
            if not three and i < 3:
                out.append((_void(block, fp16, ordered, colour, reserved=i), tag + ":reserved_bits"))
    legal = legal_modes(block)
    taken = {m for modes in legal.values() for m in modes}
    reserved = [m for m in range(2048) if m not in taken and (m & 0x1FF) != 0x1FC]
    for m in rng.choice(reserved, size=16, replace=False):
        out.append((_put(_random_bits(rng), 0, 11, int(m)), "reserved_mode"))
    dual = [m for k, modes in legal.items() if k[3] for m in modes]
    for m in rng.choice(dual, size=12):
        out.append((_put(_put(_random_bits(rng), 0, 11, int(m)), 11, 2, 3), "four_partitions_two_planes"))
    # HDR formats on the shortest weight streams, so that the colour integers fit: one partition, and several of one format
    short = sorted(legal, key=lambda k: (k[0] * k[1] * k[2] * (2 if k[3] else 1), k[4]))[:24]
    for i in range(24):
        f = HDR_FORMATS[i % 6]
        v = _put(_random_bits(rng), 0, 11, legal[short[i]][0])
        if i < 12:
            v = _put(_put(v, 11, 2, 0), 13, 4, f)
        else:
            v = _put(_put(v, 11, 2, 1), 23, 6, f << 2)
        out.append((v, "hdr_format"))
    return out


class Pool:
    """The blocks of one footprint and what the oracle says of each."""

    def __init__(self, block):
        self.block = tuple(block)
        rng = np.random.default_rng([20240, FOOTPRINTS.index(self.block)])
        legal = legal_modes(self.block)
        modes = [m for ms in legal.values() for m in ms]
        order = rng.permutation(len(modes))
        values, origins = [], []
        singles = 0
        for i in range(CANDIDATES):
            v = _put(_random_bits(rng), 0, 11, modes[order[i % len(modes)]])
            parts = int(rng.integers(0, 4))
            v = _put(v, 11, 2, parts)
            if parts == 0:
                v = _put(v, 13, 4, singles % 16)
                singles += 1
            values.append(v)
            origins.append("draw")
        for v, origin in _hand_steered(self.block, rng):
            values.append(v)
            origins.append(origin)
        self.entries = [Entry(_bytes(v), info, o) for v, info, o in zip(values, _infos(values, self.block), origins)]
        self.topped_up = collections.OrderedDict()              # what the draw left short -> (blocks added, candidates tried)
        # every legal mode: reachable with one partition and format 0, whatever follows
        count = collections.Counter(mode_key(e.info) for e in self.entries if e.info.kind == NORMAL)
        for key, ms in legal.items():
            need = MIN_PER_MODE - count[key]
            if need > 0:
                add = [_put(_put(_put(_random_bits(rng), 0, 11, ms[j % len(ms)]), 11, 2, 0), 13, 4, 0) for j in range(need)]
                self.entries += [Entry(_bytes(v), info, "mode_top_up") for v, info in zip(add, _infos(add, self.block))]
                self.topped_up["mode:%s" % (key,)] = (need, need)
        count = self.cell_count()
        for cell in MATRIX:
            need = MIN_BLOCKS - count[cell]
            if need > 0 and cell not in NOT_REACHED:
                found, tried = directed_search(cell, self.block, need)
                self.entries += [Entry(_bytes(v), info, "cell_top_up") for v, info in found]
                self.topped_up[cell] = (len(found), tried)
        self.data = np.frombuffer(b"".join(e.bits for e in self.entries), dtype=np.uint8)

    def cell_count(self):
        count = collections.Counter()
        for e in self.entries:
            count.update(cells(e.info))
        return count

    def mode_count(self):
        return collections.Counter(mode_key(e.info) for e in self.entries if e.info.kind == NORMAL)


_POOLS = {}


def pool(block):
    block = tuple(block)
    if block not in _POOLS:
        _POOLS[block] = Pool(block)
    return _POOLS[block]


def describe(entry):
    """A block for a failure message: its hex, where it came from, and its features."""
    return "%s (%s; %s; mode %s)" % (entry.bits.hex(), entry.origin, " ".join(block_census.features(entry.info)),
                                     mode_key(entry.info) if entry.info.kind == NORMAL else None)


# ---- which build a run selects ------------------------------------------------------------------------------------------

PROFILES = ("PRF_LDR", "PRF_LDR_SRGB", "PRF_HDR", "PRF_HDR_RGB_LDR_A")
OUT_TYPES = (np.uint8, np.float16, np.float32)
SWIZZLES = collections.OrderedDict([("rgba", ("SWZ_R", "SWZ_G", "SWZ_B", "SWZ_A")), ("bgra", ("SWZ_B", "SWZ_G", "SWZ_R", "SWZ_A")),
                                    ("raz1", ("SWZ_R", "SWZ_A", "SWZ_Z", "SWZ_1"))])
BUILDS_2D = [(0, False, False), (0, True, False), (1, False, False), (1, True, False), (2, False, False), (2, True, False), (2, True, True)]
GENERAL = (2, True, True)


def hdr_profile(profile):
    return profile in ("PRF_HDR", "PRF_HDR_RGB_LDR_A")


def role(info, profile):
    """What a block is to the decoder in a profile: "payload", "constant" or "error" (an FP16 constant colour is legal in the
    HDR profiles only; an HDR endpoint format in an LDR profile is a payload block whose partition has the error colour)."""
    if info.kind == NORMAL:
        return "payload"
    if info.kind == VOID_LDR or (info.kind == VOID_FP16 and hdr_profile(profile)):
        return "constant"
    return "error"


def has_hdr_format(info):
    return info.kind == NORMAL and any(info.format[i] in HDR_FORMATS for i in range(info.partition_count))


def run_build(infos, profile, out_type, swizzle):
    """The build of decode_row_texels<kMulti, kDual, kGeneral> a run of 2D blocks selects, by the rule written above it in
    csrc/wave_decode.h.  kGeneral: some texel of the run does not leave as an RGBA8 pixel built from integers -- any output
    type but U8, or a payload block decoded through the Z swizzle or (in an HDR profile) from an HDR endpoint format; it
    comes with kMulti 2 and kDual.  Otherwise kMulti is 2 with a payload block of three or four partitions, 1 with one of
    two, else 0, and kDual says whether a payload block has two planes.  Constant and error blocks count for nothing."""
    payload = [i for i in infos if role(i, profile) == "payload"]
    if np.dtype(out_type) != np.dtype(np.uint8):
        return GENERAL
    if payload and ("SWZ_Z" in swizzle or (hdr_profile(profile) and any(has_hdr_format(i) for i in payload))):
        return GENERAL
    most = max([i.partition_count for i in payload] + [1])
    return (2 if most > 2 else 1 if most > 1 else 0, any(i.dual_plane for i in payload), False)


def run_kind(infos, profile):
    """"full": RUN payload blocks of at least FULL_MODES distinct modes; "mixed": payload, constant and error blocks together."""
    roles = [role(i, profile) for i in infos]
    if len(infos) == RUN and all(r == "payload" for r in roles) and len({mode_key(i) for i in infos}) >= FULL_MODES:
        return "full"
    if {"payload", "constant", "error"} <= set(roles):
        return "mixed"
    return "other"


def expected_builds(profile, out_type, swizzle):
    """The 2D builds the composed runs must reach, full and mixed, under one way of decoding them."""
    if np.dtype(out_type) != np.dtype(np.uint8) or "SWZ_Z" in swizzle:
        return [GENERAL]
    return BUILDS_2D if hdr_profile(profile) else BUILDS_2D[:6]


# ---- the run composer ---------------------------------------------------------------------------------------------------

# block categories: s one partition, d1 one partition two planes, p2 / p3 / p4 partitions, p2d / p3d with two planes;
# a bare name takes blocks whose formats are all LDR ones, "+h" blocks with an HDR format, "+*" either
_BASE = {"s": (1, 0), "d1": (1, 1), "p2": (2, 0), "p2d": (2, 1), "p3": (3, 0), "p3d": (3, 1), "p4": (4, 0)}

# 2D: one class per build (in an LDR profile, U8, no Z swizzle) and one of blocks with HDR formats, which is the general build
# in the HDR profiles.  A kDual class holds one-plane blocks too: they take another stride in that build.
CLASSES_2D = collections.OrderedDict([
    ("single", [("s", 32)]),
    ("dual", [("d1", 16), ("s", 16)]),
    ("two", [("p2", 20), ("s", 12)]),
    ("two_dual", [("p2", 10), ("p2d", 6), ("d1", 8), ("s", 8)]),
    ("many", [("p3", 10), ("p4", 10), ("p2", 6), ("s", 6)]),
    ("many_dual", [("p3", 6), ("p4", 6), ("p3d", 5), ("p2d", 5), ("d1", 5), ("p2", 2), ("s", 3)]),
    ("hdr", [("p3+h", 6), ("p4+h", 5), ("p3d+h", 4), ("p2d+h", 4), ("d1+h", 4), ("p2+h", 4), ("s+h", 5)]),
])
CLASS_BUILD = dict(zip(CLASSES_2D, BUILDS_2D))          # ("hdr": the general build, in an HDR profile)
# 3D: one build; the classes of block the issue names
CLASSES_3D = collections.OrderedDict([
    ("single", [("s+*", 32)]),
    ("dual", [("d1+*", 16), ("p2d+*", 8), ("p3d+*", 8)]),
    ("two", [("p2+*", 24), ("p2d+*", 8)]),
    ("many", [("p3+*", 12), ("p4+*", 12), ("p3d+*", 8)]),
])
RUNS_PER_CLASS = {2: 4, 3: 3}           # full runs, and as many mixed ones, per class (2D / 3D footprints)


def _category(p, name):
    base, _, formats = name.partition("+")
    parts, dual = _BASE[base]
    out = []
    for idx, e in enumerate(p.entries):
        i = e.info
        if i.kind != NORMAL or i.partition_count != parts or i.dual_plane != dual:
            continue
        if formats == "*" or (formats == "h") == has_hdr_format(i):
            out.append(idx)
    return out


def _take(p, rng, recipe, seen):
    """Block indices by a recipe [(category, count)], blocks of modes not yet in `seen` first."""
    out = []
    for name, count in recipe:
        have = _category(p, name)
        assert have, (p.block, name)
        have = [have[j] for j in rng.permutation(len(have))]
        picked = []
        for i in have:
            if len(picked) < count and mode_key(p.entries[i].info) not in seen:
                picked.append(i)
                seen.add(mode_key(p.entries[i].info))
        for i in have:
            if len(picked) < count and i not in picked:
                picked.append(i)
        while len(picked) < count:                               # (a category smaller than its share: some blocks twice)
            picked.append(have[int(rng.integers(0, len(have)))])
        out += picked
    return [out[j] for j in rng.permutation(len(out))]


def _full_run(p, rng, recipe):
    return _take(p, rng, recipe, set())


def _mixed_run(p, rng, recipe):
    """Twenty payload blocks in the recipe's proportions, six constant and six error blocks, interleaved."""
    scaled = [(name, max(1, (count * 20) // 32)) for name, count in recipe]
    short = 20 - sum(c for _, c in scaled)
    scaled[0] = (scaled[0][0], scaled[0][1] + short)
    payload = _take(p, rng, scaled, set())
    constant = [i for i, e in enumerate(p.entries) if e.info.kind == VOID_LDR]
    fp16 = [i for i, e in enumerate(p.entries) if e.info.kind == VOID_FP16]          # (constant in HDR profiles, error in LDR ones)
    error = [i for i, e in enumerate(p.entries) if e.info.kind == ERROR]
    other = ([constant[int(j)] for j in rng.integers(0, len(constant), size=4)] + [fp16[int(j)] for j in rng.integers(0, len(fp16), size=3)] +
             [error[int(j)] for j in rng.integers(0, len(error), size=5)])
    out = payload + other
    return [out[j] for j in rng.permutation(len(out))]


class Stream:
    """Blocks laid out as an image: `data` (read-only uint8), `index` the pool index of every block, dims (w, h, d)."""

    def __init__(self, name, p, index, blocks_xyz, labels):
        self.name, self.pool, self.block = name, p, p.block
        self.index = list(index)
        self.nbx, self.nby, self.nbz = blocks_xyz
        assert len(self.index) == self.nbx * self.nby * self.nbz
        bx, by, bz = self.block[0], self.block[1], _bz(self.block)
        # not multiples of the footprint: the last block column, row and layer are clipped
        self.dims = (self.nbx * bx - 1 - bx // 3, self.nby * by - by // 2, self.nbz * bz - bz // 2 if bz > 1 else 1)
        self.labels = labels                                    # per run, in order: (class, "full" | "mixed") or ("tail", "tail")
        self.data = np.frombuffer(b"".join(p.entries[i].bits for i in self.index), dtype=np.uint8)
        self.infos = [p.entries[i].info for i in self.index]

    def runs(self, first=0, last=None):
        """(block row, first block, infos) of every run the image decoder forms: RUN blocks from the start of each block row.
        first / last: the runs a window forms that covers block columns first..last of every row."""
        last = self.nbx - 1 if last is None else last
        out = []
        for row in range(self.nby * self.nbz):
            for b0 in range(first, last + 1, RUN):
                out.append((row, b0, self.infos[row * self.nbx + b0: row * self.nbx + min(b0 + RUN, last + 1)]))
        return out

    def build_census(self, profile, out_type, swizzle, first=0, last=None):
        """Counter of (build, kind) over the runs; 3D footprints have one build, "3d"."""
        count = collections.Counter()
        for _, _, infos in self.runs(first, last):
            build = run_build(infos, profile, out_type, swizzle) if _bz(self.block) == 1 else "3d"
            count[(build, run_kind(infos, profile))] += 1
        return count

    def entry_at(self, x, y, z=0):
        """The pool entry of the block that holds texel (x, y, z), its run's first block and that run's infos."""
        bx, by, bz = self.block[0], self.block[1], _bz(self.block)
        col, row = x // bx, (z // bz) * self.nby + y // by
        b0 = col - col % RUN
        return self.pool.entries[self.index[row * self.nbx + col]], b0, self.infos[row * self.nbx + b0: row * self.nbx + min(b0 + RUN, self.nbx)]


_STREAMS = {}


def streams(block):
    """The streams of a footprint: one per tail length, each followed by its shuffle, then the whole pool."""
    block = tuple(block)
    if block in _STREAMS:
        return _STREAMS[block]
    p = pool(block)
    rng = np.random.default_rng([77, FOOTPRINTS.index(block)])
    three = _bz(block) > 1
    classes = CLASSES_3D if three else CLASSES_2D
    runs = []
    for _ in range(RUNS_PER_CLASS[3 if three else 2]):
        runs += [((name, "full"), _full_run(p, rng, recipe)) for name, recipe in classes.items()]
        runs += [((name, "mixed"), _mixed_run(p, rng, recipe)) for name, recipe in classes.items()]
    # two full runs and a tail per block row; the runs are dealt to the three streams in turn, so each holds every class
    rows = len(runs) // 2
    share = [rows // 3 + (1 if t < rows % 3 else 0) for t in range(3)]
    if three:
        share = [4, 4, 4]
    out, at = [], 0
    for t, tail in enumerate(TAILS):
        index, labels = [], []
        for _ in range(share[t]):
            for label, run in runs[at:at + 2]:
                index += run
                labels.append(label)
            at += 2
            index += [int(j) for j in rng.integers(0, len(p.entries), size=tail)]
            labels.append(("tail", "tail"))
        shape = (2 * RUN + tail, 2, 2) if three else (2 * RUN + tail, share[t], 1)
        s = Stream("%s-tail%d" % (block_id(block), tail), p, index, shape, labels)
        order = rng.permutation(len(index))
        out += [s, Stream(s.name + "-shuffled", p, [index[j] for j in order], shape, None)]
    assert at == len(runs), (at, len(runs))
    # ... and the whole pool in its own order, so that no block of it goes undecoded (the last row filled up from the start)
    width = 2 * RUN + TAILS[1]
    rows = -(-len(p.entries) // width)
    rows += rows % 2 if three else 0
    index = [j % len(p.entries) for j in range(rows * width)]
    out.append(Stream("%s-pool" % block_id(block), p, index, (width, 2, rows // 2) if three else (width, rows, 1), None))
    _STREAMS[block] = out
    return out


def composed(block):
    """The streams as composed (not the shuffles)."""
    return [s for s in streams(block) if s.labels is not None]


# ---- decoding a stream through a library's astcenc_decompress_image ---------------------------------------------------------

_CONTEXTS = {}
_REFERENCE = {}


def _context(L, A, profile, block):
    key = (id(L), profile, tuple(block))
    if key not in _CONTEXTS:
        err, cfg = L.config_init(getattr(A, profile), block[0], block[1], _bz(block), A.PRE_MEDIUM, A.FLG_DECOMPRESS_ONLY)
        assert err == 0
        err, ctx = L.context_alloc(cfg, 1)
        assert err == 0, L.error_string(err)
        _CONTEXTS[key] = (L, ctx)                                # (kept for the session: a handful of contexts)
    return _CONTEXTS[key][1]


def swizzle_of(A, name):
    return tuple(getattr(A, s) for s in SWIZZLES[name])


def decode(L, A, stream, profile, out_type, swizzle):
    """[D, H, W, 4] of `out_type` (D = 1 for a 2D footprint): the stream through astcenc_decompress_image of library L."""
    w, h, d = stream.dims
    out = np.zeros((d, h, w, 4), dtype=out_type)
    dtype = {np.dtype(np.uint8): A.TYPE_U8, np.dtype(np.float16): A.TYPE_F16, np.dtype(np.float32): A.TYPE_F32}[out.dtype]
    slices = (C.c_void_p * d)(*[out[z].ctypes.data for z in range(d)])
    img = A.Image(w, h, d, dtype, slices)
    swz = A.Swizzle(*swizzle_of(A, swizzle))
    err = L.lib.astcenc_decompress_image(_context(L, A, profile, stream.block), stream.data.ctypes.data, stream.data.nbytes, C.byref(img), C.byref(swz), 0)
    assert err == 0, L.error_string(err)
    return out


def reference_decode(ref, A, stream, profile, out_type, swizzle, keep=True):
    """decode() through the reference, once per session and never changed."""
    key = (stream.name, profile, np.dtype(out_type).name, swizzle)
    if key in _REFERENCE:
        return _REFERENCE[key]
    out = decode(ref, A, stream, profile, out_type, swizzle)
    out.setflags(write=False)
    if keep:
        _REFERENCE[key] = out
    return out


def explain(stream, want, got, profile, out_type, swizzle):
    """None when the two decodes are bit-equal (NaN payloads included); else a message that names the first differing texel's
    block, its features and its run's build."""
    if want.shape == got.shape and want.tobytes() == got.tobytes():
        return None
    item = want.dtype.itemsize
    diff = np.argwhere((want.view(np.uint8).reshape(want.shape[:3] + (4 * item,)) != got.view(np.uint8).reshape(want.shape[:3] + (4 * item,))).any(axis=3))
    z, y, x = (int(v) for v in diff[0])
    entry, b0, infos = stream.entry_at(x, y, z)
    build = run_build(infos, profile, out_type, SWIZZLES[swizzle]) if _bz(stream.block) == 1 else "3d"
    return ("%s %s %s %s: %d texels differ, first at (x=%d, y=%d, z=%d): want %s got %s; block %s; its run starts at block %d, build %s" %
            (stream.name, profile, np.dtype(out_type).name, swizzle, len(diff), x, y, z, want[z, y, x], got[z, y, x], describe(entry), b0, build))


# ---- as a program: the census files --------------------------------------------------------------------------------------


def _census_lines(title, block, data, nbx, profile="PRF_LDR"):
    """Normal blocks, distinct modes and the runs per build (with their payload blocks) of one stream as the decoder cuts it."""
    infos = block_census.block_infos(data, block)
    normal = [i for i in infos if i.kind == NORMAL]
    lines = ["%-44s blocks %5d  normal %5d  modes %4d of %4d" % (title, len(infos), len(normal), len({mode_key(i) for i in normal}), len(legal_modes(block)))]
    per = collections.OrderedDict()
    for row in range(len(infos) // nbx):
        for b0 in range(0, nbx, RUN):
            run = infos[row * nbx + b0: row * nbx + min(b0 + RUN, nbx)]
            build = run_build(run, profile, np.uint8, SWIZZLES["rgba"]) if _bz(block) == 1 else "3d"
            per.setdefault(build, []).append(sum(1 for i in run if i.kind == NORMAL))
    for build, counts in sorted(per.items(), key=lambda kv: str(kv[0])):
        hist = collections.Counter(counts)
        lines.append("    build %-18s runs %4d  payload blocks per run: %s" % (build, len(counts), " ".join("%dx%d" % (hist[c], c) for c in sorted(hist))))
    return lines


def _before():
    """The streams of tests/test_decode.py and tests/test_volume.py as they stood: random bit patterns, and reference output."""
    import astcenc_amd as A
    import images
    import oracle_libs as O
    ref = A.Library(O.LIB_REF_NONE)
    lines = ["# the decode tests before tests/decode_cases.py: per stream the normal blocks, the distinct modes among them, and per build",
             "# of decode_row_texels (kMulti, kDual, kGeneral; PRF_LDR, U8, identity swizzle) its runs and their payload blocks as NxPAYLOAD", ""]
    lines.append("## test_decode_random_bit_patterns (the only stream that is not encoder output)")
    for block in [(4, 4), (6, 6), (8, 5), (12, 12)]:
        rng = np.random.default_rng(99 + block[0] + block[1])
        data = rng.integers(0, 256, size=48 * 32 * 16, dtype=np.uint8)
        blocks = data.reshape(-1, 16)
        blocks[::7, 0] = 0xFC
        blocks[::7, 1] |= 0x01
        blocks[::14, 1] = 0xFD
        blocks[::14, 2:8] = 0xFF
        blocks[::28, 1] = 0xFF
        blocks[1::5, 1] &= 0xE7
        lines += _census_lines(block_id(block), block, data, 48)
    lines += ["", "## test_decode_wide_images_in_full_runs (reference output at -medium, 71 blocks per row)"]
    for block in [(4, 4), (6, 6), (8, 8), (10, 5), (12, 12)]:
        w, h = block[0] * 70 + 3, block[1] * 2 + 1
        im = images.ALL["noisy"](w, h)
        im[: block[1], : 40 * block[0]] = (9, 200, 31, 255)
        lines += _census_lines(block_id(block), block, ref.compress(im, block, 60.0), 71)
    lines += ["", "## test_decode_ldr_matches_reference (reference output, six blocks per row: every run is a tail)"]
    for block in [(4, 4), (6, 6), (8, 5), (12, 12)]:
        w, h = block[0] * 5 + 2, block[1] * 4 + 3
        data = np.concatenate([ref.compress(images.ALL[n](w, h), block, q) for n, q in (("noisy", 60.0), ("two_colour", 98.0), ("flat", 10.0))])
        lines += _census_lines(block_id(block), block, data, 6)
    lines += ["", "## test_volume.py, test_decompress_and_block_info_match_reference: junk (36 random blocks, a third forced to void-extent) and -medium output"]
    for block in [(3, 3, 3), (4, 4, 3), (5, 5, 4), (6, 6, 6)]:
        d, h, w = 2 * block[2] + 1, 2 * block[1] + 1, 3 * block[0] + 2
        rng = np.random.default_rng(block[0] + 10 * block[2])
        legal = ref.compress(images.volume("edges", d, h, w), block, 60.0)
        junk = rng.integers(0, 256, 36 * 16, dtype=np.uint8)
        junk.reshape(-1, 16)[::3, 0] = 0xFC
        junk.reshape(-1, 16)[::3, 1] |= 0x01
        lines += _census_lines(block_id(block) + " junk", block, junk, 4)
        lines += _census_lines(block_id(block) + " edges -medium", block, legal, 4)
    return lines


def _after():
    lines = ["# tests/decode_cases.py: per footprint the pool's matrix, then per stream what census_before.txt shows", ""]
    for block in FOOTPRINTS:
        p = pool(block)
        count, modes = p.cell_count(), p.mode_count()
        lines.append("## %s: pool of %d blocks; %d legal modes, fewest blocks of one mode %d; topped up: %s" %
                     (block_id(block), len(p.entries), len(legal_modes(block)), min(modes[k] for k in legal_modes(block)),
                      ", ".join("%s +%d (%d tried)" % (k, v[0], v[1]) for k, v in p.topped_up.items() if not k.startswith("mode:")) or "nothing"))
        lines.append("   modes topped up: %d" % sum(1 for k in p.topped_up if k.startswith("mode:")))
        row = []
        for cell in MATRIX:
            row.append("%s=%d" % (cell, count[cell]))
        for i in range(0, len(row), 8):
            lines.append("   " + "  ".join(row[i:i + 8]))
        for s in streams(block):
            lines += _census_lines(s.name, block, s.data, s.nbx)
        if _bz(block) == 1:
            for profile, out_type, swz in (("PRF_LDR", np.uint8, "rgba"), ("PRF_HDR", np.uint8, "rgba"), ("PRF_LDR", np.uint8, "raz1"), ("PRF_LDR", np.float16, "rgba")):
                total = collections.Counter()
                for s in composed(block):
                    total.update(s.build_census(profile, out_type, SWIZZLES[swz]))
                lines.append("   %s %s %s: %s" % (profile, np.dtype(out_type).name, swz, "  ".join(
                    "%s full %d mixed %d" % (b, total[(b, "full")], total[(b, "mixed")]) for b in BUILDS_2D if total[(b, "full")] + total[(b, "mixed")] + total[(b, "other")])))
        lines.append("")
    return lines


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle")]
    sys.stdout.write("\n".join(_before() if sys.argv[1:] == ["before"] else _after()) + "\n")
