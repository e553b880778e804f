# SPDX-License-Identifier: Apache-2.0
"""The decoder against every legal encoding (tests/decode_cases.py), on the CPUs: the pool's matrix and the composed runs are
what the module claims, from oracle info alone; the sequential build of the kernel source (decode_row_batch, csrc/wave_decode.h)
gives the reference decoder's texels bit for bit on every stream, for every profile, output type and three swizzles; its
astcenc_get_block_info gives the reference's bytes on the whole pool; and the plain-C oracle decoder agrees with both.  The
GPU side is tests/test_decode_coverage.py."""
import collections
import ctypes as C

import numpy as np
import pytest

import block_census
import decode_cases as D

IDS = [D.block_id(b) for b in D.FOOTPRINTS]
IDS_2D = [D.block_id(b) for b in D.FOOTPRINTS_2D]
IDS_3D = [D.block_id(b) for b in D.FOOTPRINTS_3D]


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_matrix_cells_and_legal_modes_are_filled(block):
    """MIN_BLOCKS blocks in every cell that is not listed as not reached, MIN_PER_MODE in every legal mode -- the legal modes
    asked of the oracle, the counts from its BlockInfo."""
    p = D.pool(block)
    assert len(p.entries) <= 1.15 * D.CANDIDATES, len(p.entries)
    infos = block_census.block_infos(p.data, block)                          # (classified again, from the bytes)
    assert [D.cells(i) for i in infos] == [D.cells(e.info) for e in p.entries]
    count = collections.Counter()
    for i in infos:
        count.update(D.cells(i))
    short = [(cell, count[cell]) for cell in D.MATRIX if cell not in D.NOT_REACHED and count[cell] < D.MIN_BLOCKS]
    assert not short, short
    legal = D.legal_modes(block)
    assert len(legal) > 100
    modes = collections.Counter(D.mode_key(i) for i in infos if i.kind == D.NORMAL)
    assert not [k for k in legal if modes[k] < D.MIN_PER_MODE]
    assert set(modes) <= set(legal), set(modes) - set(legal)                  # (no mode the one-partition query did not find)
    origins = collections.Counter(e.origin.split(":")[0] for e in p.entries)
    for origin in ("void_ldr", "void_fp16", "reserved_mode", "four_partitions_two_planes", "hdr_format"):
        assert origins[origin] >= D.MIN_BLOCKS, origins
    # the hand-steered blocks are what their names say
    for e in p.entries:
        what = e.origin.split(":")
        if what[0] in ("void_ldr", "void_fp16"):
            legal_void = what[1] in ("ordered", "all_ones")
            assert e.info.kind == ({"void_ldr": D.VOID_LDR, "void_fp16": D.VOID_FP16}[what[0]] if legal_void else D.ERROR), D.describe(e)
        elif what[0] in ("reserved_mode", "four_partitions_two_planes"):
            assert e.info.kind == D.ERROR, D.describe(e)


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_cells_listed_as_not_reached_are_rejected_by_the_oracle(block):
    """Every entry states a format rule, and a directed search of SEARCH candidates finds no block the oracle puts there."""
    for cell, cause in D.NOT_REACHED.items():
        assert cell in D.MATRIX and "illegal" in cause and str(D.SEARCH) in cause
        assert D.pool(block).cell_count()[cell] == 0
        found, tried = D.directed_search(cell, block, 1)
        assert tried >= 100000 and not found, (cell, tried, [hex(v) for v, _ in found])


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_rows_are_two_full_runs_and_a_tail(block):
    assert D.RUN == 32
    tails = set()
    for s in D.streams(block):
        assert s.nbx > 2 * D.RUN and s.nbx - 2 * D.RUN < D.RUN
        tails.add(s.nbx - 2 * D.RUN)
        bx, by, bz = block[0], block[1], (block[2] if len(block) > 2 else 1)
        w, h, d = s.dims
        assert w % bx and h % by and (bz == 1 or d % bz), s.dims                # clipped last column, row (and layer)
        assert (-(-w // bx), -(-h // by), -(-d // bz)) == (s.nbx, s.nby, s.nbz)
        assert s.data.nbytes == 16 * s.nbx * s.nby * s.nbz <= 16 * 1.15 * D.CANDIDATES
    assert tails == set(D.TAILS)
    names = [s.name for s in D.streams(block)]
    assert all(s.name + "-shuffled" in names for s in D.composed(block))
    pool_stream = D.streams(block)[-1]
    assert set(pool_stream.index) == set(range(len(D.pool(block).entries)))     # every block of the pool is decoded


@pytest.mark.parametrize("block", D.FOOTPRINTS_2D, ids=IDS_2D)
def test_every_2d_build_has_full_and_mixed_runs(block):
    """Per (profile, output type) and swizzle under test: each build that way of decoding can select has four full runs (RUN
    payload blocks, FULL_MODES distinct modes) and four mixed ones; over the ways together that is all seven builds."""
    reached = set()
    for profile in D.PROFILES:
        for out_type in D.OUT_TYPES:
            for swz in D.SWIZZLES:
                total = collections.Counter()
                for s in D.composed(block):
                    total.update(s.build_census(profile, out_type, D.SWIZZLES[swz]))
                expected = D.expected_builds(profile, out_type, D.SWIZZLES[swz])
                for build in expected:
                    assert total[(build, "full")] >= 4 and total[(build, "mixed")] >= 4, (profile, out_type.__name__, swz, build, total)
                reached |= set(expected)
    assert reached == set(D.BUILDS_2D)
    # a composed run selects the build its class was composed for (an LDR profile, U8, the identity swizzle; "hdr": an HDR profile)
    for s in D.composed(block):
        for (cls, kind), (_, _, infos) in zip(s.labels, s.runs()):
            if cls == "tail":
                continue
            profile = "PRF_HDR" if cls == "hdr" else "PRF_LDR"
            assert D.run_build(infos, profile, np.uint8, D.SWIZZLES["rgba"]) == D.CLASS_BUILD[cls], (s.name, cls)
            assert D.run_kind(infos, profile) == kind and D.run_kind(infos, "PRF_HDR") == kind, (s.name, cls, kind)
            if D.CLASS_BUILD[cls][1] and cls != "hdr":
                assert any(not i.dual_plane for i in infos if i.kind == D.NORMAL), "a kDual run holds one-plane blocks too"


@pytest.mark.parametrize("block", D.FOOTPRINTS_3D, ids=IDS_3D)
def test_every_3d_class_of_block_has_full_and_mixed_runs(block):
    count = collections.Counter()
    for s in D.composed(block):
        for (cls, kind), (_, _, infos) in zip(s.labels, s.runs()):
            if cls == "tail":
                continue
            assert D.run_kind(infos, "PRF_LDR") == kind == D.run_kind(infos, "PRF_HDR"), (s.name, cls, kind)
            payload = [i for i in infos if i.kind == D.NORMAL]
            ok = {"single": lambda i: i.partition_count == 1 and not i.dual_plane, "dual": lambda i: i.dual_plane,
                  "two": lambda i: i.partition_count == 2, "many": lambda i: i.partition_count >= 3}[cls]
            assert all(ok(i) for i in payload), (s.name, cls)
            count[(cls, kind)] += 1
    for cls in D.CLASSES_3D:
        assert count[(cls, "full")] >= 2 and count[(cls, "mixed")] >= 2, count


def test_run_build_on_hand_made_runs():
    """The rule itself, on runs small enough to read."""
    p = D.pool((6, 6))
    pick = lambda parts, dual, hdr: next(e.info for e in p.entries if e.info.kind == D.NORMAL and e.info.partition_count == parts and  # noqa: E731
                                         e.info.dual_plane == dual and D.has_hdr_format(e.info) == hdr)
    error = next(e.info for e in p.entries if e.info.kind == D.ERROR)
    fp16 = next(e.info for e in p.entries if e.info.kind == D.VOID_FP16)
    rgba, raz1 = D.SWIZZLES["rgba"], D.SWIZZLES["raz1"]
    assert D.run_build([pick(1, 0, False), error], "PRF_LDR", np.uint8, rgba) == (0, False, False)
    assert D.run_build([pick(1, 1, False), pick(1, 0, False)], "PRF_LDR", np.uint8, rgba) == (0, True, False)
    assert D.run_build([pick(2, 0, False)], "PRF_LDR_SRGB", np.uint8, rgba) == (1, False, False)
    assert D.run_build([pick(2, 1, False)], "PRF_LDR", np.uint8, rgba) == (1, True, False)
    assert D.run_build([pick(3, 0, False), pick(2, 0, False)], "PRF_LDR", np.uint8, rgba) == (2, False, False)
    assert D.run_build([pick(4, 0, False), pick(1, 1, False)], "PRF_LDR", np.uint8, rgba) == (2, True, False)
    assert D.run_build([pick(1, 0, True)], "PRF_LDR", np.uint8, rgba) == (0, False, False)          # (the error colour, from integers)
    assert D.run_build([pick(1, 0, True)], "PRF_HDR", np.uint8, rgba) == D.GENERAL
    assert D.run_build([pick(1, 0, False)], "PRF_LDR", np.uint8, raz1) == D.GENERAL
    assert D.run_build([error, fp16], "PRF_LDR", np.uint8, raz1) == (0, False, False)               # (no payload: nothing to compute)
    assert D.run_build([error], "PRF_LDR", np.float16, rgba) == D.GENERAL
    assert D.role(fp16, "PRF_LDR") == "error" and D.role(fp16, "PRF_HDR_RGB_LDR_A") == "constant"


@pytest.mark.parametrize("profile", D.PROFILES)
@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_emu_decodes_every_stream_as_the_reference(emu, ref, A, block, profile):
    """Bit for bit (NaN payloads included): U8, F16 and F32 through the identity, BGRA and (R, A, Z, 1) swizzles."""
    for s in D.streams(block):
        for out_type in D.OUT_TYPES:
            for swz in D.SWIZZLES:
                want = D.reference_decode(ref, A, s, profile, out_type, swz, keep=out_type is np.uint8 and swz == "rgba")
                got = D.decode(emu, A, s, profile, out_type, swz)
                bad = D.explain(s, want, got, profile, out_type, swz)
                assert bad is None, bad


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_emu_block_info_is_the_references_on_the_whole_pool(emu, ref, A, block):
    """astcenc_get_block_info, the whole struct byte for byte, in an LDR and an HDR profile."""
    p = D.pool(block)
    for profile in ("PRF_LDR", "PRF_HDR"):
        c_ref, c_emu = D._context(ref, A, profile, block), D._context(emu, A, profile, block)
        for e in p.entries:
            raw = (C.c_uint8 * 16).from_buffer_copy(e.bits)
            want, got = A.BlockInfo(), A.BlockInfo()
            ea = ref.lib.astcenc_get_block_info(c_ref, raw, C.byref(want))
            eb = emu.lib.astcenc_get_block_info(c_emu, raw, C.byref(got))
            assert ea == eb and bytes(want) == bytes(got), (profile, D.describe(e))
            # ... and the plain-C oracle's parse, which the matrix rests on, reads the same header
            assert bool(want.is_error_block) == (e.info.kind == D.ERROR), D.describe(e)
            if e.info.kind == D.NORMAL:
                assert (want.partition_count, bool(want.is_dual_plane_block), want.weight_x, want.weight_y, want.weight_z) == \
                    (e.info.partition_count, bool(e.info.dual_plane), e.info.weight_x, e.info.weight_y, e.info.weight_z), D.describe(e)
                assert [want.color_endpoint_modes[i] for i in range(want.partition_count)] == [e.info.format[i] for i in range(want.partition_count)]


@pytest.mark.parametrize("block", D.FOOTPRINTS, ids=IDS)
def test_oracle_decoder_agrees_on_the_ldr_u8_streams(ref, A, block):
    """Three implementations, one answer: oracle/astc_decode.c against the reference (which the emulator equals, above)."""
    dec = block_census.library()
    dec.astc_oracle_decode_volume.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p]
    bz = block[2] if len(block) > 2 else 1
    for s in D.streams(block):
        for profile, srgb in (("PRF_LDR", 0), ("PRF_LDR_SRGB", 1)):
            want = D.reference_decode(ref, A, s, profile, np.uint8, "rgba")
            w, h, d = s.dims
            got = np.zeros((d, h, w, 4), dtype=np.uint8)
            dec.astc_oracle_decode_volume(s.data.ctypes.data, block[0], block[1], bz, w, h, d, srgb, got.ctypes.data)
            bad = D.explain(s, want, got, profile, np.uint8, "rgba")
            assert bad is None, bad


def test_committed_census_is_that_of_the_corpus():
    """profiles/decode_coverage/census_after.txt is what `python tests/decode_cases.py after` prints today."""
    import os
    path = os.path.join(D.ROOT, "profiles", "decode_coverage", "census_after.txt")
    assert open(path).read() == "\n".join(D._after()) + "\n"
