# SPDX-License-Identifier: Apache-2.0
"""The coverage matrix of tests/encoding_cases.py, from the reference's own bytes: every mandatory cell (class of kernel
build x encoding feature) holds at least MIN_BLOCKS blocks over the class's images, the cells listed as unreachable or not
reached are indeed empty, and the sequential build of the kernel source gives the reference's bytes -- and therefore the
reference's census -- on every image.  The GPU side is tests/test_encoding_coverage.py."""
import collections

import pytest

import block_census
import encoding_cases as E
import images


@pytest.fixture(scope="module")
def reference(ref):
    return E.Reference(ref)


@pytest.fixture(scope="module")
def per_class(reference):
    """{class: Counter of features} of the reference's bytes over the class's images."""
    out = collections.OrderedDict((name, collections.Counter()) for name in E.CLASSES)
    for case in E.cases():
        out[case.build_class].update(block_census.census(reference.want(case.id), case.block))
    return out


def test_every_case_is_small_and_every_class_has_rows():
    assert {c.build_class for c in E.cases()} == set(E.CLASSES)
    for case in E.cases():
        case.image()                                     # (asserts at most 100 blocks)
        assert E.build_class(case.profile, case.block, case.quality) == case.build_class, case.id


def test_mandatory_cells_are_reached(per_class):
    """Four partitions in every generic class, an FP16 constant block in the HDR classes, and every cell the sweep tools'
    matrices reached (profiles/encoding_coverage/census_before.txt) hold MIN_BLOCKS blocks of the reference's output."""
    cells = E.mandatory_cells()
    assert set(E.MANDATORY) <= set(cells) and len(cells) > 100
    for cls, feature in cells:
        print("%-9s %-22s %d" % (cls, feature, per_class[cls][feature]))
    missing = [(cls, feature, per_class[cls][feature]) for cls, feature in cells if per_class[cls][feature] < E.MIN_BLOCKS]
    assert not missing, missing


def test_every_thorough_row_reaches_every_partition_count(reference):
    for row, (_, _, quality, _, _) in E.ROWS.items():
        if quality != E.A.PRE_THOROUGH:
            continue
        count = collections.Counter()
        for case in E.cases():
            if case.row == row:
                count.update(block_census.census(reference.want(case.id), case.block))
        for feature in E.ROW_MANDATORY:
            assert count[feature] >= E.MIN_BLOCKS, (row, feature, count[feature])


def test_tables_hold_what_they_claim(per_class):
    """BY_CONSTRUCTION features appear nowhere; a NOT_REACHED cell is no mandatory cell and is in fact below MIN_BLOCKS (so the
    table cannot go stale); every other cell of the matrix is reached."""
    for feature in E.BY_CONSTRUCTION:
        assert all(per_class[cls][feature] == 0 for cls in E.CLASSES), (feature, [per_class[cls][feature] for cls in E.CLASSES])
    mandatory = set(E.mandatory_cells())
    for cell, tried in E.NOT_REACHED.items():
        assert cell not in mandatory, cell
        assert tried
        assert per_class[cell[0]][cell[1]] < E.MIN_BLOCKS, ("reached after all: take it out of NOT_REACHED", cell, per_class[cell[0]][cell[1]])
    for cls in E.CLASSES:
        for feature in E.columns(cls.startswith("hdr")):
            if feature in E.BY_CONSTRUCTION or (cls, feature) in E.NOT_REACHED:
                continue
            assert per_class[cls][feature] >= E.MIN_BLOCKS, (cls, feature, per_class[cls][feature])
    assert all(per_class[cls]["kind:error"] == 0 for cls in E.CLASSES)


def test_committed_census_is_current(per_class):
    """profiles/encoding_coverage/census_after.txt is what the reference emits on today's images."""
    committed = {cls: {f: n for f, n in row.items() if n} for cls, row in E.read_census(E.CENSUS_AFTER).items()}
    assert committed == {cls: dict(c) for cls, c in per_class.items()}


@pytest.mark.parametrize("case_id", E.case_ids())
def test_sequential_build_matches_reference(reference, emu, case_id):
    case = reference.by_id[case_id]
    want = reference.want(case_id)
    got = emu.compress(case.image(), case.block, case.quality, profile=case.profile)
    bad = images.mismatches(want, got)
    assert len(bad) == 0, "%s: blocks differ: %s" % (case_id, bad[:8])
    assert block_census.census(got, case.block) == block_census.census(want, case.block)


# ---- float edge values through load_block (csrc/wave_*.h): the CPU twin of tests/test_encoding_coverage.py's case ---------


@pytest.mark.parametrize("case", E.float_edge_cases(), ids=E.float_edge_id)
def test_float_edge_values_sequential_build(ref, emu, case):
    dtype, profile, block, swizzle = case
    img = E.float_edge_image(dtype)
    want = ref.compress(img, block, E.FLOAT_EDGE_QUALITY, profile=profile, swizzle=swizzle)
    got = emu.compress(img, block, E.FLOAT_EDGE_QUALITY, profile=profile, swizzle=swizzle)
    bad = images.mismatches(want, got)
    assert len(bad) == 0, "blocks differ: %s" % bad[:8]
