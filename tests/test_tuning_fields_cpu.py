# SPDX-License-Identifier: Apache-2.0
"""Hand-set tuning fields (tests/tuning_cases.py) on the CPU: the reference (oracle/_ref), the sequential build of the kernel
source (oracle/emu), its reversed-lane build, and make_lds_layout().

(a) from the reference's bytes alone: every in-range case changes at least one block against its base context, every
    out-of-range case gives the bytes of the clamp edge, a field a context does not read changes nothing.  A (field, direction)
    no case makes bite is in tuning_cases.NOT_SHOWN, a single case that does not although its field does elsewhere in
    tuning_cases.QUIET; both lists fail when an entry does bite.
(b) the sequential build gives the reference's bytes for every case and every combination.
(c) so does the reversed-lane build, on every combination and on the cases of every field.
(d) every layout make_lds_layout() gives for the combinations keeps the candidate records of a batch inside the allocation
    and fits the 160 KiB the HIP backend accepts.

The fixed-context identity (a context with one field changed must not get a fixed-context build) is checked on the GPU only,
tests/test_tuning_fields.py: the sequential library reports "emu" for every context, it has no fixed builds to name."""
import math
import os
import re
import subprocess
import sys

import pytest

import tuning_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_LIMIT = 160 * 1024      # csrc/backend_hip.hip: a larger working set is refused at context_alloc


@pytest.fixture(scope="module")
def want(ref):
    return T.Outputs(ref)


@pytest.fixture(scope="module")
def forward(emu):
    return T.Outputs(emu)


@pytest.fixture(scope="module")
def reverse(built, A):
    import oracle_libs as O
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle", "emu"), "reverse"])
    return T.Outputs(A.Library(O.LIB_EMU_REVERSE))


def _bites(want, ref):
    """{case id: blocks changed}, {(field, direction): blocks changed over its in-range cases} from the reference."""
    per_case, per_pair = {}, {}
    for c in T.cases():
        if c.kind in ("below", "above", "inert", "nan"):
            continue
        d = T.direction(c.value, T.config_value(ref, c))
        assert d is not None, ("the case's value is the base context's", T.case_id(c))
        n = want.bite(c)
        per_case[T.case_id(c)] = (c, d, n)
        per_pair[(c.field, d)] = per_pair.get((c.field, d), 0) + n
    return per_case, per_pair


@pytest.mark.parametrize("field", T.FIELDS)
def test_the_field_bites_in_the_reference(want, ref, field):
    """(a) per field, from reference bytes only."""
    for c in T.cases_of(field):
        cid = T.case_id(c)
        got, base = want.want(T.context_of(c), c.image), want.want(T.base_context_of(c), c.image)
        if c.kind in ("below", "above"):
            edge = T.clamp_edge(c)
            assert T.differing(got, want.want(T.context_of(edge), c.image)) == 0, ("not clamped to %r" % (edge.value,), cid)
            continue
        if c.kind == "inert":
            assert T.differing(got, base) == 0, ("a field this context should not read changes bytes", cid)
            continue
        if c.kind == "nan":
            continue        # deterministic in the reference; what it must equal is the sequential build's business (b)
        d = T.direction(c.value, T.config_value(ref, c))
        n = T.differing(got, base)
        if c.kind == "side" and (c.value >= 0.85) == (T.config_value(ref, c) >= 0.85):
            assert n == 0, ("on the base's side of the 0.85 threshold, and bytes change", cid)
        elif (c.field, d) in T.NOT_SHOWN or cid in T.QUIET:
            assert n == 0, ("listed as not biting, and %d blocks change: take it off the list" % n, cid)
        else:
            assert n > 0, ("no block changes: the case tests nothing", cid)


def test_not_shown_is_short_and_every_field_bites(want, ref):
    per_case, per_pair = _bites(want, ref)
    assert len(T.NOT_SHOWN) <= T.MAX_NOT_SHOWN
    for pair in T.NOT_SHOWN:
        assert per_pair.get(pair, 0) == 0, ("listed in NOT_SHOWN, and it bites", pair, per_pair[pair])
    for field in T.FIELDS:
        shown = [d for d in ("down", "up") if per_pair.get((field, d), 0) > 0]
        assert shown or field in T.MAY_BE_SILENT, (field, "bites in no direction")
    # a pair with cases and no bite anywhere must be listed; a QUIET case is a case of the table
    silent = [pair for pair, n in per_pair.items() if n == 0 and pair not in T.NOT_SHOWN]
    assert not silent, silent
    assert not [cid for cid in T.QUIET if cid not in per_case], "QUIET names cases the table does not hold"


@pytest.mark.parametrize("field", T.FIELDS)
def test_sequential_build_matches_the_reference(want, forward, field):
    """(b) every case of the field, NaN and out-of-range values included."""
    bad = []
    for c in T.cases_of(field):
        n = T.differing(want.want(T.context_of(c), c.image), forward.want(T.context_of(c), c.image))
        if n:
            bad.append((T.case_id(c), n))
    assert not bad, bad


def _combo_groups():
    return [(profile, block, q) for profile, block, _ in T.COMBO_FOOTPRINTS for q in T.COMBO_PRESETS]


def _group_id(g):
    return "%s%s-q%g" % ("hdr" if g[0] == T.A.PRF_HDR else "ldr", "x".join(map(str, g[1])), g[2])


def _combos_of(group):
    return [c for c in T.combos() if (c.profile, c.block, c.quality) == group]


@pytest.mark.parametrize("group", _combo_groups(), ids=_group_id)
def test_sequential_build_matches_the_reference_on_combinations(want, forward, group):
    """(b) the sixteen corners of {candidates 1, 8} x {partitions 1, 4} x {index limits 1, 1024} x {mode limit 1, 100}."""
    bad = []
    for c in _combos_of(group):
        n = T.differing(want.want(c[:5], c.image), forward.want(c[:5], c.image))
        if n:
            bad.append((T.combo_id(c), n))
    assert not bad, bad


@pytest.mark.parametrize("group", _combo_groups(), ids=_group_id)
def test_combinations_do_not_depend_on_the_lane_order(forward, reverse, group):
    """(c) a missing barrier between the lanes of one loop changes bytes when the lanes run backwards (test_emu_lane_order.py)."""
    bad = []
    for c in _combos_of(group):
        n = T.differing(forward.want(c[:5], c.image), reverse.want(c[:5], c.image))
        if n:
            bad.append((T.combo_id(c), n))
    assert not bad, bad


def lane_order_cases():
    """One case per field and base: the upper end of the range where there is one (the longest loops), else the first."""
    out = []
    for field in T.FIELDS:
        for base in T.bases_of(field):
            mine = [c for c in T.cases_of(field) if c.base == base]
            out.append(([c for c in mine if c.kind == "hi"] or mine)[0])
    return out


def test_cases_do_not_depend_on_the_lane_order(forward, reverse):
    cases = lane_order_cases()
    assert {c.field for c in cases} == set(T.FIELDS)
    bad = []
    for c in cases:
        n = T.differing(forward.want(T.context_of(c), c.image), reverse.want(T.context_of(c), c.image))
        if n:
            bad.append((T.case_id(c), n))
    assert not bad, bad


LAYOUT_SCRIPT = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import astcenc_amd as A, oracle_libs as O
import tuning_cases as T
lib = A.Library(O.LIB_EMU)
for c in T.combos():
    sys.stderr.write("case %%s\n" %% T.combo_id(c))
    block = c.block
    one = T.image(c.image, block)[..., :block[1], :block[0], :]          # (the layout is the context's: one block is enough)
    T.compress(lib, c[:5], np.ascontiguousarray(one))
""" % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "astc-encoder_amd", "python"), os.path.join(ROOT, "oracle"))
LAYOUT = re.compile(r"lds layout: total (\d+) .* candw (\d+) .* batch: cstate (\d+) stride (\d+) per batch (\d+) / (\d+)")


def test_layouts_of_the_combinations_fit(built):
    """(d) make_lds_layout() with limits no preset holds: the records of the largest batch end inside the allocation
    (test_lds_layout.py checks that for the presets), every total fits a CU's 160 KiB, one layout per context."""
    env = dict(os.environ, ASTC_EMU_DUMP_LAYOUT="1")
    r = subprocess.run([sys.executable, "-c", LAYOUT_SCRIPT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    totals, case = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("case "):
            case = line[5:]
        m = LAYOUT.search(line)
        if not m:
            continue
        total, candw, cstate, stride, nb1, nb2 = (int(x) for x in m.groups())
        assert case not in totals, ("two layouts for one context", case)
        assert cstate + (max(nb1, nb2) - 1) * stride <= total, (case, line)
        totals[case] = total
    largest = max(totals, key=totals.get)
    print("largest layout: %d B (%s)" % (totals[largest], largest))
    assert len(totals) == len(T.combos()), "%d layouts for %d contexts" % (len(totals), len(T.combos()))
    assert totals[largest] <= LDS_LIMIT, "largest layout %d B (%s) of %d allowed" % (totals[largest], largest, LDS_LIMIT)


def test_table_covers_what_it_says():
    """The table itself: every field at both ends, an interior value, outside the range on every clamped side, NaN and +inf
    for the float fields; the footprints; the combinations' corners on the smallest and largest footprint of every class."""
    for field in T.FIELDS:
        kinds = [k for _, k in T.VALUES[field]]
        values = [v for v, _ in T.VALUES[field]]
        if field == "tune_search_mode0_enable":
            assert [v for v in values if v < 0.85] and [v for v in values if v >= 0.85]
        else:
            assert "lo" in kinds and "mid" in kinds and "below" in kinds, field
            assert "hi" in kinds or field == "tune_refinement_limit", field
        if field in T.INT_FIELDS and field != "tune_refinement_limit":
            assert "above" in kinds, field
        if field in T.FLOAT_FIELDS:
            assert any(math.isnan(v) for v in values) and any(math.isinf(v) for v in values), field
        bases = T.bases_of(field)
        assert field == "rgbm_m_scale" or [T.BASES[b][1] for b in bases] == [(6, 6), (10, 8), (5, 5, 5), (6, 6)], field
    assert set(T.PARTITION_FIELDS) >= {"tune_%dpartition_index_limit" % n for n in (2, 3, 4)}
    assert len(T.combos()) == 8 * 2 * 16
    for profile, block, cls in T.COMBO_FOOTPRINTS:
        assert T.build_class(profile, block, T.A.PRE_FASTEST, {"tune_candidate_limit": 1}) == cls, (block, cls)
    assert {cls for _, _, cls in T.COMBO_FOOTPRINTS} == {"ldr64", "ldr", "hdr64", "hdr", "3d"}
    assert len({T.combo_id(c) for c in T.combos()}) == len(T.combos()) and len({T.case_id(c) for c in T.cases()}) == len(T.cases())
