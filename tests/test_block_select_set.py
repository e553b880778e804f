# SPDX-License-Identifier: Apache-2.0
"""Block selection over an image set with a block budget (astcenc_amd_select_blocks_set_device; csrc/kernel_select_set.hip,
csrc/block_budget.h): synthetic records, no compression, against a numpy model in float64 (numpy rounds every operation)

    e, n, candidate as tests/test_block_select.py's model, n from the block's own entry        key = e / n
    order = np.argsort(-key[candidates], kind="stable"); the first max_blocks of it, sorted ascending

Every comparison is for equality: the list, both counts, the untouched sentinel words past the count and in the guards on both
sides of the list, and a second run that gives the identical list.

Sets (SETS): one block; the 6x6 chain of 50x45 (99 blocks in 6 entries, n from 1 to 36); entry seams inside a wavefront's trip of
64 blocks and at the edge of a tile of 4096 blocks; about 70 000 blocks in 300 entries of random small sizes, one of them with
three slices; a 3D footprint; and, once, more than 2^21 blocks in two entries.

Patterns (PATTERNS), each with the budgets 0, 1, c - 1, c, c + 1, c // 2 and none: distinct random keys; a third of the
candidates with one bit-identical key, spread over the whole set, so that the cutoff of c // 2 falls inside the tie; keys that
differ in the lowest bits of the mantissa; keys over the whole exponent range and +inf; records whose order by e is the reverse of
their order by e / n (a kernel that ranks by e fails: `by_mean`); NaN records and 0 * inf through a zero weight (never
candidates); no candidates; thresholds 0 and +inf."""
import ctypes as C

import numpy as np
import pytest

import test_block_select as S

pytestmark = pytest.mark.gpu
SENTINEL = S.SENTINEL
GUARD = S.GUARD
NONE = 0xFFFFFFFF


def chain_dims(w, h):
    dims = [(w, h, 1)]
    while dims[-1][0] > 1 or dims[-1][1] > 1:
        dims.append((max(dims[-1][0] // 2, 1), max(dims[-1][1] // 2, 1), 1))
    return dims


def many_entries():
    rng = np.random.default_rng(5)
    dims = [(int(rng.integers(1, 160)), int(rng.integers(1, 160)), 1) for _ in range(300)]
    dims[137] = (31, 17, 3)                     # a 2D footprint over three slices
    return dims


# name -> (footprint, [dims of every entry])
SETS = {
    "one_block": ((6, 6, 1), [(5, 5, 1)]),
    "chain_50x45": ((6, 6, 1), chain_dims(50, 45)),
    "seams": ((4, 4, 1), [(252, 4, 1), (4, 4, 1), (260, 4, 1), (256, 256, 1), (3, 3, 1)]),
    "many": ((5, 5, 1), many_entries()),
    "footprint_3d": ((3, 3, 3), [(10, 7, 5), (4, 4, 4)]),
}
LARGE = ((4, 4, 1), [(5800, 5804, 1), (7, 7, 1)])
PATTERNS = ["distinct", "tie", "low_bits", "exponents", "by_mean", "nan", "none", "threshold_0", "threshold_inf"]


def set_texels(block, dims):
    return np.concatenate([S.texels(block, d) for d in dims])


def set_entry_of(block, dims):
    return np.concatenate([np.full(S.texels(block, d).size, i, dtype=np.uint32) for i, d in enumerate(dims)])


def keys_model(records, n, weight, threshold):
    """(candidate flags, keys as float64) of every block."""
    w = np.asarray(weight, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = ((w[0] * records[:, 0] + w[1] * records[:, 1]) + w[2] * records[:, 2]) + w[3] * records[:, 3]
        cand = e > np.float64(threshold) * n.astype(np.float64)
        key = e / n.astype(np.float64)
    return cand, key


def model(records, n, weight, threshold, max_blocks):
    """(the list, the candidate count)."""
    cand, key = keys_model(records, n, weight, threshold)
    index = np.flatnonzero(cand)
    order = np.argsort(-key[cand], kind="stable")
    if max_blocks != NONE:
        order = order[:max_blocks]
    return np.sort(index[order]).astype(np.uint32), int(index.size)


def case(pattern, n, seed):
    """(records [blocks, 4], weights, threshold) of a pattern."""
    rng = np.random.default_rng(seed)
    blocks = n.size
    nd = n.astype(np.float64)
    weight, threshold = (1.0, 1.0, 1.0, 1.0), 0.01
    records = np.zeros((blocks, 4))
    want = rng.random(blocks) < 0.6
    if blocks == 1:
        want[:] = True
    low = rng.random(blocks) * nd * 0.001                             # e < 0.001 n: no candidate
    if pattern == "distinct":
        key = 0.02 + rng.random(blocks)
        records[:, 1] = np.where(want, key * nd, low)
    elif pattern == "tie":
        # candidates in three classes by index: above the tie, the tie (0.5 n is exact, and so is 0.5 n / n), below it
        cls = rng.integers(0, 3, blocks)
        key = np.where(cls == 0, 0.75 + rng.random(blocks), np.where(cls == 1, 0.5, 0.02 + 0.4 * rng.random(blocks)))
        records[:, 2] = np.where(want, key * nd, low)
    elif pattern == "low_bits":
        step = rng.integers(0, 4, blocks).astype(np.float64)
        key = 0.3 * (1.0 + step * 2.0 ** -52)
        records[:, 0] = np.where(want, key * nd, low)
    elif pattern == "exponents":
        key = 10.0 ** rng.uniform(-300, 300, blocks)
        key[rng.random(blocks) < 0.05] = np.inf
        threshold = 0.0
        with np.errstate(all="ignore"):
            records[:, 3] = np.where(want, key * nd, 0.0)
    elif pattern == "by_mean":
        # e = n + 1 grows with n while e / n = 1 + 1 / n falls: the fewer texels, the higher the rank
        records[:, 0] = np.where(want, nd + 1.0 + rng.integers(0, 2, blocks), low)
    elif pattern == "nan":
        weight = (1.0, 0.0, 2.0, 0.5)
        records[:, 0] = np.where(want, (0.02 + rng.random(blocks)) * nd, low)
        which = rng.integers(0, 8, blocks)
        records[which == 0, 0] = np.nan
        records[which == 1, 0] = np.inf                               # a candidate, key +inf
        records[which == 2, 1] = np.inf                               # 0 * inf: a NaN, never a candidate
        records[which == 3, 3] = np.nan
    elif pattern == "none":
        records[:, 1] = low
    elif pattern == "threshold_0":
        threshold = 0.0
        records[:, 2] = np.where(want, rng.random(blocks) * nd, 0.0)
    elif pattern == "threshold_inf":
        threshold = np.inf
        records[:, 1] = rng.random(blocks) * nd
        records[::5, 2] = np.inf
    return np.ascontiguousarray(records), weight, threshold


def budgets(c):
    return sorted({b for b in (0, 1, c - 1, c, c + 1, c // 2) if b >= 0}) + [NONE]


@pytest.fixture(scope="module")
def contexts(product, A):
    made = {}

    def get(block):
        if block not in made:
            err, cfg = product.config_init(A.PRF_LDR, block[0], block[1], block[2], A.PRE_FAST, 0)
            assert err == 0
            err, ctx = product.context_alloc(cfg, 1)
            assert err == 0, product.error_string(err)
            made[block] = ctx
        return made[block]
    yield get
    for ctx in made.values():
        product.context_free(ctx)


def select(product, A, ctx, t_records, dims, weight, threshold, max_blocks, words):
    import torch
    whole = torch.full((GUARD + words + GUARD,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    err, cand, count = product.select_blocks_set_device(ctx, dims, t_records, A.block_criterion(threshold, weight), whole[GUARD:GUARD + words], max_blocks)
    assert err == 0, product.error_string(err)
    return cand, count, whole.cpu().numpy().view(np.uint32)


def check(product, A, ctx, block, dims, pattern, seed, only_budget=None):
    import torch
    n = set_texels(block, dims)
    records, weight, threshold = case(pattern, n, seed)
    t_records = torch.from_numpy(records).cuda()
    c = model(records, n, weight, threshold, NONE)[1]
    for max_blocks in budgets(c) if only_budget is None else [only_budget(c)]:
        want, _ = model(records, n, weight, threshold, max_blocks)
        what = (block, len(dims), pattern, max_blocks, c)
        assert want.size == min(c, max_blocks), what
        words = max(min(n.size, max_blocks), 1)         # (the budget's words are enough; a budget of 0 still needs a buffer)
        cand, count, got = select(product, A, ctx, t_records, dims, weight, threshold, max_blocks, words)
        assert cand == c and count == want.size, (what, cand, count, want.size)
        assert np.array_equal(got[GUARD:GUARD + count], want), what
        assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + count:] == SENTINEL).all(), what
        cand2, count2, again = select(product, A, ctx, t_records, dims, weight, threshold, max_blocks, words)
        assert (cand2, count2) == (cand, count) and np.array_equal(again, got), what
    return records, n, weight, threshold, c


@pytest.mark.parametrize("name", list(SETS))
def test_patterns(product, A, contexts, name):
    block, dims = SETS[name]
    for i, pattern in enumerate(PATTERNS):
        records, n, weight, threshold, c = check(product, A, contexts(block), block, dims, pattern, 500 + i)
        if pattern in ("none", "threshold_inf"):
            assert c == 0
        elif n.size >= 60:
            assert c >= 8, (name, pattern)
        if pattern == "tie" and n.size >= 60:
            # the cutoff of c // 2 falls inside the tie, which spreads over entries (and, in the larger sets, tiles)
            cand, key = keys_model(records, n, weight, threshold)
            tied = np.flatnonzero(cand & (key == 0.5))
            above = int((key[cand] > 0.5).sum())
            assert above < c // 2 < above + tied.size, (name, above, tied.size, c)
            assert len(set(set_entry_of(block, dims)[tied].tolist())) >= 2
            if n.size > 8192:
                assert len(set((tied // 4096).tolist())) >= 2
        if pattern == "by_mean" and name in ("chain_50x45", "many"):
            # (the case tells the two rankings apart: the top half by e is another set than the top half by e / n)
            e = records[:, 0]
            index = np.flatnonzero(cand_of(records, n, weight, threshold))
            by_e = np.sort(index[np.argsort(-e[index], kind="stable")[:c // 2]])
            assert not np.array_equal(by_e, model(records, n, weight, threshold, c // 2)[0])


def cand_of(records, n, weight, threshold):
    return keys_model(records, n, weight, threshold)[0]


def test_set_geometry():
    """What the docstring says of the sets (no GPU work, but it guards the cases above)."""
    block, dims = SETS["chain_50x45"]
    assert dims == [(50, 45, 1), (25, 22, 1), (12, 11, 1), (6, 5, 1), (3, 2, 1), (1, 1, 1)]
    assert [S.texels(block, d).size for d in dims] == [72, 20, 4, 1, 1, 1]
    n = set_texels(block, dims)
    assert n.min() == 1 and n.max() == 36
    assert [S.texels((4, 4, 1), d).size for d in SETS["seams"][1]] == [63, 1, 65, 4096, 1]
    assert 60000 < set_texels(*SETS["many"]).size < 80000


def test_beyond_2_21_blocks(product, A, contexts):
    block, dims = LARGE
    _, n, _, _, c = check(product, A, contexts(block), block, dims, "distinct", 7, only_budget=lambda c: c // 3)
    assert n.size > 1024 * 2048 and c > 900000


@pytest.mark.parametrize("block,dims", S.GEOMETRY, ids=["%d" % c for c in S.COUNTS])
def test_one_entry_without_a_budget_is_the_single_image_call(product, A, contexts, block, dims):
    import torch
    n = S.texels(block, dims)
    for i, pattern in enumerate(("random", "nan_inf", "alternating")):
        records, weight, threshold = S.case(pattern, n, 40 + i)
        t_records = torch.from_numpy(records).cuda()
        count1, single = S.select(product, A, contexts(block), t_records, dims, weight, threshold, n.size)
        cand, count, got = select(product, A, contexts(block), t_records, [dims], weight, threshold, NONE, n.size)
        assert cand == count == count1 and np.array_equal(got, single), (block, dims, pattern)


def test_errors_write_nothing(product, A, contexts):
    import torch
    block, dims = SETS["chain_50x45"]
    ctx = contexts(block)
    blocks = 99
    n = set_texels(block, dims)
    records = torch.from_numpy(case("distinct", n, 1)[0]).cuda()
    whole = torch.full((GUARD + blocks + GUARD,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    out = whole[GUARD:GUARD + blocks]
    L = product.lib
    good = A.block_criterion(0.01)
    cand, count = C.c_uint(55), C.c_uint(77)

    def entries_of(dims):
        return (A.ImageSetEntry * len(dims))(*[A.ImageSetEntry(None, None, 0, d[0], d[1], d[2], A.TYPE_U8, A.Swizzle(*A.SWZ_RGBA)) for d in dims])

    def call(ctx=ctx, entries=entries_of(dims), n_entries=len(dims), rec=records.data_ptr(), rec_len=blocks * 32, crit=good, budget=NONE,
             lst=out.data_ptr(), lst_len=blocks * 4, cnd=C.byref(cand), cnt=C.byref(count)):
        return L.astcenc_amd_select_blocks_set_device(ctx, entries, n_entries, rec, rec_len, C.byref(crit) if crit is not None else None, budget,
                                                      lst, lst_len, None, cnd, cnt)

    assert call(ctx=None) == A.ERR_BAD_PARAM
    assert call(crit=None) == A.ERR_BAD_PARAM
    assert call(cnt=None) == A.ERR_BAD_PARAM
    assert call(entries=None) == A.ERR_BAD_PARAM
    for bad in ((0, 22, 1), (25, 0, 1), (25, 22, 0)):
        assert call(entries=entries_of([dims[0], bad] + dims[2:])) == A.ERR_BAD_PARAM
    # more than 2^32 - 1 blocks in all: two entries of 2^31 blocks each at 6x6
    huge = [(6 * 65536, 6 * 32768, 1)] * 2
    assert call(entries=entries_of(huge), n_entries=2) == A.ERR_BAD_PARAM
    nan, inf = float("nan"), float("inf")
    for weights, threshold in (((nan, 1, 1, 1), 0.01), ((1, -1.0, 1, 1), 0.01), ((1, 1, inf, 1), 0.01), ((1, 1, 1, 1), nan), ((1, 1, 1, 1), -0.5)):
        assert call(crit=A.block_criterion(threshold, weights)) == A.ERR_BAD_PARAM, (weights, threshold)
    assert call(rec=None) == A.ERR_BAD_CONTEXT
    assert call(lst=None) == A.ERR_BAD_CONTEXT
    assert call(rec_len=blocks * 32 - 1) == A.ERR_OUT_OF_MEM
    assert call(lst_len=blocks * 4 - 1) == A.ERR_OUT_OF_MEM
    assert call(budget=10, lst_len=10 * 4 - 1) == A.ERR_OUT_OF_MEM
    assert cand.value == 55 and count.value == 77 and (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # an empty set succeeds with both counts 0; the optional count may be null; a list of the budget's size is enough
    assert call(n_entries=0) == A.SUCCESS and cand.value == 0 and count.value == 0
    cand.value, count.value = 55, 77
    assert call(entries=None, n_entries=0, rec=None, lst=None) == A.SUCCESS and cand.value == 0 and count.value == 0
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert call(cnd=None, budget=10, lst_len=10 * 4) == A.SUCCESS and count.value == 10
    got = whole.cpu().numpy().view(np.uint32)
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + 10:] == SENTINEL).all() and (got[GUARD:GUARD + 10] != SENTINEL).all()
