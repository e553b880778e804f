# SPDX-License-Identifier: Apache-2.0
"""Block selection (astcenc_amd_select_blocks_device; csrc/kernel_select.hip, csrc/block_select.h): synthetic records, no
compression, against a numpy model of the criterion

    e = ((w0 s0 + w1 s1) + w2 s2) + w3 s3        n = the block's texels inside the image        selected iff e > threshold * n

in float64 (numpy rounds every operation, as the contract asks).  The list must equal np.flatnonzero(model) exactly, the count
must be its length, the words past the count and the guards on both sides of the list must be untouched, and two runs must agree.

Block counts (GEOMETRY): 1, 63, 64, 65 (one wavefront trip and its edges), 4096 and 4097 (two tiles and one block of a third),
70 000 (35 tiles), a little over 2^21 (the scan's second trip: more than 1024 tiles; one pattern only), and three small ones
whose blocks are partial in x, y and z and a 2D footprint over slices, so that n differs between blocks.

One-line mistakes these catch: a wavefront's base that forgets the wavefronts before it in the tile, or a tile's that forgets
the scan's carry (alternating, random); >= for > (the ties of `random`); n taken as the whole footprint (partial blocks, whose
records lie between the two limits); a NaN selected; the predicate evaluated past the last block (only the last, 63 / 65 /
4097); anything written past the count (none selected, only the first)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SENTINEL = np.uint32(0xA5A5A5A5)
GUARD = 16                       # words on both sides of the list

# (block, (x, y, z)) -> blocks
GEOMETRY = [((6, 6, 1), (5, 5, 1)), ((4, 4, 1), (250, 2, 1)), ((4, 4, 1), (256, 4, 1)), ((5, 5, 1), (63, 23, 1)), ((4, 4, 1), (256, 256, 1)),
            ((6, 6, 1), (100, 1445, 1)), ((4, 4, 1), (1120, 1000, 1)), ((4, 4, 4), (30, 30, 10)), ((3, 3, 3), (10, 7, 5)), ((6, 6, 1), (40, 20, 3))]
COUNTS = [1, 63, 64, 65, 4096, 4097, 70000, 192, 24, 84]
LARGE = ((4, 4, 1), (5800, 5804, 1))         # 1450 x 1451 = 2 103 950 blocks, 1028 tiles
PATTERNS = ["none", "all", "alternating", "random", "first", "last", "nan_inf", "zero_weights", "threshold_0", "threshold_inf"]


def texels(block, dims):
    """[blocks] texels of every block that lie inside the image, raster order."""
    axes = []
    for b, d in zip(block, dims):
        nb = -(-d // b)
        axes.append(np.minimum(b, d - np.arange(nb) * b))
    nx, ny, nz = axes
    return (nz[:, None, None] * ny[None, :, None] * nx[None, None, :]).reshape(-1).astype(np.uint32)


def model(records, n, weight, threshold):
    w = np.asarray(weight, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = ((w[0] * records[:, 0] + w[1] * records[:, 1]) + w[2] * records[:, 2]) + w[3] * records[:, 3]
        return e > np.float64(threshold) * n.astype(np.float64)


def case(pattern, n, seed):
    """(records [blocks, 4], weights, threshold) of a pattern."""
    rng = np.random.default_rng(seed)
    blocks = n.size
    nd = n.astype(np.float64)[:, None]
    weight, threshold = (1.0, 1.0, 1.0, 1.0), 0.01
    low = rng.random((blocks, 4)) * nd * 0.001 / 4                  # e < 0.001 n
    # between threshold * n and threshold * the whole footprint where a block is partial: n matters
    high = (1.0 + rng.random((blocks, 4))) * nd * 0.01 / 3
    want = np.zeros(blocks, dtype=bool)
    if pattern == "all":
        want[:] = True
    elif pattern == "alternating":
        want[::2] = True
    elif pattern in ("random", "zero_weights", "nan_inf", "threshold_0", "threshold_inf"):
        want = rng.random(blocks) < 0.5
    elif pattern == "first":
        want[0] = True
    elif pattern == "last":
        want[-1] = True
    records = np.where(want[:, None], high, low)
    if pattern == "random":
        # ties: e == threshold * n exactly is not selected
        ties = np.arange(blocks)[3::11]
        records[ties] = 0.0
        records[ties, 1] = np.float64(threshold) * n[ties].astype(np.float64)
    if pattern == "zero_weights":
        weight = (0.0, 2.5, 0.0, 0.125)
        records[:, 0] = rng.random(blocks) * 1e6                    # a large error in a channel that does not count
    if pattern == "nan_inf":
        weight = (1.0, 0.0, 2.0, 0.5)
        which = rng.integers(0, 8, blocks)
        records[which == 0, 0] = np.nan
        records[which == 1, 0] = np.inf                             # selected
        records[which == 2, 1] = np.inf                             # 0 * inf: a NaN, never selected
        records[which == 3, 3] = np.nan
    if pattern == "threshold_0":
        threshold = 0.0
        records[~want] = 0.0
    if pattern == "threshold_inf":
        threshold = np.inf
        records[::5, 2] = np.inf
    return np.ascontiguousarray(records), weight, threshold


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


def select(product, A, ctx, t_records, dims, weight, threshold, blocks):
    import torch
    whole = torch.full((GUARD + blocks + GUARD,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    err, count = product.select_blocks_device(ctx, t_records, dims, A.block_criterion(threshold, weight), whole[GUARD:GUARD + blocks])
    assert err == 0, product.error_string(err)
    return count, whole.cpu().numpy().view(np.uint32)


def check(product, A, ctx, block, dims, pattern, seed):
    import torch
    n = texels(block, dims)
    records, weight, threshold = case(pattern, n, seed)
    want = np.flatnonzero(model(records, n, weight, threshold)).astype(np.uint32)
    t_records = torch.from_numpy(records).cuda()
    count, got = select(product, A, ctx, t_records, dims, weight, threshold, n.size)
    what = (block, dims, pattern)
    assert count == want.size, (what, count, want.size)
    assert np.array_equal(got[GUARD:GUARD + count], want), what
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + count:] == SENTINEL).all(), what
    count2, again = select(product, A, ctx, t_records, dims, weight, threshold, n.size)
    assert count2 == count and np.array_equal(again, got), what
    return want


@pytest.mark.parametrize("block,dims,blocks", [g + (c,) for g, c in zip(GEOMETRY, COUNTS)], ids=["%d" % c for c in COUNTS])
def test_patterns(product, A, contexts, block, dims, blocks):
    assert texels(block, dims).size == blocks
    for i, pattern in enumerate(PATTERNS):
        want = check(product, A, contexts(block), block, dims, pattern, 100 + i)
        if pattern in ("none", "threshold_inf"):
            assert want.size == 0
        if pattern == "all":
            assert want.size == blocks


def test_scan_second_trip(product, A, contexts):
    block, dims = LARGE
    want = check(product, A, contexts(block), block, dims, "random", 7)
    assert texels(block, dims).size > 1024 * 2048 and want.size > 900000


def test_partial_blocks_count_their_texels(product, A, contexts):
    """Every block of a volume with partial blocks on all three axes selected by records that lie below threshold * the whole
    footprint wherever a block has a quarter of it or less: a kernel that takes n as the footprint selects none of those."""
    block, dims = (4, 4, 4), (30, 30, 10)
    n = texels(block, dims)
    records, weight, threshold = case("all", n, 3)
    assert check(product, A, contexts(block), block, dims, "all", 3).size == n.size
    whole_footprint = np.full_like(n, 64)
    assert model(records, n, weight, threshold).all() and not model(records, whole_footprint, weight, threshold)[n <= 16].any()
    assert sorted(set(n.tolist())) == [8, 16, 32, 64]


def test_errors_write_nothing(product, A, contexts):
    import torch
    block, dims = (5, 5, 1), (63, 23, 1)
    ctx = contexts(block)
    blocks = 65
    records = torch.from_numpy(case("all", texels(block, dims), 1)[0]).cuda()
    whole = torch.full((GUARD + blocks + GUARD,), int(SENTINEL.view(np.int32)), dtype=torch.int32, device="cuda")
    out = whole[GUARD:GUARD + blocks]
    L = product.lib
    good = A.block_criterion(0.01)
    count = C.c_uint(77)

    def call(ctx=ctx, rec=records.data_ptr(), rec_len=blocks * 32, dims=dims, crit=good, lst=out.data_ptr(), lst_len=blocks * 4, cnt=C.byref(count)):
        return L.astcenc_amd_select_blocks_device(ctx, rec, rec_len, dims[0], dims[1], dims[2], C.byref(crit) if crit is not None else None, lst, lst_len, None, cnt)

    assert call(ctx=None) == A.ERR_BAD_PARAM
    assert call(crit=None) == A.ERR_BAD_PARAM
    assert call(cnt=None) == A.ERR_BAD_PARAM
    for bad_dims in ((0, 23, 1), (63, 0, 1), (63, 23, 0)):
        assert call(dims=bad_dims) == A.ERR_BAD_PARAM
    nan, inf = float("nan"), float("inf")
    for weights, threshold in (((nan, 1, 1, 1), 0.01), ((1, -1.0, 1, 1), 0.01), ((1, 1, inf, 1), 0.01), ((1, 1, 1, 1), nan), ((1, 1, 1, 1), -0.5),
                               ((1, 1, 1, 1), -inf)):
        assert call(crit=A.block_criterion(threshold, weights)) == A.ERR_BAD_PARAM, (weights, threshold)
    assert call(rec=None) == A.ERR_BAD_CONTEXT
    assert call(lst=None) == A.ERR_BAD_CONTEXT
    assert call(rec_len=blocks * 32 - 1) == A.ERR_OUT_OF_MEM
    assert call(lst_len=blocks * 4 - 1) == A.ERR_OUT_OF_MEM
    assert count.value == 77 and (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()
    # (+inf is a legal threshold, zero weights are legal)
    assert call(crit=A.block_criterion(inf, (0, 0, 0, 0))) == A.SUCCESS and count.value == 0
    assert (whole.cpu().numpy().view(np.uint32) == SENTINEL).all()
