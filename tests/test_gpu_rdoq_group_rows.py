"""rdoq_wave decides the 4x4 groups of one diagonal of a block's group grid together, a group per row of 16 lanes, and forms the
sums group by group afterwards (ctu_core.h): the device search against the oracle on 128x128 pictures whose decided blocks hold
several groups on a diagonal, diagonals of two passes, groups without levels beside groups with levels, a last group inside its
diagonal, and levels on both sides of the regular-bin budget.  A slip in a row's position, its Rice parameter, the budget test or
the order of the sums changes a level or a decision and shows in a CTU's CRC or in its models.  One P / B sequence: its kernel
compiles the same rdoq_wave."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu
from test_gpu_coder_models_only import CASES as CODER_CASES, certainly_over_budget, transform_blocks
from test_gpu_rdoq_scan_sums import diag, scan_of

pytestmark = pytest.mark.gpu

CASES = CODER_CASES + [(128, 128, 8, 37, 2005), (128, 128, 8, 22, 7)]
SHAPES = ["luma 8", "luma 16", "luma 32", "luma 32 of a 64x64 CU", "chroma 8", "chroma 16"]
# what a decided block's levels say of the passes that produced them.  A group is a 4x4 group of the block in diagonal order; only
# groups at or below the group of the last level count (the final levels are a lower bound of what RDOQ sees: its own last
# candidate lies at or behind the last level).
TWO, FOUR, FIVE = "two or more groups on one diagonal", "four on one diagonal", "five or more on one diagonal (two passes)"
MIXED = "a group without levels on a diagonal that also holds one with levels"
OVER, UNDER = "certainly over the regular-bin budget", "certainly not over it"
INSIDE = "the last level's group inside its diagonal, another group of that diagonal below it"
WANTED = {TWO: SHAPES, FOUR: ["luma 16", "luma 32", "chroma 16"], FIVE: ["luma 32", "luma 32 of a 64x64 CU"], MIXED: SHAPES,
          OVER: SHAPES, UNDER: SHAPES, INSIDE: ["luma 16", "luma 32", "chroma 16", "luma 32 of a 64x64 CU"]}


def paths_of(block):
    """-> the set of WANTED's predicates a coded block's levels stand for"""
    n = block.shape[0]
    a = np.abs(block.astype(np.int64)).ravel()[scan_of(n)]
    cg_last = int(np.flatnonzero(a)[-1]) >> 4
    has = a.reshape(-1, 16).any(axis=1)
    got = {OVER if certainly_over_budget(block) else UNDER}
    by_diag = {}
    for g, (gx, gy) in enumerate(diag(n // 4)[:cg_last + 1]):
        by_diag.setdefault(gx + gy, []).append(g)
    for d, gs in by_diag.items():
        if len(gs) >= 2:
            got.add(TWO)
        if len(gs) >= 4:
            got.add(FOUR)
        if len(gs) >= 5:
            got.add(FIVE)
        if has[gs].any() and not has[gs].all():
            got.add(MIXED)
    gx, gy = diag(n // 4)[cg_last]
    full = sum(1 for x, y in diag(n // 4) if x + y == gx + gy)
    if 2 <= len(by_diag[gx + gy]) < full:
        got.add(INSIDE)
    return got


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once; the coverage the cases are there for is asserted here, on the oracle's
    result, before any comparison."""
    res, seen = {}, {s: set() for s in SHAPES}
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        for name, blk in transform_blocks(o, W, Hh):
            if name in seen:
                seen[name] |= paths_of(blk)
    for p, shapes in WANTED.items():
        for s in shapes:
            assert p in seen[s], (s, p)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_with_a_diagonals_groups_decided_together_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_with_a_diagonals_groups_decided_together_equals_the_encoders_records(hip):
    """The P / B kernel's rdoq_wave: the smallest P / B golden through test_gpu_ctu_search_pb's own route; the records carry luma and
    chroma levels."""
    import torch
    from uvg266_amd import api
    import test_gpu_ctu_search_pb as PB
    name = min(PB.GOLDENS, key=lambda n: os.path.getsize(os.path.join(H.GOLDEN, n + ".npz")))
    g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    W, Hh, depth, pics, P = H.inter_pictures_from_golden(g)
    descs, tens, recs = PB.device_pictures(W, Hh, depth, pics, P)
    api.ctu_search_pb(descs, depth)
    torch.cuda.synchronize()
    luma = chroma = 0
    for t, (fr, d) in zip(tens, recs):
        assert H.compare_device_inter_picture(W, Hh, d, PB.result_of(W, Hh, t)) == [], f"frame {fr}"
        co = np.asarray(d["coeff"]).reshape(-1, 6144)
        luma += int(np.count_nonzero(co[:, :4096]))
        chroma += int(np.count_nonzero(co[:, 4096:]))
    assert luma > 0 and chroma > 0
