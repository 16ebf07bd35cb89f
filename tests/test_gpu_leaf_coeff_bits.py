"""coeff_bits4r (ctu_leaf4.h: the bit count of every 4x4 block -- the luma block of a 4x4 CU, the Cb and Cr blocks of a 4x4 area and
of an 8x8 CU -- and, without the count, the coder's pass over them) on the packed sweep: the device search against the oracle on
small pictures.  The search's own models are what the function adapts, and the decisions are what its sums feed, so the CTUs' CRCs
(partition, modes, levels, reconstruction) and all three model sets are compared.  The cases are chosen so that the 4x4 CUs of the
final decisions hold luma blocks certainly over the budget of 28 regular bins and not, with their last level at scan position 0 and
at 15, with a level of 4 and more (a remainder) and of 300 and more (the long escape code), and chroma blocks of 4x4 areas over the
budget and not, ending at 0 and at 15 -- asserted on the oracle's result alone (a lower bound of what the search counts) before
anything is compared.  One P / B sequence holds the P / B kernel's copy.

No test here can see a sum that is off without flipping a decision: for that stand the comparison of `bench.py --dump-outputs`
against the parent's and the full-size goldens of the suite."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_coder_models_only import certainly_over_budget
from test_gpu_ctu_search import run_gpu

pytestmark = pytest.mark.gpu

# (W, H, depth, QP, t of H.varied_picture)
CASES = [(128, 128, 8, 7, 5), (128, 128, 8, 7, 2005), (128, 128, 8, 12, 1005), (128, 128, 8, 22, 5), (128, 128, 10, 7, 5), (128, 128, 10, 2, 5),
         (64, 64, 10, 7, 5)]
SCAN4 = np.array([0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15])          # raster index of every scan position (up-right diagonals)
LUMA = ["over the budget", "not over the budget", "last position 0", "last position 15", "a level >= 4", "a level >= 300"]
CHROMA = ["over the budget", "not over the budget", "last position 0", "last position 15"]


def leaf_blocks(res, W, Hh):
    """-> (luma blocks, chroma blocks) of the 4x4 CUs of the oracle's final decisions: the coded 4x4 luma block of every 4x4 CU and
    the coded Cb / Cr blocks of every 8x8 area of four 4x4 CUs (the area's chroma flags stand in each of its four entries)"""
    luma, chroma = [], []
    wc = (W + 63) // 64
    for y4 in range(Hh // 4):
        for x4 in range(W // 4):
            if int(res["cu"][y4, x4, 1]) != 2:
                continue
            x, y = x4 * 4, y4 * 4
            cbf = int(res["cu"][y4, x4, 5])
            co = res["coeff"][(y // 64) * wc + x // 64]
            lx, ly = x % 64, y % 64
            if cbf & 1:
                luma.append(co[:4096].reshape(64, 64)[ly:ly + 4, lx:lx + 4])
            if x % 8 == 0 and y % 8 == 0:
                for c in (0, 1):
                    if cbf & (2 << c):
                        chroma.append(co[4096:].reshape(2, 32, 32)[c, ly // 2:ly // 2 + 4, lx // 2:lx // 2 + 4])
    return luma, chroma


def properties(block):
    a = np.abs(block.astype(np.int64)).ravel()[SCAN4]
    last = int(np.nonzero(a)[0][-1])
    over = certainly_over_budget(block)
    return [over, not over, last == 0, last == 15, bool((a >= 4).any()), bool((a >= 300).any())]


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once, and the coverage the cases are there for."""
    res, seen_l, seen_c, cus = {}, [0] * len(LUMA), [0] * len(CHROMA), 0
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        cus += int((o["cu"][:Hh // 4, :W // 4, 1] == 2).sum())
        luma, chroma = leaf_blocks(o, W, Hh)
        for blk in luma:
            assert blk.any(), case
            for i, p in enumerate(properties(blk)):
                seen_l[i] += int(p)
        for blk in chroma:
            assert blk.any(), case
            for i, p in enumerate(properties(blk)[:len(CHROMA)]):
                seen_c[i] += int(p)
    print("4x4 CUs: %d; luma blocks %s; chroma blocks of 4x4 areas %s" % (cus, dict(zip(LUMA, seen_l)), dict(zip(CHROMA, seen_c))))
    for i, p in enumerate(LUMA):
        assert seen_l[i] > 0, ("luma", p, seen_l)
    for i, p in enumerate(CHROMA):
        assert seen_c[i] > 0, ("chroma", p, seen_c)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_on_the_leafs_counted_costs_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_on_the_leafs_counted_costs_equals_the_encoders_records(hip):
    """The P / B kernel compiles the same function: the smallest P / B golden through test_gpu_ctu_search_pb's own route (decisions,
    levels, reconstruction and every picture's three model sets); the records carry luma and chroma levels."""
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
