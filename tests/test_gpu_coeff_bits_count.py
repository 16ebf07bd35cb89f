"""The counting variant of coeff_bits (coeff_bits<PX, true>, ctu_core.h: the bit count behind every RD cost of a block of 8x8 and up)
on the unrolled, packed sweep: the device search against the oracle on 128x128 pictures.  The search's own models are what the
counting variant adapts with update = 1, and the decisions are what its sums feed, so the CTUs' CRCs (partition, modes, levels,
reconstruction) and all three model sets are compared.  The shapes the function counts are luma 8 / 16 / 32, the 32x32 luma and
16x16 chroma blocks of a 64x64 CU (counted with update = 0) and chroma 8 / 16; the cases are chosen so that each of them occurs
certainly over the regular-bin budget and not, with all its levels in the first coefficient group and with its last level in the
block's final group, and with a group without levels between coded groups -- asserted on the oracle's result, on the final decisions'
blocks (a lower bound of what the search counts), before anything is compared.  One P / B sequence holds the P / B kernel's copy.

No test here can see a sum that is off without flipping a decision: for that stand the comparison of `bench.py --dump-outputs`
against the parent's and the full-size goldens of the suite (every CU of the 1080p and 2160p records)."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_coder_models_only import CASES as MODELS_ONLY_CASES, certainly_over_budget
from test_gpu_ctu_search import run_gpu

pytestmark = pytest.mark.gpu

# (W, H, depth, QP, t of H.varied_picture)
CASES = MODELS_ONLY_CASES + [(128, 128, 8, 27, 5)]
SHAPES = ["luma 8", "luma 16", "luma 32", "luma 32 of a 64x64 CU", "chroma 16 of a 64x64 CU", "chroma 8", "chroma 16"]
PROPS = ["over the budget", "not over the budget", "all levels in the first group", "last level in the final group",
         "a group without levels between coded groups"]


def scan_of(orc, n):
    """raster index of every scan position of an n x n block, from the oracle's own tables"""
    scan, scg = np.zeros(n * n, np.uint32), np.zeros(n * n // 16, np.uint32)
    orc.lib.orc8_rdoq_scans(n, n, H.ptr(scan), H.ptr(scg))
    return scan


def counted_blocks(res, W, Hh):
    """-> [(shape name, levels)] of every coded transform block that the counting variant prices (CUs of 8x8 and up; the 4x4 chroma
    blocks of an 8x8 CU are coeff_bits4r's), from the oracle's cu and coeff"""
    out = []
    wc = (W + 63) // 64
    for y4 in range(Hh // 4):
        for x4 in range(W // 4):
            n = 1 << int(res["cu"][y4, x4, 1])
            x, y = x4 * 4, y4 * 4
            if n < 8 or x % n or y % n:
                continue
            tn = min(n, 32)
            of64 = " of a 64x64 CU" if n == 64 else ""
            for ty in range(y, y + n, tn):
                for tx in range(x, x + n, tn):
                    cbf = int(res["cu"][ty // 4, tx // 4, 5])
                    co = res["coeff"][(ty // 64) * wc + tx // 64]
                    lx, ly = tx % 64, ty % 64
                    if cbf & 1:
                        out.append(("luma %d" % tn + of64, co[:4096].reshape(64, 64)[ly:ly + tn, lx:lx + tn]))
                    cw = tn // 2
                    for c in (0, 1):
                        if cbf & (2 << c) and cw >= 8:
                            out.append(("chroma %d" % cw + of64, co[4096:].reshape(2, 32, 32)[c, ly // 2:ly // 2 + cw, lx // 2:lx // 2 + cw]))
    return out


def properties(block, scan):
    """which of PROPS a block's levels have"""
    a = np.abs(block.astype(np.int64)).ravel()[scan]
    groups = a.reshape(-1, 16).any(axis=1)
    last = int(np.nonzero(a)[0][-1])
    over = certainly_over_budget(block)
    return [over, not over, last < 16, last >= a.size - 16, bool((~groups[1:last >> 4]).any())]


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once, and the coverage the cases are there for."""
    scans = {n: scan_of(orc, n) for n in (8, 16, 32)}
    res, seen = {}, {s: [0] * len(PROPS) for s in SHAPES}
    whole64 = lost64 = 0
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        for name, blk in counted_blocks(o, W, Hh):
            assert blk.any(), (case, name)
            for i, p in enumerate(properties(blk, scans[blk.shape[0]])):
                seen[name][i] += int(p)
        # a CTU whose first 32x32 area ends as one CU had the 64x64 candidate tried against its split (combine_intra_cus) and lost
        first = o["cu"][0:Hh // 4:16, 0:W // 4:16, 1]
        whole64 += int((first == 6).sum())
        lost64 += int((first == 5).sum())
    for s in SHAPES:
        for i, p in enumerate(PROPS):
            assert seen[s][i] > 0, (s, p, seen)
    assert whole64 > 0 and lost64 > 0, (whole64, lost64)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_on_the_counted_costs_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_on_the_counted_costs_equals_the_encoders_records(hip):
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
