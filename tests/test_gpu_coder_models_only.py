"""The coder's pass over a decided CTU adapts the context models and counts nothing (coeff_bits<PX, false>, ctu_core.h): the device
search against the oracle on 128x128 pictures chosen so that the pass meets every transform block shape -- luma 8 / 16 / 32, the four
32x32 blocks of a 64x64 CU, chroma 4 (of an 8x8 CU) / 8 / 16 -- each with levels on both sides of the regular-bin budget.  All three
model sets are compared: a slip of the counting paths (the search's RD costs) shows as well as one of the pass.  One P / B sequence
holds coder_pass_pb's calls."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu

pytestmark = pytest.mark.gpu

# (W, H, depth, QP, t of H.varied_picture)
CASES = [(128, 128, 8, 7, 5),          # luma 8 / 16 / 32 and a 64x64 CU's blocks over the budget; chroma with levels, none over
         (128, 128, 8, 7, 2005),       # chroma 4x4 of 8x8 CUs, 8x8 and 16x16 over the budget
         (128, 128, 8, 12, 1005),      # the budget ending inside some blocks only
         (128, 128, 8, 22, 5),         # every size with levels, none over; blocks without levels
         (128, 128, 10, 12, 2005),     # 10 bit
         (128, 128, 8, 42, 1005)]      # 64x64 CUs, sparse levels, empty chroma blocks
SHAPES = ["luma 8", "luma 16", "luma 32", "luma 32 of a 64x64 CU", "chroma 4 of an 8x8 CU", "chroma 8", "chroma 16"]


def certainly_over_budget(block):
    """A lower bound of the regular bins of a block's levels (a greater-1 flag per level, parity and greater-2 per level above 1)
    against the budget of 28 bins per 16 coefficients."""
    a = np.abs(block.astype(np.int64))
    return int(((a != 0) + 2 * (a > 1)).sum()) > block.size * 28 // 16


def transform_blocks(res, W, Hh):
    """-> [(shape name, levels)] of every coded transform block of 8x8 and larger CUs, from the oracle's cu and coeff"""
    out = []
    wc = (W + 63) // 64
    for y4 in range(Hh // 4):
        for x4 in range(W // 4):
            n = 1 << int(res["cu"][y4, x4, 1])
            x, y = x4 * 4, y4 * 4
            if n < 8 or x % n or y % n:
                continue
            tn = min(n, 32)
            for ty in range(y, y + n, tn):
                for tx in range(x, x + n, tn):
                    cbf = int(res["cu"][ty // 4, tx // 4, 5])
                    co = res["coeff"][(ty // 64) * wc + tx // 64]
                    lx, ly = tx % 64, ty % 64
                    if cbf & 1:
                        out.append(("luma 32 of a 64x64 CU" if n == 64 else "luma %d" % tn, co[:4096].reshape(64, 64)[ly:ly + tn, lx:lx + tn]))
                    for c in (0, 1):
                        if cbf & (2 << c):
                            cw = tn // 2
                            name = "chroma 4 of an 8x8 CU" if n == 8 else "chroma %d" % cw
                            out.append((name, co[4096:].reshape(2, 32, 32)[c, ly // 2:ly // 2 + cw, lx // 2:lx // 2 + cw]))
    return out


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once; the coverage the cases are there for is asserted here, on the oracle's
    result, before any comparison: every shape with levels, at least once certainly over the budget and at least once not."""
    res, seen = {}, {s: [0, 0] for s in SHAPES}
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        for name, blk in transform_blocks(o, W, Hh):
            assert blk.any(), (case, name)
            seen[name][certainly_over_budget(blk)] += 1
    for s in SHAPES:
        assert seen[s][0] > 0 and seen[s][1] > 0, (s, seen)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_models_after_the_coders_pass_equal_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_coders_pass_equals_the_encoders_records(hip):
    """coder_pass_pb's calls: the smallest P / B golden through test_gpu_ctu_search_pb's own route, every picture's three model sets
    among what is compared; the records carry luma and chroma levels."""
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
