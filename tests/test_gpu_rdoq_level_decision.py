"""The level decision of RDOQ on the device is coded_level2 (ctu_core.h: straight-line code, both candidates from four paired table
reads) at every call site -- the 4x4 leaf's leaf_rdoq / leaf_rdoq_rows, rdoq_wave's fixed point and its lane-0 walk: the device search
against the oracle on 128x128 pictures whose decided blocks meet the decision in every block class, with levels of every class of
its rate (1; 2 or 3; 4..8: the Rice code; >= 9: towards the exp-Golomb code) on both sides of the regular-bin budget.  A slip
changes a level or a cost and shows in a CTU's CRC or in its models.  One P / B sequence: its kernel compiles the same functions."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu
from test_gpu_coder_models_only import CASES as MODEL_CASES, certainly_over_budget, transform_blocks

pytestmark = pytest.mark.gpu

ADDED = (128, 128, 10, 7, 5)          # the 10-bit case of MODEL_CASES decides no 4x4 CU
CASES = MODEL_CASES + [ADDED]
CLASSES = ["luma 4 of a 4x4 CU", "chroma 4 of a 4x4 area", "chroma 4 of an 8x8 CU", "luma 8", "luma 16", "luma 32", "luma 32 of a 64x64 CU", "chroma 8", "chroma 16"]
MARKS = ["a level 1", "a level 2 or 3", "a level 4..8", "a level >= 9", "certainly over the regular-bin budget", "certainly not over it"]


def leaf_blocks(res, W, Hh):
    """-> [(class name, levels)] of every transform block with levels of the 4x4 CUs, from the oracle's cu and coeff: a luma block per
    CU, a Cb and a Cr block per 8x8 area"""
    out = []
    wc = (W + 63) // 64
    for y in range(0, Hh, 8):
        for x in range(0, W, 8):
            if int(res["cu"][y // 4, x // 4, 1]) != 2:
                continue
            co = res["coeff"][(y // 64) * wc + x // 64]
            lx, ly = x % 64, y % 64
            for dy in (0, 4):
                for dx in (0, 4):
                    out.append((CLASSES[0], co[:4096].reshape(64, 64)[ly + dy:ly + dy + 4, lx + dx:lx + dx + 4]))
            for c in (0, 1):
                out.append((CLASSES[1], co[4096:].reshape(2, 32, 32)[c, ly // 2:ly // 2 + 4, lx // 2:lx // 2 + 4]))
    return [(name, blk) for name, blk in out if blk.any()]


def marks_of(block):
    a = np.abs(block.astype(np.int64))
    got = {MARKS[5 - certainly_over_budget(block)]}
    for k, m in enumerate([a == 1, (a == 2) | (a == 3), (a >= 4) & (a <= 8), a >= 9]):
        if m.any():
            got.add(MARKS[k])
    return got


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once; what the cases are there for is asserted here, on the oracle's result,
    before any comparison."""
    res, seen, seen_added = {}, {c: set() for c in CLASSES}, {c: set() for c in CLASSES}
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        for name, blk in leaf_blocks(o, W, Hh) + transform_blocks(o, W, Hh):
            (seen_added if case == ADDED else seen)[name] |= marks_of(blk)
    for c in CLASSES:          # MODEL_CASES alone: all 54 combinations
        for m in MARKS:
            assert m in seen[c], (c, m)
    for m in MARKS:            # the added case: 10-bit 4x4 CUs
        assert m in seen_added[CLASSES[0]], (ADDED, CLASSES[0], m)
    for m in (MARKS[0], MARKS[1], MARKS[2], MARKS[5]):
        assert m in seen_added[CLASSES[1]], (ADDED, CLASSES[1], m)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_with_the_straight_line_decision_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_with_the_straight_line_decision_equals_the_encoders_records(hip):
    """The P / B kernel's copies of the decision: the smallest P / B golden through test_gpu_ctu_search_pb's own route; the records
    carry luma and chroma levels."""
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
