"""rdoq_wave's last-position search (ctu_core.h) keeps base_cost as a chain that runs down the owners' lanes, forms a group's
sixteen totals once, each in its lane, and chooses among them by a reduction (rq_last_lower / rq_last_pick): the device search
against the oracle on the eight 128x128 pictures of test_gpu_rdoq_group_rows.py, whose decided blocks meet the sums in every shape
the code treats differently -- per block shape, the last position in group 0 (the numbers stay in registers) and beyond it (the
cost arrays: LDS for 8x8, the workgroup's scratch above), groups without levels (skipped by their flag), walks that run down to
position 0 and walks that stop at a level above 1, both sides of the regular-bin budget, a last group that is neither the first nor
the top one; and the passes of test_gpu_rdoq_group_rows.py, whose groups hand their numbers to the sums.  A slip in base_cost, a
total or the choice moves a last position, which shows in a CTU's CRC or in its models.  The 10-bit case is the slim build's path.
(The P / B kernel keeps the uniform walk of this search -- ctu_core.h says why -- and the neighbouring files test it.)"""
import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu
from test_gpu_coder_models_only import transform_blocks
from test_gpu_rdoq_scan_sums import MIDDLE, PATHS, paths_of as sum_paths_of
from test_gpu_rdoq_group_rows import CASES, WANTED, paths_of as row_paths_of

pytestmark = pytest.mark.gpu

SUM_SHAPES = ["luma 8", "luma 16", "luma 32", "chroma 8", "chroma 16"]
CU64 = "luma 32 of a 64x64 CU"
ALL_LE1 = "all levels <= 1"          # (no 64x64 CU of these pictures keeps a luma block of levels <= 1 only: absent from that shape alone)


def check_coverage(results):
    """The predicates the cases are there for, on the oracle's results: test_gpu_rdoq_scan_sums.PATHS and MIDDLE per shape,
    test_gpu_rdoq_group_rows.WANTED."""
    assert ALL_LE1 in PATHS
    sums, rows = {s: set() for s in SUM_SHAPES + [CU64]}, {s: set() for s in SUM_SHAPES + [CU64]}
    for case, o in results.items():
        W, Hh = case[0], case[1]
        for name, blk in transform_blocks(o, W, Hh):
            if name in sums:
                sums[name] |= sum_paths_of(blk)
                rows[name] |= row_paths_of(blk)
    for s in SUM_SHAPES:
        for p in PATHS + [MIDDLE]:
            assert p in sums[s], (s, p)
    for p in PATHS + [MIDDLE]:
        if p != ALL_LE1:
            assert p in sums[CU64], (CU64, p)
    for p, shapes in WANTED.items():
        for s in shapes:
            assert p in rows[s], (s, p)


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once; the coverage is asserted here, before any comparison."""
    res = {}
    for case in CASES:
        W, Hh, depth, qp, t = case
        res[case] = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
    check_coverage(res)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_with_the_last_position_chosen_by_reduction_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case

