"""rdoq_wave's sums in scan order (ctu_core.h: the tail behind the last candidate, a group's accumulation and statistics, the
last-position search) run as unrolled steps on owner-masked values with the integers taken from ballots: the device search against
the oracle on 128x128 pictures whose decided luma blocks of 8, 16 and 32 meet every path of those sums.  A slip in a sum changes a
level or a decision and shows in a CTU's CRC or in its models.  One P / B sequence: its kernel compiles the same rdoq_wave."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu
from test_gpu_coder_models_only import CASES, certainly_over_budget, transform_blocks

pytestmark = pytest.mark.gpu

SIZES = [8, 16, 32]
# what a decided block's levels say of the sums that produced them
PATHS = ["last position in group 0",                    # the register path (cg_last == 0)
         "last position beyond group 0",
         "a group without levels below the last group",  # the group flag and the zero-out arithmetic
         "all levels <= 1",                              # the last-position walk runs down to position 0
         "a level > 1",                                  # it stops early
         "certainly over the regular-bin budget",
         "certainly not over it"]
MIDDLE = "last position in neither group 0 nor the top group"      # whole groups in the tail loop (luma 8 and 32)


def diag(n):
    """the up-right diagonal scan of an n x n grid -> [(x, y)]: diagonals x + y ascending, each from the bottom-left upwards"""
    return [(s - y, y) for s in range(2 * n - 1) for y in range(min(s, n - 1), -1, -1) if s - y < n]


def scan_of(n):
    """raster index of every scan position of an n x n block: 4x4 groups in diagonal order, a group's 16 positions likewise"""
    return np.array([(gy * 4 + y) * n + gx * 4 + x for gx, gy in diag(n // 4) for x, y in diag(4)])


def paths_of(block):
    """-> the set of PATHS (and MIDDLE) a coded block's levels stand for"""
    n = block.shape[0]
    a = np.abs(block.astype(np.int64)).ravel()[scan_of(n)]
    last = int(np.flatnonzero(a)[-1])
    cg_last, groups = last >> 4, a.reshape(-1, 16).any(axis=1)
    got = {PATHS[0] if cg_last == 0 else PATHS[1], PATHS[3] if a.max() <= 1 else PATHS[4],
           PATHS[5] if certainly_over_budget(block) else PATHS[6]}
    if not groups[1:cg_last].all():
        got.add(PATHS[2])
    if 0 < cg_last < n * n // 16 - 1:
        got.add(MIDDLE)
    return got


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once; the coverage the cases are there for is asserted here, on the oracle's
    result, before any comparison."""
    res, seen = {}, {n: set() for n in SIZES}
    for case in CASES:
        W, Hh, depth, qp, t = case
        o = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
        res[case] = o
        for name, blk in transform_blocks(o, W, Hh):
            if name.startswith("luma"):
                seen[blk.shape[0]] |= paths_of(blk)
    for n in SIZES:
        for p in PATHS + ([MIDDLE] if n != 16 else []):
            assert p in seen[n], (n, p)
    return res


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_with_the_unrolled_sums_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_with_the_unrolled_sums_equals_the_encoders_records(hip):
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
