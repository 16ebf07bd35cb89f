"""The device RDOQ's fixed point starts from a rate-aware guess (rq_start_level in ctu_core.h: rdoq_wave's passes through dst, the
4x4 leaf's leaf_rdoq / leaf_rdoq_rows in the lanes' registers) instead of the quantisation candidates.  The start must not show in
the result: the device search against the oracle, per-CTU CRCs and models, on the pictures whose passes tests/test_rdoq_start.py
has counted on the host -- positions where the guess goes to 0 and the decision keeps 1, positions where the guess keeps 1 and the
decision takes 0, for every block size; passes without regular bins, which start from the candidates again; groups left to lane 0's
walk, which finds guesses in dst where the parent left candidates -- and on a 10-bit picture at QP 51.  A start that does not reach
dst, or a change measured against anything but the current level, leaves a level of the guess behind and shows in a CTU's CRC.  One
P / B sequence: its kernel compiles the same rdoq_wave."""
import os

import numpy as np
import pytest

import helpers as H
from test_gpu_ctu_search import run_gpu
from test_gpu_rdoq_group_rows import CASES as ROW_CASES
from test_rdoq_start import LOW_QP

pytestmark = pytest.mark.gpu

CASES = ROW_CASES + [LOW_QP, (64, 64, 10, 51, 3)]


@pytest.fixture(scope="module")
def oracle_results(orc):
    """The oracle's result of every case, computed once."""
    return {case: H.oracle_search_picture(orc, case[2], H.search_params(case[0], case[1], case[3]), *H.varied_picture(case[0], case[1], case[4], case[2]))
            for case in CASES}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d_%dbit_qp%d_t%d" % c)
def test_search_from_the_guessed_start_equals_the_oracle(hip, orc, oracle_results, case):
    W, Hh, depth, qp, t = case
    o = oracle_results[case]
    r = run_gpu(hip, depth, H.search_params(W, Hh, qp), [H.varied_picture(W, Hh, t, depth)])[0]
    assert np.array_equal(H.ctu_crcs(r, W, Hh), H.ctu_crcs(o, W, Hh)), case
    assert np.array_equal(r["models"], o["models"]), case


def test_pb_search_from_the_guessed_start_equals_the_encoders_records(hip):
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
