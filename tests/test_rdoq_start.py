"""rq_start_level (ctu_core.h): the device's RDOQ decides a pass's positions by a fixed-point iteration, and since this change the
iteration starts from a rate-aware guess -- a candidate of 1 that a neutral context would drop starts at 0 -- instead of the
candidates.  The fixed point does not depend on its start; the number of rounds does.  Both statements are checked here on the host:
tests/emul/ctu_emul.cpp is built with -DCTU_RDOQ_START_STATS (ctu_rdoq_emul.h), which runs, beside the serial walk, a plain
transcription of the device's iteration (rdoq_wave's passes of up to four groups of a diagonal, the 4x4 leaf's one group) on
rdoq_decide_at from four starts: the candidates, the guess as the device places it, all zeros, a seeded random start <= candidate.
Every start of every group has to end at the walk's levels; the rounds of a pass (the maximum over its groups) are counted per
block size and colour class, and so are the positions where the guess was wrong in either direction -- both kinds have to occur for
every block size, so that tests/test_gpu_rdoq_start.py cannot pass on inputs where the start does not matter.

Rounds summed over the passes, start = candidates -> start = guess, as printed by this test (luma + chroma of a size):
  448x256 bench picture, QP 22: see test_the_guess_needs_fewer_rounds_on_the_bench_picture's output (asserted: fewer for every size)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from test_gpu_rdoq_group_rows import CASES

# (W, H, depth, QP, t of H.varied_picture)
LOW_QP = (64, 64, 8, 2, 2005)          # 8 bit, QP <= 7: the regular-bin budget ends inside groups (lane 0's walk on the device)
BENCH = (448, 256, 8, 22, 0)           # layout.synthetic_yuv420(448, 256, 0, 8): the bench's content at its QP
FIELDS = ["passes", "rounds from the candidates", "rounds from the guess", "rounds from zeros", "rounds from a random start", "starts that end elsewhere",
          "guess 0, decision 1", "guess 1, decision 0", "last positions with candidate 1", "passes of 1 round from the guess", "passes of 2 rounds",
          "passes of 3 or more rounds", "passes left to the serial walk (the budget may end inside)"]
CLASSES = ["%s %d" % (c, n) for n in (4, 8, 16, 32) for c in ("luma", "chroma")]


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    """the host emulation with the statistics hook, built for this module only"""
    out = str(tmp_path_factory.mktemp("rdoq_start") / "libctu_emul_start.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-DCTU_RDOQ_START_STATS", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"),
                           "-I" + os.path.join(H.ROOT, "include"), "-o", out, os.path.join(H.ROOT, "tests", "emul", "ctu_emul.cpp")])
    return ctypes.CDLL(out)


def run(emul, case):
    """-> (the picture's result, statistics [class, field])"""
    W, Hh, depth, qp, t = case
    prm = H.search_params(W, Hh, qp)
    wc, hc = (W + 63) // 64, (Hh + 63) // 64
    px = H.px_dtype(depth)
    y, u, v = (np.ascontiguousarray(a, px) for a in H.varied_picture(W, Hh, t, depth))
    ry, ru, rv = np.zeros((Hh, W), px), np.zeros((Hh // 2, W // 2), px), np.zeros((Hh // 2, W // 2), px)
    scu = np.zeros(hc * 16 * wc * 16, H.SCU_NP)
    co = np.zeros(wc * hc * 6144, np.int16)
    mo = np.zeros(wc * hc * 3 * H.N_MODELS, np.uint32)
    cp = H.ctu_params(prm)
    emul.ctu_emul_set_lazy(0)
    emul.ctu_emul_rdoq_start_stats(None, 1)
    assert emul.ctu_emul_search_picture(depth, ctypes.byref(cp), H.ptr(y), H.ptr(u), H.ptr(v), H.ptr(ry), H.ptr(ru), H.ptr(rv), H.ptr(scu), H.ptr(co), H.ptr(mo)) == 0
    st = np.zeros((8, len(FIELDS)), np.int64)
    emul.ctu_emul_rdoq_start_stats(H.ptr(st), 1)
    return H.search_result_from_device_layout(W, Hh, ry, ru, rv, scu, co, mo), st


def show(case, st):
    print("%dx%d %d bit QP %d t %d" % case)
    for k, c in enumerate(CLASSES):
        if st[k, 0]:
            print("  %-10s" % c + "; ".join("%s %d" % (f, st[k, j]) for j, f in enumerate(FIELDS)))


@pytest.fixture(scope="module")
def small(emul):
    """the statistics of the small pictures, taken once"""
    return {case: run(emul, case) for case in CASES + [LOW_QP]}


def test_the_hook_leaves_the_emulation_as_it_is(small):
    case = CASES[0]
    W, Hh, depth, qp, t = case
    want = H.emul_search_picture(depth, H.search_params(W, Hh, qp), *H.varied_picture(W, Hh, t, depth))
    got = small[case][0]
    assert np.array_equal(H.ctu_crcs(got, W, Hh), H.ctu_crcs(want, W, Hh))


def test_every_start_ends_at_the_walks_levels(small):
    total = np.zeros((8, len(FIELDS)), np.int64)
    for case, (_, st) in small.items():
        show(case, st)
        assert st[:, 0].sum() > 0, case
        assert st[:, 5].sum() == 0, (case, st[:, 5])
        total += st
    by_size = total.reshape(4, 2, -1).sum(axis=1)
    for k, n in enumerate((4, 8, 16, 32)):
        # both kinds of wrong guess, and a last position that the device's guess may have lowered, for every size
        assert by_size[k, 6] > 0 and by_size[k, 7] > 0 and by_size[k, 8] > 0, (n, by_size[k])


def test_the_low_qp_picture_has_groups_on_the_serial_path(small):
    st = small[LOW_QP][1]
    assert st[2:, 12].sum() > 0 and st[2:, 0].sum() > 0


def test_the_guess_needs_fewer_rounds_on_the_bench_picture(emul):
    _, st = run(emul, BENCH)
    show(BENCH, st)
    assert st[:, 5].sum() == 0
    by_size = st.reshape(4, 2, -1).sum(axis=1)
    for k, n in enumerate((4, 8, 16, 32)):
        print("  size %d: %d passes, %d rounds from the candidates (%.2f a pass), %d from the guess (%.2f): %+.0f %%" % (
            n, by_size[k, 0], by_size[k, 1], by_size[k, 1] / by_size[k, 0], by_size[k, 2], by_size[k, 2] / by_size[k, 0],
            100.0 * (by_size[k, 2] - by_size[k, 1]) / by_size[k, 1]))
        assert by_size[k, 2] < by_size[k, 1], n
