"""rq_last_lower / rq_last_pick (ctu_core.h): the device RDOQ's last-position search forms a group's sixteen totals in their lanes
and chooses among them by a reduction -- the lowest total, among equal totals the highest position, and nothing unless the lowest
is strictly below the incoming best cost.  Both functions are compiled for the host from the kernel's header
(tests/emul_rdoq/last_pick.cpp, with the host emulation's flags), reduced in the order of the device's lanes and compared with the
reference's walk (descending positions, strict <) on random totals and on inputs built to tie: equal totals at several positions, a
total equal to the incoming best cost, every kstop (the highest level above 1: the walk's end), no candidate, one candidate.

Two mutants run on the same inputs and must be caught: one that prefers the LOWEST position among equal totals, and one that takes
<= against the incoming best cost."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NAMES = ["cases", "cases where the reduction differs from the walk", "best cost stays", "a candidate wins", "the highest of several equal minimal totals wins",
         "the candidates' minimum equals the incoming best cost", "no candidate", "one candidate", "cases that catch the lowest-position mutant",
         "cases that catch the <= mutant"] + ["kstop %d" % k for k in range(16)] + ["the winner is not the highest candidate"]


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rdoq_last_pick") / "liblast_pick.so")
    src = os.path.join(H.ROOT, "tests", "emul_rdoq", "last_pick.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    fn = ctypes.CDLL(out).last_pick_compare
    fn.restype = None
    fn.argtypes = [ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    return fn


def test_the_reduction_equals_the_walk_and_the_mutants_do_not(compare):
    counts, first = np.zeros(32, np.int64), np.zeros(19, np.float64)
    compare(17, 400000, H.ptr(counts), H.ptr(first))
    for k, nm in enumerate(NAMES):
        print("%s: %d" % (nm, counts[k]))
    assert counts[0] == 400000
    assert counts[1] == 0, "cand %#x best_cost %r totals %r kstop %d" % (int(first[0]), first[1], list(first[2:18]), int(first[18]))
    # so that the comparison cannot pass on inputs that decide nothing: every outcome and every kstop occurs
    for k in list(range(2, 8)) + list(range(10, 27)):
        assert counts[k] > 0, NAMES[k]
    # the mutants: lowest position among equals, <= against the incoming best cost
    assert counts[8] > 0, "a pick of the lowest position among equal totals passes"
    assert counts[9] > 0, "a pick that takes a total equal to the incoming best cost passes"
