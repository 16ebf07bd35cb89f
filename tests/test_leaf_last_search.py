"""lf_last_search (ctu_leaf4.h): the 4x4 leaf's RDOQ searches the last significant position down the sixteen lanes of the block's
row -- the operands gathered into scan order, the candidates from the ballots of "level != 0" and "level > 1" (the walk ends at the
highest level above 1; nothing beyond the last candidate holds a level), base_cost handed a lane down for fifteen rounds with lane
15 keeping the incoming value, the sixteen totals formed once, and the choice made by rq_last_lower / rq_last_pick (ctu_core.h).
tests/emul_leaf/last_search4.cpp replays those steps lane by lane on the host, with the two functions of the choice compiled from
the kernel's header, and compares them with the serial walk the leaf ran before (descending scan positions, strict <, stop behind
the first level above 1) on random blocks: the chosen position and the best cost bit for bit, base_cost after step 0 where the walk
still reads it (no level above 1).  Every class is counted and asserted present: every last candidate 0..15, every kstop 0..15 and
none, no level at all, all levels 1, equal totals at two candidates, a total equal to the incoming best cost, zeros between levels.

Two mutants run on the same inputs and must be caught: one that prefers the LOWEST position among equal totals, and one that takes
<= against the incoming best cost."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

CASES = 400000
NAMES = {0: "cases", 1: "cases where the lanes' form differs from the walk", 2: "cases that catch the lowest-position mutant", 3: "cases that catch the <= mutant",
         4: "no level at all", 5: "all levels 1", 6: "the highest of several candidates with the same minimal total wins",
         7: "the candidates' minimum equals the incoming best cost", 8: "zeros between levels", 9: "no level above 1 (kstop: none)",
         10: "a candidate wins", 11: "best cost stays although there is a candidate", 12: "base_cost after step 0 compared"}
NAMES.update({16 + k: "last candidate at %d" % k for k in range(16)})
NAMES.update({32 + k: "kstop %d" % k for k in range(16)})


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("leaf_last_search") / "liblast_search4.so")
    src = os.path.join(H.ROOT, "tests", "emul_leaf", "last_search4.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    fn = ctypes.CDLL(out).last_search4_compare
    fn.restype = None
    fn.argtypes = [ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    return fn


def test_the_lanes_form_equals_the_walk_and_the_mutants_do_not(compare):
    counts, first = np.zeros(64, np.int64), np.zeros(100, np.float64)
    compare(21, CASES, H.ptr(counts), H.ptr(first))
    for k in sorted(NAMES):
        print("%s: %d" % (NAMES[k], counts[k]))
    assert counts[0] == CASES
    assert counts[1] == 0, ("last_sp %d base_cost %r best_cost %r lev %r c0 %r cc %r cs %r klast %r walk %d lanes %d"
                            % (int(first[0]), first[1], first[2], list(first[3:19].astype(int)), list(first[19:35]), list(first[35:51]),
                               list(first[51:67]), list(first[67:83]), int(first[83]), int(first[84])))
    # so that the comparison cannot pass on inputs that decide nothing: every class occurs
    for k in sorted(NAMES):
        if k >= 4:
            assert counts[k] > 0, NAMES[k]
    # the mutants: lowest position among equals, <= against the incoming best cost
    assert counts[2] > 0, "a pick of the lowest position among equal totals passes"
    assert counts[3] > 0, "a pick that takes a total equal to the incoming best cost passes"
