"""coeff_bits4r (ctu_leaf4.h) counts a 4x4 block's coefficient bits on the packed sweep: the sixteen position lanes pack one key word
each (lf4_key: the sig / greater-1 / parity / greater-2 bytes, context << 1 | bin, 0xff where the position codes no such bin,
0xffffffff beyond the last position and behind the budget's end), every model lives in a lane (lf4_lane_model) and steps through the
key words in coding order (cb_step).  tests/emul_leaf/coeff_bits_keys.cpp compiles both functions and cb_idx / cb_rpk / cb_addpk /
cb_step's host form from the kernel's header, replays the sweep lane by lane and compares the sum (in units of 2^-15) and ALL models
with coeff_bits_serial, for luma and for chroma: every last position 0..15, the levels 1, 2, 3, 4, 5, 300 and +-32767, blocks whose
budget of 28 regular bins ends at every scan position it can end at (a position spends four bins at most and the last one three, so
seven positions pass before it ends: -1, that is never, and 0..8), blocks with all sixteen levels set, random blocks.

Two mutants of the key word run on the same inputs and must be caught: the parity byte not gated by a > 1, and the greater-2 bin
taken at a >= 3."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

PER_TYPE = ["last position %d" % k for k in range(16)] + ["a level of |%d|" % v for v in (1, 2, 3, 4, 5, 300)] + ["a level of 32767", "a level of -32767"] + \
           ["the budget ends at scan position %d" % k for k in range(-1, 9)] + \
           ["the budget walk ran and the budget held", "all sixteen levels set", "random blocks", "two and more bins on one model", "a bypass-coded position with level 0"]
CASES = 300000


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("leaf_coeff_bits_keys") / "libleaf_coeff_bits_keys.so")
    src = os.path.join(H.ROOT, "tests", "emul_leaf", "coeff_bits_keys.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    fn = ctypes.CDLL(out).leaf_coeff_bits_compare
    fn.restype = None
    fn.argtypes = [ctypes.c_uint64, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]
    return fn


def test_the_packed_sweep_equals_the_serial_walk_and_the_mutants_do_not(compare):
    counts, first = np.zeros(128, np.int64), np.zeros(20, np.float64)
    compare(29, CASES, H.ptr(counts), H.ptr(first))
    print("cases %d, differing %d, caught by the parity mutant %d, by the greater-2 mutant %d" % tuple(counts[:4]))
    for t, nm in enumerate(("luma", "chroma")):
        for i, p in enumerate(PER_TYPE):
            print("%s, %s: %d" % (nm, p, counts[8 + 56 * t + i]))
    assert counts[0] == CASES
    assert counts[1] == 0, "colour %d levels %r serial %r replay %r (case %d)" % (int(first[0]), [int(v) for v in first[1:17]], first[17], first[18], int(first[19]))
    # so that the comparison cannot pass on inputs that decide nothing: every class occurs, for luma and for chroma
    for t, nm in enumerate(("luma", "chroma")):
        for i, p in enumerate(PER_TYPE):
            assert counts[8 + 56 * t + i] > 0, (nm, p)
    assert counts[2] > 0, "a parity byte that is not gated by a > 1 passes"
    assert counts[3] > 0, "a greater-2 bin taken at a >= 3 passes"
