"""coded_level2 (ctu_core.h): the level decision of RDOQ as straight-line code -- both candidates priced from four paired table reads,
the escape code's length in closed form -- which the device's call sites run, against coded_level + ic_rate, the transcription of
uvg_get_coded_level / uvg_get_ic_rate that the host emulation's rdoq_serial keeps.  Both are compiled for the host from the kernel's
header (tests/emul_rdoq/level_decision.cpp, with the host emulation's flags) and compared on level, coded_cost and coded_cost_sig as
64-bit patterns over: luma and chroma, last 0 / 1, reg_bins 0 / 4, go_rice 0..3, every ctx_sig and ctx_set of the type, q_bits
14..20, candidates 0..5 with every context pair, 6..70 and the changes of the escape code's length up to the prefix cap (and 32 767
and beyond where q_bits lets the quantiser reach them), level_double across the candidate's whole rounding interval."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NAMES = ["decisions", "decisions that differ", "candidate kept", "candidate lowered by one", "'not significant' chosen", "exp-Golomb escape codes (q >= 5)",
         "escape codes with the prefix at its cap", "decisions of a last position", "bypass-priced decisions"]
QUANT_SCALES = [26214, 23302, 20560, 18396, 16384, 14564]


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rdoq_level_decision") / "liblevel_decision.so")
    src = os.path.join(H.ROOT, "tests", "emul_rdoq", "level_decision.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    fn = ctypes.CDLL(out).level_decision_compare
    fn.restype = None
    fn.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    return fn


def tables():
    """-> (name, 2 * 244 bin costs).  A bin costs between nearly nothing and some 7.5 bits in 1 / 32768 bit (kEntropyBits)."""
    yield "all zero", np.zeros(488, np.uint32)
    yield "all equal", np.full(488, 40000, np.uint32)
    yield "random", np.random.default_rng(16).integers(0, 1 << 18, 488).astype(np.uint32)


def qp_numbers(qp):
    """lambda and error_scale as the search has them at a QP: an 8-bit 8x8 block (transform shift 4) of an intra picture"""
    q = QUANT_SCALES[qp % 6]
    return 0.57 * 2.0 ** ((qp - 12) / 3.0), 32768.0 / 2.0 ** 8 / q / q


@pytest.mark.parametrize("qp", [0, 22, 51])
def test_the_straight_line_decision_equals_coded_level(compare, qp):
    lam, escale = qp_numbers(qp)
    total = np.zeros(9, np.int64)
    for name, tab in tables():
        counts, first = np.zeros(9, np.int64), np.zeros(12, np.int64)
        compare(H.ptr(tab), lam, escale, H.ptr(counts), H.ptr(first))
        assert counts[1] == 0, (qp, name, "t %d last %d reg_bins %d go_rice %d ctx_sig %d ctx_set %d q_bits %d level_double %d max_abs_level %d: "
                                "level %d, straight-line %d (cost differs: %d)" % tuple(first))
        total += counts
    for k, nm in enumerate(NAMES):
        print("QP %d: %s: %d" % (qp, nm, total[k]))
    assert total[0] > 3000000
    # so that the comparison cannot pass on inputs that decide nothing: each outcome and both long forms of the escape code occur
    for k in (2, 3, 4, 5, 6, 7, 8):
        assert total[k] > 0, (qp, NAMES[k])
    assert total[7] < total[0] and total[8] < total[0]
