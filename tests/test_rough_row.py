"""ang_row8 / make_ang_mode (intra_pred_dev.h): the branch-free angular row of eight samples that the device's rough search predicts
with (ctu_core.h rough_costs), against predict_row<8> on make_mode_info -- every mode 2..66, every row and tile column of 8x8, 16x16
and 32x32 blocks, 8 and 10 bit, on random, constant and alternating reference rows.  Both are compiled for the host from the
kernel's header (tests/emul_rough/rough_row.cpp).  The four reference arrays are filled independently of one another, so a wrong
choice between the smoothed and the plain rows shows."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

NAMES = ["rows", "rows that differ", "tap sums outside [0, maxv]", "samples from the projected side reference", "samples changed by the angular PDPC",
         "samples changed by the pure modes' PDPC", "rows from the smoothed references"]


@pytest.fixture(scope="module")
def compare(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rough_row") / "librough_row.so")
    src = os.path.join(H.ROOT, "tests", "emul_rough", "rough_row.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    fn = ctypes.CDLL(out).rough_row_compare
    fn.restype = None
    return fn


def fills(n, maxv):
    """-> (name, [top, left, ftop, fleft]), 4 n + 8 entries each"""
    m = 4 * n + 8
    rng = np.random.default_rng(1000 * n + maxv)
    for k in range(6):
        yield "random %d" % k, [rng.integers(0, maxv + 1, m).astype(np.uint16) for _ in range(4)]
    yield "all 0", [np.zeros(m, np.uint16) for _ in range(4)]
    yield "all maxv", [np.full(m, maxv, np.uint16) for _ in range(4)]
    alt = (np.arange(m) & 1).astype(np.uint16) * maxv
    yield "alternating", [alt.copy(), (maxv - alt).astype(np.uint16), (maxv - alt).astype(np.uint16), alt.copy()]
    # steep steps: where the cubic taps overshoot most
    step = ((np.arange(m) // 3) & 1).astype(np.uint16) * maxv
    yield "steps", [step.copy(), np.roll(step, 1), np.roll(step, 2), (maxv - step).astype(np.uint16)]


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("n", [8, 16, 32])
def test_the_row_equals_predict_row(compare, n, maxv):
    total = np.zeros(7, np.int64)
    for name, rows in fills(n, maxv):
        counts, first = np.zeros(7, np.int64), np.full(4, -1, np.int32)
        compare(n, maxv, *(H.ptr(r) for r in rows), H.ptr(counts), H.ptr(first))
        assert counts[0] == 65 * n * (n // 8)
        assert counts[1] == 0, (n, maxv, name, "mode %d row %d column %d + %d" % tuple(first))
        total += counts
    for k in range(2, 7):
        print("%dx%d, maxv %d: %s: %d" % (n, n, maxv, NAMES[k], total[k]))
        if k == 2 and n == 32:
            # the distance threshold of 32x32 blocks is 0 (kDistThres): every fractional angle takes the smoothing taps, which are
            # all positive and sum to 64 -- only the cubic taps can leave the range, and a 32x32 block never has them at a phase
            # other than 0
            assert total[k] == 0
        else:
            assert total[k] > 0, (n, maxv, NAMES[k])
