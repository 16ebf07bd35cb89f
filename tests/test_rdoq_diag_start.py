"""rdoq_diag_start (ctu_core.h): the first scan index of a diagonal of the group grid as a closed form -- the device RDOQ finds
the groups of a pass with it.  Against the diagonal scan itself, for the grids of 8x8, 16x16 and 32x32 blocks.  The function is
compiled for the host from the kernel's header (tests/emul_rdoq/diag_start.cpp, with the host emulation's flags)."""
import ctypes
import os
import subprocess

import pytest

import helpers as H


def diag(n):
    """the up-right diagonal scan of an n x n grid -> [(x, y)]: diagonals x + y ascending, each from the bottom-left upwards"""
    return [(s - y, y) for s in range(2 * n - 1) for y in range(min(s, n - 1), -1, -1) if s - y < n]


@pytest.fixture(scope="module")
def closed_form(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rdoq_diag_start") / "libdiag_start.so")
    src = os.path.join(H.ROOT, "tests", "emul_rdoq", "diag_start.cpp")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O0", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden",
                           "-Wno-unknown-pragmas", "-I" + os.path.join(H.ROOT, "uvg266_amd", "csrc"), "-o", out, src])
    return ctypes.CDLL(out).rdoq_diag_start_host


@pytest.mark.parametrize("n", [2, 4, 8])
def test_the_closed_form_is_where_the_scan_starts_a_diagonal(closed_form, n):
    order = diag(n)
    for d in range(2 * n - 1):
        assert closed_form(n, d) == min(i for i, (x, y) in enumerate(order) if x + y == d), (n, d)
    # ... and every position lies inside its own diagonal's range
    for i, (x, y) in enumerate(order):
        s = closed_form(n, x + y)
        assert s <= i < s + min(x + y, 2 * n - 2 - x - y) + 1, (n, i)
