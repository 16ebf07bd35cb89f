"""The filter stage's hand-out order (uvg266_amd/csrc/ctu_ticket.h, built for the host by tests/emul_ticket): ticket -> (picture, CTU row, CTU
column) of a launch over the CTU rows [row0, row1) of n pictures.  A wrong order is a workgroup that waits for a CTU no running workgroup
will take -- a hang on the device, so the order is held here, on the CPU, for every band of a spread of picture shapes."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emul():
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emul_ticket", "_build", "libticket_emul.so"))
    lib.ticket_emul_order.restype = ctypes.c_int
    lib.ticket_emul_order.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p]
    lib.ticket_emul_one.restype = None
    lib.ticket_emul_one.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    return lib


def order(lib, wc, row0, row1, n):
    out = np.full((wc * (row1 - row0) * n, 3), -7, np.int32)
    assert lib.ticket_emul_order(wc, row0, row1, n, out.ctypes.data) == len(out)
    return [tuple(int(v) for v in r) for r in out]


def whole_picture_order(wc, hc, n):
    """The order the whole-picture launch has always had, restated: diagonal by diagonal (d = cx + cy); inside a diagonal picture by picture;
    inside a picture by ascending row."""
    seq = []
    for d in range(wc + hc - 1):
        lo, hi = max(0, d - (wc - 1)), min(d, hc - 1)
        for pic in range(n):
            for cy in range(lo, hi + 1):
                seq.append((pic, cy, d - cy))
    return seq


SHAPES = [(wc, hc, n) for wc in (1, 2, 7, 13) for hc in (1, 3, 4, 8) for n in (1, 3)]


@pytest.mark.parametrize("wc,hc,n", SHAPES)
def test_every_band_hands_out_its_ctus_once_and_behind_their_neighbours(emul, wc, hc, n):
    for r0 in range(hc):
        for r1 in range(r0 + 1, hc + 1):
            seq = order(emul, wc, r0, r1, n)
            want = {(p, cy, cx) for p in range(n) for cy in range(r0, r1) for cx in range(wc)}
            assert len(seq) == len(want) and set(seq) == want, (r0, r1)          # every CTU of the band once, none outside it
            at = {c: t for t, c in enumerate(seq)}
            for (p, cy, cx), t in at.items():
                for ny, nx in ((cy, cx - 1), (cy - 1, cx), (cy - 1, cx + 1)):  # left, upper, upper right -- where they lie in the band
                    if r0 <= ny and 0 <= nx < wc:
                        assert at[(p, ny, nx)] < t, ((r0, r1), (p, cy, cx), (ny, nx))


@pytest.mark.parametrize("wc,hc,n", SHAPES)
def test_the_whole_picture_keeps_its_order(emul, wc, hc, n):
    assert order(emul, wc, 0, hc, n) == whole_picture_order(wc, hc, n)


def test_a_band_is_the_whole_picture_order_of_its_rows_moved_down(emul):
    for wc, r0, r1, n in ((7, 2, 5, 3), (1, 1, 3, 1), (13, 7, 8, 3)):
        assert order(emul, wc, r0, r1, n) == [(p, cy + r0, cx) for p, cy, cx in whole_picture_order(wc, r1 - r0, n)]


def test_tickets_outside_the_launch_name_no_ctu(emul):
    out = np.zeros(3, np.int32)
    for t in (-1, 7 * 3 * 2, 7 * 3 * 2 + 1000):
        emul.ticket_emul_one(t, 7, 2, 5, 2, out.ctypes.data)
        assert tuple(out) == (-1, -1, -1), t
