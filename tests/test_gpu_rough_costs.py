"""The rough search's cost function for CUs of 8x8 and more (ctu_core.h rough_costs8: the branch-free angular row ang_row8, planar and
DC in a sweep of their own, the DC value by a wave sum): the device against the oracle's restatement of uvg_search_lcu on 136x72
pictures (partial CTUs at both edges), every CU, every CTU's CRCs and all its models.  The depth range is pinned to (3, 3), (2, 2)
and (1, 1) so that the rough search's mode of an 8x8, a 16x16 and a 32x32 CU reaches the output ((2, 2) and (1, 1) give the sizes
{8, 16} and {8, 32} here: the bottom row of partial CTUs splits down to 8).  The content has, in areas of 32x32, stripes along the
directions of one mode of every kind the row treats differently -- see angles_picture -- and the oracle's decisions are checked for
all of them at the pinned size before anything runs on the device."""
import numpy as np
import pytest

import test_gpu_rough_select as RS

pytestmark = pytest.mark.gpu

W, HH = RS.W, RS.HH
DEPTHS, LEVELS, QPS, PINS = [8, 10], [2, 3], [22, 32], [(3, 3), (2, 2), (1, 1)]


def _direction(mode, xx, yy):
    """The coordinate that is constant along the direction of an angular mode: a sample at (x, y) is predicted from the main
    reference at x + (y + 1) * intraPredAngle / 32 (the vertical modes; the horizontal ones with x and y exchanged)."""
    disp = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32]
    md = mode - 50 if mode >= 34 else 18 - mode
    sd = disp[abs(md)] * (1 if md >= 0 else -1)
    return xx + yy * sd / 32.0 if mode >= 34 else yy + xx * sd / 32.0


# The mode whose direction the stripes of each 32x32 area left of x = 96 follow ([row][column]).  What the 32x32 CU of an area can be
# predicted from decides what it can be asked to choose: the top row of areas has no samples above it, the left column none to its
# left, and the samples below left are there only where the CTU to the left holds them -- (2, 0).  The CU at (0, 0) has no reference
# samples at all: every mode predicts the same flat block and the cheapest to signal, planar, wins.
AREAS = [[18, 8, 2],
         [62, 18, 34]]
# The stripes are wide, so that the first round's coarse list (every 4th or 8th mode) has a neighbour of the direction among its
# three survivors, with a fine component on top, so that the direction's own neighbours lose in the last rounds.  The pure mode's
# stripes are narrow; the area with nothing but a left reference keeps to the wide ones.
PERIOD = {18: 11.0, 8: 29.0}
# DC and planar differ by little on the ramp and the patches; with this seed of the noise DC is decided in every pinned case
SEED = 0


def _pattern(m, xx, yy):
    """Cosine stripes along the direction of mode m.  The phase makes the patterns of the modes 2 and 34 agree on the column
    x = 63, which is the left reference of both (2, 0) and (2, 1)."""
    t = _direction(m, xx, yy) - 63.0
    if m in PERIOD:
        return 128 + 60 * np.cos(2 * np.pi * t / PERIOD[m])
    return 128 + 45 * np.cos(2 * np.pi * t / 29.0) + 18 * np.cos(2 * np.pi * t / 7.0)


def angles_picture(depth):
    """Left of x = 96, per 32x32 area, stripes along one mode's direction (AREAS): the pure horizontal mode, modes towards both ends
    of the range, both integer slopes -- 34 is also the middle of the negative angles --, at the scale of 16x16 and 32x32 CUs.  The
    row above and the column to the left of an area, which belong to its neighbours, carry the AREA'S pattern as far as its 32x32
    CU can use them as references, so that the CU can be predicted at all.  Right of x = 96 the ramp and the flat patches of
    test_gpu_rough_select's stripes, where planar and DC win.  The last 8 rows go on with their neighbours' content.  A little
    noise."""
    yy, xx = np.mgrid[0:HH, 0:W].astype(np.float64)
    Y = np.zeros((HH, W))
    for ry in range(3):
        for rx in range(3):
            area = (xx // 32 == rx) & (yy // 32 == ry)
            Y[area] = _pattern(AREAS[min(ry, 1)][rx], xx, yy)[area]
    for ry in range(2):
        for rx in range(3):
            m, x0, y0 = AREAS[ry][rx], 32 * rx, 32 * ry
            md = m - 50 if m >= 34 else 18 - m
            P = _pattern(m, xx, yy)
            if ry > 0:                                  # the row above, to the right only for the positive angles of the vertical modes
                x1 = x0 + (64 if (m >= 34 and md > 0) else 32)
                Y[y0 - 1, max(x0 - 1, 0):x1] = P[y0 - 1, max(x0 - 1, 0):x1]
            if rx > 0:                                  # the column to the left, further down only where the CTU to the left is complete
                y1 = min(y0 + (64 if (m < 34 and md > 0 and x0 % 64 == 0) else 32), HH)
                Y[max(y0 - 1, 0):y1, x0 - 1] = P[max(y0 - 1, 0):y1, x0 - 1]
    Y[0:64, 95] = 100.0                                 # a dark column left of the ramp with one bright sample: the left references
    Y[31, 95] = 160.0                                   # of the CUs on the ramp's edge, where DC has to beat planar
    right = xx >= 96
    Y[right] = (100 + 0.8 * (xx - 96) + 1.5 * yy)[right]
    flat = right & (yy >= 40)
    Y[flat] = 90 + 20 * ((xx[flat] // 8 + yy[flat] // 8) % 3)
    return RS._finish(depth, Y + np.random.default_rng(SEED).normal(0, 1.0, Y.shape))


RS.PICTURES.setdefault("angles", angles_picture)


def decided_modes(o, pin):
    """-> histogram of the luma modes of the CUs of the pinned size in the oracle's result"""
    st = 1 << (4 - pin[0])                      # the CU's size in 4x4 units
    cu = o["cu"][:HH // 4:st, :W // 4:st]
    cu = cu[(cu[:, :, 0] == 1) & (cu[:, :, 1] == 6 - pin[0])]           # intra, log2 of the size
    return np.bincount(cu[:, 6].astype(np.int64), minlength=67)


@pytest.fixture(scope="module")
def angles_covered(orc):
    """On the oracle's result of every pinned run: the decided modes of the CUs of the pinned size include planar, DC, a pure mode, an
    integer slope, a mode in 3..10, one in 58..65 and one of the negative angles 19..49."""
    for depth in DEPTHS:
        for levels in LEVELS:
            for qp in QPS:
                for pin in PINS:
                    _, o = RS.oracle_of(orc, "angles", depth, levels, qp, pin)
                    h = decided_modes(o, pin)
                    print("angles: %d bit, rough_levels %d, QP %d, depth %d: modes %s" % (depth, levels, qp, pin[0], np.flatnonzero(h).tolist()))
                    assert h.sum() >= 8, (depth, levels, qp, pin)
                    assert h[0] and h[1] and h[18] + h[50] and h[2] + h[34] + h[66] and h[3:11].sum() and h[58:66].sum() and h[19:50].sum(), \
                        (depth, levels, qp, pin, np.flatnonzero(h).tolist())
    return True


@pytest.mark.parametrize("pin", PINS, ids=lambda p: "depth%d" % p[0])
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_every_kind_of_mode_equals_the_oracle(hip, orc, angles_covered, depth, levels, qp, pin):
    RS.device_against_oracle(hip, orc, "angles", depth, levels, qp, pin)


@pytest.mark.parametrize("depth,levels", [(8, 2), (10, 3)])
def test_default_range_equals_the_oracle(hip, orc, depth, levels):
    """All four sizes in one picture: the depth waves' routes and the walk's."""
    RS.device_against_oracle(hip, orc, "angles", depth, levels, 27, (1, 4))


def test_pb_search_equals_the_encoders_records(hip):
    """The P / B kernel compiles the same function: the smallest P / B golden through test_gpu_ctu_search_pb's own route."""
    RS.test_pb_search_equals_the_encoders_records(hip)
