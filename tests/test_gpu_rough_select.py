"""The rough search's selection in the lanes that hold the costs (ctu_core.h rs_pick_min / rs_insert; ctu_leaf4.h leaf_rough: lane L
is mode L + 2, planar, DC and mode 66 wave-uniform beside them; search_intra_rough: a lane per listed mode): the device against the
oracle's restatement of uvg_search_lcu on 136x72 pictures (partial CTUs at both edges), every CTU's CRCs and all its models.  The
depth range is pinned so that the rough search's mode reaches the output: (4, 4) makes every CU a 4x4 leaf, (3, 3) an 8x8 CU on the
walk's wave; (3, 4) adds the depth wave's route.  Two contents: one on which different modes tie in cost (the order of insertion
decides), one whose decided modes lie at both ends of the angular range (modes 2, 3 and 66, their neighbours, planar and DC)."""
import os

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

W, HH = 136, 72
DEPTHS, LEVELS, QPS, PINS = [8, 10], [2, 3], [22, 32], [(4, 4), (3, 3)]


def _finish(depth, Y):
    s = 1 if depth == 8 else 4
    cy, cx = np.mgrid[0:HH // 2, 0:W // 2]
    U = 128 + 20 * np.sin(cx / 5.0 + cy / 11.0)
    V = 128 + 20 * np.cos(cy / 6.0 - cx / 13.0)
    return tuple(np.clip(np.rint(p * s), 0, (1 << depth) - 1).astype(H.px_dtype(depth)) for p in (Y, U, V))


def ties_picture(depth):
    """A base value plus {0, 1, 2} held over 2x2 samples (at 10 bit: times 4; the rows from 48 on: times 3, so that more than the
    most probable modes win), with every other 16x16 area of the upper rows exactly flat: on a flat area every mode has the same
    distortion and one of a few bit costs."""
    rng = np.random.default_rng(11)
    Y = 120.0 + np.kron(rng.integers(0, 3, (HH // 2, W // 2)), np.ones((2, 2)))
    Y[48:] = 120.0 + 3 * (Y[48:] - 120.0)
    for ay in range(0, 48, 16):
        for ax in range(0, 128, 32):
            Y[ay:ay + 16, ax + (ay & 16):ax + (ay & 16) + 16] = 121.0
    return _finish(depth, Y)


def stripes_picture(depth):
    """Sine stripes along the up-right diagonal and along the directions of the modes 3 / 65 and 4 / 64 in bands of 16 columns, a ramp
    and flat patches to their right, a little noise."""
    yy, xx = np.mgrid[0:HH, 0:W].astype(np.float64)
    Y = np.zeros((HH, W))
    for i, a in enumerate([45.0, 47.8, 42.2, 47.8, 50.9, 39.1]):
        t = np.deg2rad(a)
        band = (xx >= i * 16) & (xx < (i + 1) * 16)
        Y[band] = (128 + 60 * np.sin(2 * np.pi * (xx * np.cos(t) + yy * np.sin(t)) / (6.0 + 2 * (i % 2))))[band]
    right = xx >= 96
    Y[right] = (100 + 0.8 * (xx - 96) + 1.5 * yy)[right]
    flat = right & (yy >= 40)
    Y[flat] = 90 + 20 * ((xx[flat] // 8 + yy[flat] // 8) % 3)
    return _finish(depth, Y + np.random.default_rng(0).normal(0, 1.0, Y.shape))


PICTURES = {"ties": ties_picture, "stripes": stripes_picture}
_oracle = {}


def oracle_of(orc, content, depth, levels, qp, pin):
    """The oracle's result of a case, computed once."""
    key = (content, depth, levels, qp, pin)
    if key not in _oracle:
        prm = H.search_params(W, HH, qp)
        prm.depth_min, prm.depth_max, prm.combine_intra_cus, prm.rough_levels = pin[0], pin[1], 0, levels
        _oracle[key] = (prm, H.oracle_search_picture(orc, depth, prm, *PICTURES[content](depth)))
    return _oracle[key]


def device_against_oracle(hip, orc, content, depth, levels, qp, pin):
    import torch
    from uvg266_amd import api
    prm, o = oracle_of(orc, content, depth, levels, qp, pin)
    pic = PICTURES[content](depth)
    P = api.ctu_params(prm.pic_w, prm.pic_h, prm.qp, lam=prm.lam, rough_levels=levels)
    P.depth_min, P.depth_max, P.combine_intra_cus = prm.depth_min, prm.depth_max, prm.combine_intra_cus
    cs = api.CtuSearch(P, [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pic)])
    cs.run()
    torch.cuda.synchronize()
    ry, ru, rv = (t.cpu().numpy() for t in cs.rec[0])
    scu = cs.cu[0].cpu().numpy().reshape(-1).view(H.SCU_NP)
    r = H.search_result_from_device_layout(W, HH, ry, ru, rv, scu, cs.coeff[0].cpu().numpy(), cs.models[0].cpu().numpy().view(np.uint32))
    case = (content, depth, levels, qp, pin)
    assert np.array_equal(r["cu"][:, :, 6], o["cu"][:, :, 6]), ("modes", case)
    assert np.array_equal(H.ctu_crcs(r, W, HH), H.ctu_crcs(o, W, HH)), case
    assert np.array_equal(r["models"], o["models"]), case


def round0_modes(levels):
    off = 1 << levels
    return np.array([0, 1] + list(range(2 + off // 2, 67, off)), np.int8)


def blocks_with_a_shared_minimum(orc, depth, levels, n):
    """Blocks of n x n whose smallest distortion (min(SATD, 2 SAD), the oracle's open-loop cost function) over round 0's listed modes is
    shared by two or more of them."""
    from uvg266_amd import layout
    y = PICTURES["ties"](depth)[0]
    modes = round0_modes(levels)
    blks = layout.intra_availability(layout.block_grid(W, HH, n), n, W, HH)
    costs = np.zeros((len(blks), len(modes)), np.uint32)
    orc.fn(depth, "intra_search_frame", None)(H.ptr(y), W, H.ptr(y), W, W, HH, n, H.ptr(blks), len(blks), H.ptr(modes), len(modes), H.ptr(costs))
    return int(((costs == costs.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum())


@pytest.fixture(scope="module")
def ties_covered(orc):
    """The coverage the tie content is there for, asserted on the CPU before any device comparison.  A proxy: the oracle's open-loop
    costs are taken from SOURCE references and carry no mode bits, where the search predicts from reconstructed samples and adds the
    bits; on the exactly flat areas the reconstruction is flat as well and the bit cost takes one of a few values, so the ties stay."""
    for depth in DEPTHS:
        for levels in LEVELS:
            for n in (4, 8):
                k = blocks_with_a_shared_minimum(orc, depth, levels, n)
                print("ties: %d bit, rough_levels %d, %dx%d blocks with a shared minimum: %d" % (depth, levels, n, n, k))
                assert k >= 20, (depth, levels, n, k)
    return True


@pytest.fixture(scope="module")
def stripes_covered(orc):
    """On the oracle's result of every pinned run of the stripes: the decided modes include 2, 3 and 66, one of 4..7, one of 62..65,
    planar and DC -- at size 4 and at size 8."""
    for depth in DEPTHS:
        for levels in LEVELS:
            for qp in QPS:
                for pin in PINS:
                    _, o = oracle_of(orc, "stripes", depth, levels, qp, pin)
                    st = 1 if pin[0] == 4 else 2
                    cu = o["cu"][:HH // 4:st, :W // 4:st]
                    assert (cu[:, :, 0] == 1).all() and (cu[:, :, 1] == (2 if pin[0] == 4 else 3)).all()
                    h = np.bincount(cu[:, :, 6].ravel(), minlength=67)
                    assert h[2] and h[3] and h[66] and h[4:8].sum() and h[62:66].sum() and h[0] and h[1], (depth, levels, qp, pin, h)
    return True


@pytest.mark.parametrize("pin", PINS, ids=lambda p: "depth%d" % p[0])
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_ties_equal_the_oracle(hip, orc, ties_covered, depth, levels, qp, pin):
    device_against_oracle(hip, orc, "ties", depth, levels, qp, pin)


@pytest.mark.parametrize("pin", PINS, ids=lambda p: "depth%d" % p[0])
@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_edge_modes_equal_the_oracle(hip, orc, stripes_covered, depth, levels, qp, pin):
    device_against_oracle(hip, orc, "stripes", depth, levels, qp, pin)


@pytest.mark.parametrize("content,depth,levels", [("ties", 8, 2), ("stripes", 10, 3)])
def test_default_range_equals_the_oracle(hip, orc, content, depth, levels):
    """8x8 CUs on the depth wave (its candidate route) against their 4x4 split on the walk's."""
    device_against_oracle(hip, orc, content, depth, levels, 27, (3, 4))


def test_pb_search_equals_the_encoders_records(hip):
    """The P / B kernel compiles the same headers: the smallest P / B golden through test_gpu_ctu_search_pb's own route."""
    import torch
    from uvg266_amd import api
    import test_gpu_ctu_search_pb as PB
    name = min(PB.GOLDENS, key=lambda n: os.path.getsize(os.path.join(H.GOLDEN, n + ".npz")))
    g = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    Wp, Hp, depth, pics, P = H.inter_pictures_from_golden(g)
    descs, tens, recs = PB.device_pictures(Wp, Hp, depth, pics, P)
    api.ctu_search_pb(descs, depth)
    torch.cuda.synchronize()
    for t, (fr, d) in zip(tens, recs):
        assert H.compare_device_inter_picture(Wp, Hp, d, PB.result_of(Wp, Hp, t)) == [], f"frame {fr}"
