"""The 4x4 leaf's joint block pass (ctu_leaf4.h leaf_recon_rows: the luma block of the fourth 4x4 CU of an 8x8 area and the area's Cb
and Cr blocks, or the Cb and Cr blocks of an 8x8 CU, a block per row of 16 lanes) forced into the output: on the default depth range
a 4x4 split rarely wins on smooth content, so these pictures are searched with the leaf depth pinned.  The device against the
oracle's restatement of uvg_search_lcu: every CTU's CRCs and all its context models."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def run_gpu(hip, depth, prm, pic):
    import torch
    from uvg266_amd import api
    P = api.ctu_params(prm.pic_w, prm.pic_h, prm.qp, lam=prm.lam)
    P.depth_min, P.depth_max, P.combine_intra_cus = prm.depth_min, prm.depth_max, prm.combine_intra_cus
    cs = api.CtuSearch(P, [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pic)])
    cs.run()
    torch.cuda.synchronize()
    ry, ru, rv = (t.cpu().numpy() for t in cs.rec[0])
    scu = cs.cu[0].cpu().numpy().reshape(-1).view(H.SCU_NP)
    return H.search_result_from_device_layout(prm.pic_w, prm.pic_h, ry, ru, rv, scu, cs.coeff[0].cpu().numpy(), cs.models[0].cpu().numpy().view(np.uint32))

W, HH = 136, 72          # partial CTUs at the right and bottom edges; 17 x 9 = 153 areas of 8x8


def picture(depth):
    s = 1 if depth == 8 else 4
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:HH, 0:W]
    cy, cx = np.mgrid[0:HH // 2, 0:W // 2]
    Y = 128 * s + 40 * s * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 12 * s, (HH, W))
    U = 128 * s + 30 * s * np.sin(cx / 5.0 + cy / 11.0) + rng.normal(0, 3 * s, (HH // 2, W // 2))
    V = 128 * s + 30 * s * np.cos(cy / 6.0 - cx / 13.0) + rng.normal(0, 3 * s, (HH // 2, W // 2))
    dt = np.uint8 if depth == 8 else np.uint16
    return tuple(np.clip(np.rint(p), 0, (1 << depth) - 1).astype(dt) for p in (Y, U, V))


def device_against_oracle(hip, orc, depth, qp, dmin, dmax):
    pic = picture(depth)
    prm = H.search_params(W, HH, qp)
    prm.depth_min, prm.depth_max, prm.combine_intra_cus = dmin, dmax, 0
    o = H.oracle_search_picture(orc, depth, prm, *pic)
    r = run_gpu(hip, depth, prm, pic)
    assert np.array_equal(H.ctu_crcs(r, W, HH), H.ctu_crcs(o, W, HH)), (depth, qp, dmin, dmax)
    assert np.array_equal(r["models"], o["models"]), (depth, qp, dmin, dmax)
    return o


@pytest.mark.parametrize("depth", [8, 10])
def test_only_4x4_cus_equal_the_oracle(hip, orc, depth):
    """Case A: every CU a 4x4 one, so every area's fourth CU takes the joint pass of Y, Cb and Cr.  All four combinations of the two
    chroma flags must occur (Cr is carried under both values of Cb's flag and one is kept): at least 10 areas each, counted on the
    oracle's result."""
    o = device_against_oracle(hip, orc, depth, 32, 4, 4)
    cbf = o["cu"][:HH // 4:2, :W // 4:2, 5].astype(int)
    assert cbf.size == 153
    counts = [int((((cbf >> 1) & 3) == k).sum()) for k in range(4)]          # neither, Cb only, Cr only, both
    print("areas by (cbf_cb, cbf_cr): none %d, cb %d, cr %d, both %d" % tuple(counts))
    assert min(counts) >= 10, counts


@pytest.mark.parametrize("depth", [8, 10])
def test_8x8_and_4x4_cus_equal_the_oracle(hip, orc, depth):
    """Case B: 8x8 CUs against their 4x4 split: the Cb + Cr pass of the 8x8 CU on the depth wave beside the leaf's."""
    device_against_oracle(hip, orc, depth, 27, 3, 4)


def test_large_levels_equal_the_oracle(hip, orc):
    """Case C: 10 bit at QP 2, only 4x4 CUs: levels so large that a 4x4 block's budget of regular bins runs out (the branch
    28 - spent < 4 of the leaf's RDOQ), in rows that run out at different positions."""
    device_against_oracle(hip, orc, 10, 2, 4, 4)
