"""oracle/orc_search.c (the closed-loop intra CTU search: split / mode decisions, reconstruction, levels, model adaptation)
against records of the real reference encoder (tools/refcheck/ctu_dump.c -> tests/golden/ref_ctu*.npz):
every CTU of two small pictures item by item, every CTU of a 1080p picture through per-CTU CRCs."""
import numpy as np
import pytest

import helpers as H


@pytest.mark.parametrize("name", ["ref_ctu_832x480_8_qp22", "ref_ctu_416x240_10_qp37", "ref_ctu_320x192_8_qp42", "ref_ctu_192x128_10_qp12", "ref_ctu_256x128_8_qp7", "ref_ctu_264x136_10_qp32"])
def test_every_ctu_equals_the_reference_run(orc, name):
    g = every_ctu_equals_the_reference_run(orc, name)
    Hh, W = g["rec_y"].shape
    h4, w4 = Hh // 4, W // 4
    # the partition really is a mix of sizes, and the search's final models differ from the coder's somewhere (why both are kept)
    sizes = set(np.unique(g["cu"][:h4, :w4, 1]).tolist())
    assert len(sizes) >= 4 and sizes <= {2, 3, 4, 5, 6}
    assert any(not np.array_equal(g["models"][k, 1], g["models"][k, 2]) for k in range(len(g["models"])))


@pytest.mark.parametrize("name", ["ref_ctu_136x72_10_qp0", "ref_ctu_200x136_8_qp51", "ref_ctu_40x24_8_qp22", "ref_ctu_24x136_10_qp37"])
def test_every_ctu_at_the_extremes_equals_the_reference_run(orc, name):
    """The same parity at QP 0 / 51, on white noise and lone impulses, on pictures smaller than one CTU -- content whose partitions are
    uniform (all small CUs on noise, no 64x64 CU in a picture of 40x24), so without the mix-of-sizes check above."""
    every_ctu_equals_the_reference_run(orc, name)


def every_ctu_equals_the_reference_run(orc, name):
    g = H.ctu_golden(name)
    W, Hh, depth, qp, y, u, v = H.golden_source(g)
    prm = H.search_params(W, Hh, qp)
    assert np.array_equal(g["lam"][:3], [prm.lam, prm.lam_sqrt, prm.c_lam])          # state->lambda, lambda_sqrt, c_lambda of the run
    r = H.oracle_search_picture(orc, depth, prm, y, u, v)
    wc = (W + 63) // 64
    for k in range(len(g["models"])):
        for j, what in enumerate(("at the CTU's start", "after the search", "after the coder")):
            assert np.array_equal(r["models"][k, j], g["models"][k, j]), (k % wc, k // wc, what)
    h4, w4 = Hh // 4, W // 4
    assert np.array_equal(r["cu"][:h4, :w4], g["cu"][:h4, :w4])
    assert np.array_equal(r["trees"][:h4, :w4], g["trees"][:h4, :w4])
    for p in ("rec_y", "rec_u", "rec_v"):
        assert np.array_equal(r[p], g[p]), p
    # levels: the reference leaves uninitialised memory outside the picture (its work-tree copies are malloc'ed), so only inside
    assert np.array_equal(H.ctu_crcs(r, W, Hh)[:, 2], H.ctu_crcs(dict(r, coeff=g["coeff"]), W, Hh)[:, 2])
    return g


def test_1080p_picture_equals_the_reference_run_ctu_by_ctu(orc):
    g = H.ctu_golden("ref_ctucrc_1920x1080_8_qp22")
    W, Hh, depth, qp, y, u, v = H.golden_source(g)
    r = H.oracle_search_picture(orc, depth, H.search_params(W, Hh, qp), y, u, v)
    got = H.ctu_crcs(r, W, Hh)
    bad = np.argwhere((got != g["crc"]).any(axis=1)).ravel()
    assert bad.size == 0, bad[:10]
