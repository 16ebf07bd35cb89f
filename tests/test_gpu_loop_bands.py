"""The closed loop of ONE picture sharded over ranks by CTU rows (uvghip_loop_plan_create_rows: search, per-CTU filter stage with the SAO
decision's chain, coder): N emulated ranks on one GPU, each with its own plan and its own buffers -- reconstruction, side information,
levels, models, output planes AND the workspace POISONED before the plan is created --, run top to bottom; between two ranks only what the
upper one's side 1 list names moves into the lower one's side 0 list.  Every band's output rows, decisions, SAO models and slice rows are
the reference encoder's (tests/golden/ref_ctu_*.npz), and the bands' rows and checksum terms make up the encoder's .266."""
import ctypes

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu


def poisoner(seed):
    """-> (prepare callback for api.ClosedLoop, dict that receives copies of the poisoned output / reconstruction allocations)."""
    kept = {}

    def fill(t, s):
        import torch
        g = torch.Generator(device="cuda").manual_seed(s)
        if t.dtype == torch.uint16:
            t.copy_(torch.randint(0, 1024, t.shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint16))
        elif t.dtype == torch.uint8:
            t.copy_(torch.randint(0, 256, t.shape, generator=g, device="cuda", dtype=torch.int32).to(torch.uint8))
        else:
            t.copy_(torch.randint(-20000, 20000, t.shape, generator=g, device="cuda", dtype=torch.int32).to(t.dtype))

    def prepare(cl):
        k = 0
        for i in range(cl.n):
            for t in list(cl.rec_full[i]) + list(cl.out_full[i]) + [cl.cu[i], cl.coeff[i], cl.models[i]]:
                fill(t, seed * 1000 + k)
                k += 1
        fill(cl.loop_ws, seed * 1000 + 999)
        kept["out"] = [[t.clone() for t in o] for o in cl.out_full]
        kept["rec"] = [[t.clone() for t in o] for o in cl.rec_full]
    return prepare, kept


def hand_down(upper, lower):
    """What the transports would move between two neighbouring bands: the upper band's side 1 pieces into the lower band's side 0 pieces."""
    from uvg266_amd import bands
    bands.emulate([[(1, upper.halo(1), [])], [(0, [], lower.halo(0))]])


def band_results(cl):
    """Everything a band produced, on the host."""
    info, models = cl.results()
    rows, nb = cl.slice_data()
    return dict(out=[[t.cpu().numpy() for t in o] for o in cl.out_full], info=info, models=models, rows=rows.cpu().numpy(), nb=nb.cpu().numpy())


def check_band(cl, lay, res, kept, want, W, Hh, label):
    """want: per picture a dict final (three planes), sao [ctus, 2, 17] or None, sao_models, rows (list of bytes per CTU row) -- entries may be
    None for what has no reference.  Output rows outside out_rows() and the planes' padding columns still hold the poison."""
    wc = (W + 63) // 64
    y0, y1 = cl.out_rows()
    delay = 10 if cl.sao_type else 8
    assert y0 == (64 * lay.ctu_row0 - delay if lay.ctu_row0 else 0) and y1 == (Hh if lay.down < 0 else 64 * lay.ctu_row1 - delay), label
    k0, k1 = lay.ctu_row0 * wc, lay.ctu_row1 * wc
    for i, w in enumerate(want):
        for c in range(3):
            sh = 1 if c else 0
            a, b, pw = y0 >> sh, y1 >> sh, W >> sh
            got, poison = res["out"][i][c], kept["out"][i][c].cpu().numpy()
            assert np.array_equal(got[a:b, :pw], w["final"][c][a:b]), (label, i, "output plane", c)
            assert np.array_equal(got[:a], poison[:a]) and np.array_equal(got[b:], poison[b:]), (label, i, "output rows of another band were written", c)
            assert np.array_equal(got[:, pw:], poison[:, pw:]), (label, i, "padding columns of the output", c)
        if w.get("sao") is not None:
            assert np.array_equal(H.sao_info_comparable(res["info"][i][k0:k1]), H.sao_info_comparable(w["sao"][k0:k1])), (label, i, "sao")
            assert np.array_equal(res["models"][i][k0:k1], w["sao_models"][k0:k1]), (label, i, "sao models")
        for r in range(lay.ctu_row0, lay.ctu_row1):
            assert res["rows"][i, r, :res["nb"][i, r]].tobytes() == w["rows"][r], (label, i, "slice row", r)


def golden_want(g):
    off = g["row_off"]
    return dict(final=[g["final_y"], g["final_u"], g["final_v"]], sao=g["sao"], sao_models=g["sao_models"],
                rows=[g["row_bytes"][off[r]:off[r + 1]].tobytes() for r in range(len(off) - 1)])


def dev(planes):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in planes)


@pytest.mark.parametrize("name,nranks", [("ref_ctu_832x480_8_qp22", 2), ("ref_ctu_832x480_8_qp22", 3), ("ref_ctu_832x480_8_qp22", 8), ("ref_ctu_416x240_10_qp37", 2),
                                         ("ref_ctu_416x240_10_qp37", 4), ("ref_ctu_24x136_10_qp37", 3)])
def test_bands_of_the_closed_loop_equal_the_encoders_run(hip, name, nranks):
    import torch
    from uvg266_amd import api, bands, tiles
    g = H.ctu_golden(name)
    W, Hh, depth, qp, y, u, v = H.golden_source(g)
    P = api.ctu_params(W, Hh, qp, lam=H.search_params(W, Hh, qp).lam)
    wc, hc = (W + 63) // 64, (Hh + 63) // 64
    src = dev((y, u, v))
    want = [golden_want(g)]
    loops, lays, kepts = [], [], []
    for r in range(nranks):
        lay = bands.BandLayout(Hh, nranks, r)
        prepare, kept = poisoner(r + 1)
        loops.append(api.ClosedLoop(P, [src], rows=(lay.ctu_row0, lay.ctu_row1), prepare=prepare))
        lays.append(lay); kepts.append(kept)
    contributions = []
    for r, (cl, lay) in enumerate(zip(loops, lays)):
        # the lists: nothing above the first band, nothing below the last; a boundary's bytes are the documented ones, the same on both sides
        assert (len(cl.halo_pieces(0)) > 0) == (r > 0) and (len(cl.halo_pieces(1)) > 0) == (r + 1 < nranks)
        ops = cl.halo_ops(up=r - 1 if r else None, down=r + 1 if r + 1 < nranks else None)
        per = bands.halo_loop_bytes(depth, 1, W, 3)
        assert bands.spec_bytes(ops) == (per if r + 1 < nranks else 0, per if r else 0) and cl.halo_bytes() == (per if nranks > 1 else 0)
        if r:
            # ... and the pieces are those of bands.BandLayout.halo_loop, in its order (rows and bytes per row)
            meta = lambda rows, cols, dt: torch.empty((rows, cols), dtype=dt, device="meta")
            px = src[0].dtype
            named = [meta(Hh, W, px), meta(Hh // 2, W // 2, px), meta(Hh // 2, W // 2, px), meta(hc * 16, wc * 16 * 32, torch.uint8), meta(3 * wc * hc, 257, torch.int32),
                     meta(Hh, W, px), meta(Hh // 2, W // 2, px), meta(Hh // 2, W // 2, px), meta(hc, wc * 34, torch.int32), meta(wc * hc, 6, torch.int16)]
            listed = [(t.shape[1] * t.element_size(), b - a) for t, a, b in lay.halo_loop(*named, wc)[0][2]]
            assert [(rb, rows) for _, rb, rows, _ in cl.halo_pieces(0)] == listed
            hand_down(loops[r - 1], cl)
        cl.run()
        torch.cuda.synchronize()
        check_band(cl, lay, band_results(cl), kepts[r], want, W, Hh, (name, nranks, r))
        contributions.append(cl.substreams((lay.ctu_row0, lay.ctu_row1)))
    # rank 0's job: every band's rows and checksum terms -> the picture's NAL units = the tail of the encoder's file
    nals = tiles.write_nals(np.stack([c[0] for c in contributions]), [c[1] for c in contributions], np.stack([c[2] for c in contributions]), 0, sao=True)
    stream = g["bitstream"].tobytes()
    assert stream[stream.find(b"\x00\x00\x01\x00\x41"):] == nals[0]
    sums = (np.stack([c[2] for c in contributions]).astype(np.uint64).sum(axis=0) & 0xFFFFFFFF)[0]
    assert [int(s) for s in sums] == [H.picture_checksum(g[k], depth) for k in ("final_y", "final_u", "final_v")]


@pytest.mark.parametrize("name,pad", [("ref_ctu_832x480_8_qp22", 16), ("ref_ctu_416x240_10_qp37", 5), ("ref_ctu_24x136_10_qp37", 2)])
def test_one_packed_message_moves_what_the_piece_lists_name(hip, name, pad):
    """Three pictures, two bands.  The upper band packs its side 1 pieces of all pictures into one buffer (one launch), the buffer is copied
    device to device, the lower band -- whose planes have a PADDED stride, the sender's have not -- unpacks it (one launch): the same results
    as a lower band fed piece by piece, and the padding still holds its poison.  pad 16 / 5 / 2 samples: rows that keep the 16-byte path,
    rows at 2-byte and at 4-byte alignment."""
    import torch
    from uvg266_amd import api, bands, layout
    g = H.ctu_golden(name)
    W, Hh, depth, qp, y, u, v = H.golden_source(g)
    P = api.ctu_params(W, Hh, qp, lam=H.search_params(W, Hh, qp).lam)
    srcs = [dev((y, u, v))] + [dev(layout.synthetic_yuv420(W, Hh, t, depth)) for t in (5, 6)]
    lays = [bands.BandLayout(Hh, 2, r) for r in range(2)]
    mk = lambda r, seed, pad=0: (lambda pk: (api.ClosedLoop(P, srcs, rows=(lays[r].ctu_row0, lays[r].ctu_row1), pad=pad, prepare=pk[0]), pk[1]))(poisoner(seed))
    (upper, _), (fed, fed_kept), (lower, kept) = mk(0, 1), mk(1, 2), mk(1, 3, pad)
    upper.run()
    torch.cuda.synchronize()
    hand_down(upper, fed)
    fed.run()
    assert upper.halo_bytes() == lower.halo_bytes() == bands.halo_loop_bytes(depth, 3, W, 3)
    msg = upper.halo_pack()
    wire = torch.empty_like(msg)
    wire.copy_(msg)                                    # the one transfer of a boundary
    lower.halo_unpack(wire)
    lower.run()
    torch.cuda.synchronize()
    a, b = band_results(fed), band_results(lower)
    # the piece-fed band against the encoder's records (the first picture), then the message-fed band against the piece-fed one
    check_band(fed, lays[1], a, fed_kept, [golden_want(g)], W, Hh, (name, "fed by pieces"))
    want = [dict(final=[a["out"][i][c][:, :W >> (1 if c else 0)] for c in range(3)], sao=a["info"][i], sao_models=a["models"][i],
                 rows=[a["rows"][i, r, :a["nb"][i, r]].tobytes() if r >= lays[1].ctu_row0 else None for r in range(a["nb"].shape[1])]) for i in range(3)]
    check_band(lower, lays[1], b, kept, want, W, Hh, (name, "fed by the message"))
    # the unpacked rows lie where the lists say, and only there: the reconstruction's padding columns and the rows above the 16 received
    y0 = lays[1].y0
    for i in range(3):
        for c in range(3):
            sh = 1 if c else 0
            got, poison, pw = lower.rec_full[i][c].cpu().numpy(), kept["rec"][i][c].cpu().numpy(), W >> sh
            assert np.array_equal(got[:, pw:], poison[:, pw:]), (i, c, "padding columns of the reconstruction")
            assert np.array_equal(got[:(y0 - 16) >> sh], poison[:(y0 - 16) >> sh]), (i, c, "rows above the hand-over")
            assert np.array_equal(got[(y0 - 16) >> sh:y0 >> sh, :pw], upper.rec_full[i][c].cpu().numpy()[(y0 - 16) >> sh:y0 >> sh, :pw]), (i, c, "the received rows")


def test_a_band_plan_of_the_whole_picture_is_the_whole_picture_plan(hip):
    import torch
    from uvg266_amd import api
    g = H.ctu_golden("ref_ctu_416x240_10_qp37")
    W, Hh, depth, qp, y, u, v = H.golden_source(g)
    P = api.ctu_params(W, Hh, qp, lam=H.search_params(W, Hh, qp).lam)
    src = dev((y, u, v))
    a, b = api.ClosedLoop(P, [src]), api.ClosedLoop(P, [src], rows=(0, (Hh + 63) // 64))
    for cl in (a, b):
        assert cl.halo_pieces(0) == [] and cl.halo_pieces(1) == [] and cl.halo_bytes() == 0 and cl.out_rows() == (0, Hh)
        cl.run()
    torch.cuda.synchronize()
    ra, rb = band_results(a), band_results(b)
    assert all(np.array_equal(p, q) for p, q in zip(ra["out"][0], rb["out"][0]))
    assert np.array_equal(ra["info"], rb["info"]) and np.array_equal(ra["models"], rb["models"]) and np.array_equal(ra["nb"], rb["nb"])
    assert all(np.array_equal(ra["rows"][0, r, :ra["nb"][0, r]], rb["rows"][0, r, :rb["nb"][0, r]]) for r in range(ra["nb"].shape[1]))
    assert a.picture_nals(0, 0) == b.picture_nals(0, 0)


def test_two_bands_without_sao_equal_the_whole_picture_run(hip):
    """sao_type 0: the output is the deblocked picture, 8 rows behind; the hand-over has no SAO pieces (the list is shorter, not padded)."""
    import torch
    from uvg266_amd import api, bands, layout
    W, Hh, depth, qp = 200, 136, 8, 27
    P = api.ctu_params(W, Hh, qp)
    src = dev(layout.synthetic_yuv420(W, Hh, 4, depth))
    whole = api.ClosedLoop(P, [src], sao_type=0)
    whole.run()
    torch.cuda.synchronize()
    ref = band_results(whole)
    want = [dict(final=ref["out"][0], rows=[ref["rows"][0, r, :ref["nb"][0, r]].tobytes() for r in range(ref["nb"].shape[1])])]
    loops = []
    for r in range(2):
        lay = bands.BandLayout(Hh, 2, r)
        prepare, kept = poisoner(r + 1)
        cl = api.ClosedLoop(P, [src], sao_type=0, rows=(lay.ctu_row0, lay.ctu_row1), prepare=prepare)
        assert len(cl.halo_pieces(0)) == (5 if r else 0) and len(cl.halo_pieces(1)) == (0 if r else 5)
        assert cl.halo_bytes() == bands.halo_loop_bytes(depth, 1, W, 0) == bands.spec_bytes(cl.halo_ops(up=0 if r else None, down=None if r else 1))[r]
        if r:
            hand_down(loops[0], cl)
        cl.run()
        torch.cuda.synchronize()
        check_band(cl, lay, band_results(cl), kept, want, W, Hh, ("no sao", r))
        loops.append(cl)
    cut = 64 * bands.BandLayout(Hh, 2, 0).ctu_row1 - 8          # the deblocking delay alone
    assert loops[0].out_rows() == (0, cut) and loops[1].out_rows() == (cut, Hh)


def test_refusals_of_the_band_plan(hip):
    import torch
    from uvg266_amd import api, layout, lib
    W, Hh = 136, 136
    P = api.ctu_params(W, Hh, 27)
    src = dev(layout.synthetic_yuv420(W, Hh, 1, 8))
    for rows in ((-1, 2), (0, 4), (2, 2), (2, 1)):
        with pytest.raises(RuntimeError, match="CTU row range"):
            api.ClosedLoop(P, [src], rows=rows)
    with pytest.raises(RuntimeError):
        api.ClosedLoop(P, [src], sao_type=4, rows=(0, 1))
    top, mid = api.ClosedLoop(P, [src], rows=(0, 1)), api.ClosedLoop(P, [src], rows=(1, 2))
    n = ctypes.c_int(0)
    piece = (lib.HaloPiece * 16)()
    for side in (-1, 2):
        assert hip.uvghip_loop_plan_halo(mid.loop, side, piece, 16, ctypes.byref(n)) != 0 and b"side" in hip.uvghip_last_error()
    assert hip.uvghip_loop_plan_halo(mid.loop, 0, piece, 9, ctypes.byref(n)) != 0 and n.value == 10 and b"cap" in hip.uvghip_last_error()
    assert hip.uvghip_loop_plan_halo(mid.loop, 0, piece, 10, ctypes.byref(n)) == 0 and n.value == 10
    msg = torch.zeros(mid.halo_bytes(), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="nothing comes from above"):
        top.halo_unpack(msg)
    bottom = api.ClosedLoop(P, [src], rows=(2, 3))
    with pytest.raises(RuntimeError, match="nothing goes down"):
        bottom.halo_pack(msg)
    with pytest.raises(RuntimeError, match="band plan"):
        mid.picture_nals(0, 0)
    torch.cuda.synchronize()
