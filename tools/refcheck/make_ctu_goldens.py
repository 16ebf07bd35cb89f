#!/usr/bin/env python3
"""Dev-time: regenerate tests/golden/ref_ctu_*.npz / ref_ctucrc_*.npz from runs of the real reference encoder
(tools/refcheck/ctu_dump.c through ctu_dump.sh; needs the survey's reference build, see README.md).

  python tools/refcheck/make_ctu_goldens.py

Full records (every CTU's models at its start / after its search / after the real coder, cu_info fields, reconstruction before
the in-loop filters, levels) for two small pictures; per-CTU CRC-32 of the same items for BASELINE-sized pictures.
The source pictures are uvg266_amd.layout.synthetic_yuv420; their CRC is stored so that a test notices a
generator that drifted."""
import os, struct, subprocess, sys, zlib
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from uvg266_amd import layout

DT = [np.uint8, np.uint16, np.int16, np.int32, np.uint32, np.int64, np.float64]


def read_records(path):
    data = open(path, "rb").read()
    p, recs = 0, []
    while p < len(data):
        magic, nl = struct.unpack_from("<II", data, p); p += 8
        assert magic == 0x52454631
        name = data[p:p + nl].decode(); p += nl
        na, = struct.unpack_from("<I", data, p); p += 4
        arrs = []
        for _ in range(na):
            c, n = struct.unpack_from("<II", data, p); p += 8
            a = np.frombuffer(data, DT[c], n, p); p += a.nbytes
            arrs.append(a)
        recs.append((name, arrs))
    return recs


def run(W, H, depth, qp, t, tag, picture=None, extra=()):
    px = np.uint8 if depth == 8 else np.uint16
    y, u, v = (picture or layout.synthetic_yuv420)(W, H, t, depth)
    yuv = f"/tmp/gold_{tag}.yuv"
    with open(yuv, "wb") as f:
        for p in (y, u, v):
            f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), "1", out,
                           "preset", "medium", "period", "1", "qp", str(qp)] + list(extra), stderr=subprocess.DEVNULL)
    recs = read_records(out + ".bin")
    S = [r for n, r in recs if n == "search"]
    Cd = [r for n, r in recs if n == "coded"]
    global SAO, FINAL, ROWS, ALF, APS
    SAO = [r for n, r in recs if n == "sao"]
    ROWS = [r for n, r in recs if n == "row"]
    ALF = [r for n, r in recs if n == "alf"]
    APS = [r for n, r in recs if n == "aps"]
    if ALF:
        # with ALF on the coding of the CTUs is simulated during the search and done for real after uvg_alf_enc_process
        # (encoderstate.c:1040-1052): every coding tree and every row is recorded twice -- the second pass is the bitstream
        assert len(Cd) == 2 * len(S) and len(ROWS) % 2 == 0
        Cd, ROWS = Cd[len(S):], ROWS[len(ROWS) // 2:]
    FINAL = [r for n, r in recs if n == "final"][0]
    src_crc = zlib.crc32(y.tobytes() + u.tobytes() + v.tobytes())
    bitstream = np.frombuffer(open(out + ".266", "rb").read(), np.uint8)
    return S, Cd, src_crc, bitstream, px


def sao_items(W, H, Cd, px):
    """The in-loop filter side of the run: per CTU the SAO decision (luma, chroma sao_info_t as 17 ints), the two SAO context
    models after the CTU's SAO syntax, the CTU's block as uvg_sao_search_lcu saw it (deblocked by the CTU's own edges only),
    and the picture the encoder returned (after deblocking + SAO)."""
    wc, hc = (W + 63) // 64, (H + 63) // 64
    info = np.zeros((hc * wc, 2, 17), np.int32)
    models = np.zeros((hc * wc, 6), np.uint16)
    snap = [np.zeros((H, W), px), np.zeros((H // 2, W // 2), px), np.zeros((H // 2, W // 2), px)]
    assert len(SAO) == wc * hc
    for r in SAO:
        cx, cy = int(r[0][1]), int(r[0][2])
        assert int(r[0][3]) == 0 and int(r[0][4]) == 1 and int(r[0][5]) == 3          # search_cabac.update, only_count, cfg.sao_type
        assert (r[2] == r[3]).all() and (r[2] == r[4]).all()                          # the decision reads the coder's models and leaves them
        k = cy * wc + cx
        info[k, 0], info[k, 1] = r[5], r[6]
        x, y = cx * 64, cy * 64
        hh, ww = min(64, H - y), min(64, W - x)
        snap[0][y:y + hh, x:x + ww] = r[7].reshape(64, 64)[:hh, :ww]
        snap[1][y // 2:(y + hh) // 2, x // 2:(x + ww) // 2] = r[8].reshape(32, 32)[:hh // 2, :ww // 2]
        snap[2][y // 2:(y + hh) // 2, x // 2:(x + ww) // 2] = r[9].reshape(32, 32)[:hh // 2, :ww // 2]
    global CODER, CODER_STATE, TREE_BYTES, TREE_OFF
    CODER = np.zeros((hc * wc, 3), np.int64)          # per CTU: bits its coding tree took in the arithmetic coder, the coder's range before / after
    CODER_STATE = np.zeros((hc * wc, 2, 5), np.int64) # per CTU: low, range, bits_left, num_buffered_bytes, buffered_byte before / after its coding tree
    chunks = [b""] * (hc * wc)
    for c in Cd:
        k = (int(c[0][2]) // 64) * wc + int(c[0][1]) // 64
        models[k] = c[3]
        CODER[k] = int(c[4][2]) - int(c[4][0]), int(c[4][1]), int(c[4][3])
        CODER_STATE[k] = c[5].reshape(2, 5)
        chunks[k] = c[6].tobytes()
    TREE_OFF = np.concatenate([[0], np.cumsum([len(b) for b in chunks])]).astype(np.int64)
    TREE_BYTES = np.frombuffer(b"".join(chunks), np.uint8)
    global ROW_BYTES, ROW_OFF
    assert len(ROWS) == hc and [int(r[0][0]) for r in ROWS] == list(range(hc)) and all(int(r[0][1]) == len(r[1]) for r in ROWS)
    ROW_OFF = np.concatenate([[0], np.cumsum([len(r[1]) for r in ROWS])]).astype(np.int64)      # the WPP substreams, row by row
    ROW_BYTES = np.concatenate([r[1] for r in ROWS])
    final = [FINAL[1].reshape(H, W), FINAL[2].reshape(H // 2, W // 2), FINAL[3].reshape(H // 2, W // 2)]
    return info, models, snap, final


def items(s, c, W, H):
    """In-picture parts of one CTU's record."""
    x, y = int(s[0][1]), int(s[0][2])
    hh, ww = min(64, H - y), min(64, W - x)
    cu = s[4].reshape(16, 16, 12)[:hh // 4, :ww // 4, :11]
    trees = s[5].reshape(16, 16, 2)[:hh // 4, :ww // 4]
    ry, ru, rv = s[6].reshape(64, 64)[:hh, :ww], s[7].reshape(32, 32)[:hh // 2, :ww // 2], s[8].reshape(32, 32)[:hh // 2, :ww // 2]
    cy = s[9].reshape(64, 64)[:hh, :ww]
    cuv = s[10].reshape(2, 32, 32)[:, :hh // 2, :ww // 2]
    return x, y, hh, ww, cu, trees, ry, ru, rv, cy, cuv


def full(W, H, depth, qp, t=0, picture=None, out_dir=None, alf=False):
    # alf: False, True (= "full") or the --alf value ("no-cc": ALF without the cross-component filter)
    alf_mode = "full" if alf is True else alf
    tag = f"{W}x{H}_{depth}_qp{qp}" + ("_alf" if alf else "") + ("_nocc" if alf_mode == "no-cc" else "")
    # (one worker thread: without threads the queue runs a job the moment it is submitted (threadqueue.c:452) and a CTU's bitstream job
    # runs before the picture's ALF job -- the .266 of such a run is not what the encoder produces with its dependencies honoured)
    S, Cd, src_crc, bs, px = run(W, H, depth, qp, t, tag, picture, extra=("alf", alf_mode, "threads", "1") if alf else ())
    wc, hc = (W + 63) // 64, (H + 63) // 64
    assert len(S) == wc * hc == len(Cd)
    models = np.zeros((hc * wc, 3, 1286), np.uint8)
    cu = np.zeros((hc * 16, wc * 16, 11), np.uint8)
    trees = np.zeros((hc * 16, wc * 16, 2), np.uint32)
    rec = [np.zeros((H, W), px), np.zeros((H // 2, W // 2), px), np.zeros((H // 2, W // 2), px)]
    coeff = np.zeros((hc * wc, 6144), np.int16)
    for s, c in zip(S, Cd):
        x, y, hh, ww, ccu, ctr, ry, ru, rv, cy, cuv = items(s, c, W, H)
        k = (y // 64) * wc + x // 64
        models[k, 0], models[k, 1], models[k, 2] = s[2][:1286], s[3][:1286], c[2][:1286]
        cu[y // 4:y // 4 + hh // 4, x // 4:x // 4 + ww // 4] = ccu
        trees[y // 4:y // 4 + hh // 4, x // 4:x // 4 + ww // 4] = ctr
        rec[0][y:y + hh, x:x + ww] = ry
        rec[1][y // 2:y // 2 + hh // 2, x // 2:x // 2 + ww // 2] = ru
        rec[2][y // 2:y // 2 + hh // 2, x // 2:x // 2 + ww // 2] = rv
        co = coeff[k]
        co[:4096].reshape(64, 64)[:hh, :ww] = cy
        co[4096:].reshape(2, 32, 32)[:, :hh // 2, :ww // 2] = cuv
    meta = np.array([W, H, depth, qp, t, int(S[0][0][3])], np.int32)
    info, sm, snap, final = sao_items(W, H, Cd, px)
    more = {}
    if alf:
        # the ALF decisions of the picture (record "alf", see alf()) and the parameter sets written in front of it (record "aps":
        # meta = frame, map index, aps_id, aps_type, new_filter_flag[2], non_linear_flag[2], num_luma_filters, num_alternatives_chroma,
        # new_cc_alf_filter[2], cc_alf_filter_count[2], alf_type; luma = coeff[25][13], clipp[25][13], filter_coeff_delta_idx[25];
        # chroma = coeff[8][7], clipp[8][7]; cc = coeff[2][4][8])
        assert len(ALF) == 1
        a, n = ALF[0], wc * hc
        more = dict(alf_meta=a[0], alf_flags=a[7].reshape(7, n), alf_set_idx=a[8], alf_luma_aps=a[9].reshape(8, -1), alf_chroma_aps=a[10], alf_cc_coeff=a[11].reshape(2, 4, 8),
                    alf_pre_y=a[1].reshape(H, W), alf_pre_u=a[2].reshape(H // 2, W // 2), alf_pre_v=a[3].reshape(H // 2, W // 2),
                    aps_meta=np.stack([r[0] for r in APS]) if APS else np.zeros((0, 16), np.int32), aps_luma=np.stack([r[1] for r in APS]) if APS else np.zeros((0, 675), np.int16),
                    aps_chroma=np.stack([r[2] for r in APS]) if APS else np.zeros((0, 112), np.int16), aps_cc=np.stack([r[3] for r in APS]) if APS else np.zeros((0, 64), np.int16))
    np.savez_compressed(os.path.join(out_dir or os.path.join(ROOT, "tests/golden"), f"ref_ctu_{tag}.npz"), **more, meta=meta, lam=S[0][1], src_crc=np.uint32(src_crc), models=models,
                        cu=cu, trees=trees, rec_y=rec[0], rec_u=rec[1], rec_v=rec[2], coeff=coeff, bitstream=bs,
                        sao=info, sao_models=sm, coder=CODER, coder_state=CODER_STATE, tree_bytes=TREE_BYTES, tree_off=TREE_OFF, row_bytes=ROW_BYTES, row_off=ROW_OFF, snap_y=snap[0], snap_u=snap[1], snap_v=snap[2], final_y=final[0], final_u=final[1], final_v=final[2])
    if not out_dir: print("wrote", tag, len(S), "CTUs")


def crcs(W, H, depth, qp, t=0):
    tag = f"{W}x{H}_{depth}_qp{qp}"
    S, Cd, src_crc, bs, px = run(W, H, depth, qp, t, tag)
    wc, hc = (W + 63) // 64, (H + 63) // 64
    out = np.zeros((hc * wc, 4), np.uint32)          # cu+trees, reconstruction, levels, models after the coder
    for s, c in zip(S, Cd):
        x, y, hh, ww, ccu, ctr, ry, ru, rv, cy, cuv = items(s, c, W, H)
        k = (y // 64) * wc + x // 64
        out[k, 0] = zlib.crc32(np.ascontiguousarray(ccu).tobytes() + np.ascontiguousarray(ctr).tobytes())
        out[k, 1] = zlib.crc32(np.ascontiguousarray(ry).tobytes() + np.ascontiguousarray(ru).tobytes() + np.ascontiguousarray(rv).tobytes())
        out[k, 2] = zlib.crc32(np.ascontiguousarray(cy).tobytes() + np.ascontiguousarray(cuv).tobytes())
        out[k, 3] = zlib.crc32(c[2][:1286].tobytes())
    meta = np.array([W, H, depth, qp, t, int(S[0][0][3])], np.int32)
    info, sm, snap, final = sao_items(W, H, Cd, px)
    fcrc = np.zeros((hc * wc, 2), np.uint32)          # per CTU: the block the SAO decision saw, the block of the final picture (Y, U, V)
    for k in range(hc * wc):
        y, x = (k // wc) * 64, (k % wc) * 64
        blk = lambda P: b"".join(np.ascontiguousarray(p[(y >> c):(y >> c) + (64 >> c), (x >> c):(x >> c) + (64 >> c)]).tobytes() for p, c in zip(P, (0, 1, 1)))
        fcrc[k] = zlib.crc32(blk(snap)), zlib.crc32(blk(final))
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_ctucrc_{tag}.npz"), meta=meta, lam=S[0][1], src_crc=np.uint32(src_crc), crc=out,
                        bitstream_crc=np.uint32(zlib.crc32(bs.tobytes())), bitstream_len=np.int64(len(bs)), sao=info, sao_models=sm, filter_crc=fcrc, coder=CODER, coder_state=CODER_STATE,
                        tree_crc=np.array([zlib.crc32(TREE_BYTES[TREE_OFF[k]:TREE_OFF[k + 1]].tobytes()) for k in range(hc * wc)], np.uint32), tree_off=TREE_OFF,
                        row_crc=np.array([zlib.crc32(ROW_BYTES[ROW_OFF[k]:ROW_OFF[k + 1]].tobytes()) for k in range(hc)], np.uint32), row_off=ROW_OFF)
    print("wrote crc", tag, len(S), "CTUs")


def stream(W, H, depth, qp, ts):
    """A whole multi-picture -p 1 stream of the encoder (no per-CTU records kept): the .266 and what it was made from."""
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{len(ts)}frames"
    yuv = f"/tmp/gold_{tag}.yuv"
    crcs = []
    with open(yuv, "wb") as f:
        for t in ts:
            y, u, v = layout.synthetic_yuv420(W, H, t, depth)
            crcs.append(zlib.crc32(y.tobytes() + u.tobytes() + v.tobytes()))
            for p in (y, u, v):
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(len(ts)), out,
                           "preset", "medium", "period", "1", "qp", str(qp)], stderr=subprocess.DEVNULL)
    bs = np.frombuffer(open(out + ".266", "rb").read(), np.uint8)
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_stream_{tag}.npz"), meta=np.array([W, H, depth, qp], np.int32), ts=np.array(ts, np.int32),
                        src_crc=np.array(crcs, np.uint32), bitstream=bs)
    print("wrote stream", tag, len(bs), "bytes")


def stream_alf(W, H, depth, qp, ts, crc_only=False):
    """A whole multi-picture -p 1 --alf full stream (one worker thread): the .266, its source pictures and per picture the ALF decisions and
    the APSs written in front of it (records "alf" / "aps" of ctu_dump.c) -- the rest of every picture follows from the source."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{len(ts)}frames_alf"
    yuv = f"/tmp/gold_{tag}.yuv"
    crcs = []
    with open(yuv, "wb") as f:
        for t in ts:
            y, u, v = helpers.varied_picture(W, H, t, depth)
            crcs.append(zlib.crc32(y.tobytes() + u.tobytes() + v.tobytes()))
            for p in (y, u, v):
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(len(ts)), out,
                           "preset", "medium", "period", "1", "qp", str(qp), "alf", "full", "threads", "1"], stderr=subprocess.DEVNULL)
    recs = read_records(out + ".bin")
    A = sorted([r for n, r in recs if n == "alf"], key=lambda r: int(r[0][0]))
    P = [r for n, r in recs if n == "aps"]
    assert len(A) == len(ts)
    n = ((W + 63) // 64) * ((H + 63) // 64)
    bs = np.frombuffer(open(out + ".266", "rb").read(), np.uint8)
    more = dict(bitstream=bs)
    if crc_only:
        # a size whose .266 is too large to keep (BASELINE configs[3]: 2160p): the parameter sets in front of the first APS NAL unit as they
        # are, of everything behind them the length and the CRC
        at = bs.tobytes().find(b"\x00\x00\x01\x00\x89")
        assert at > 0
        more = dict(bitstream_head=bs[:at].copy(), bitstream_tail_len=np.int64(len(bs) - at), bitstream_tail_crc=np.uint32(zlib.crc32(bs[at:].tobytes())))
        tag += "_crc"
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_stream_{tag}.npz"), meta=np.array([W, H, depth, qp], np.int32), ts=np.array(ts, np.int32),
                        src_crc=np.array(crcs, np.uint32), **more, alf_meta=np.stack([a[0] for a in A]), alf_flags=np.stack([a[7].reshape(7, n) for a in A]),
                        alf_set_idx=np.stack([a[8] for a in A]), alf_luma_aps=np.stack([a[9].reshape(8, -1) for a in A]), alf_chroma_aps=np.stack([a[10] for a in A]),
                        alf_cc_coeff=np.stack([a[11].reshape(2, 4, 8) for a in A]),
                        aps_meta=np.stack([r[0] for r in P]) if P else np.zeros((0, 16), np.int32), aps_luma=np.stack([r[1] for r in P]) if P else np.zeros((0, 675), np.int16),
                        aps_chroma=np.stack([r[2] for r in P]) if P else np.zeros((0, 112), np.int16), aps_cc=np.stack([r[3] for r in P]) if P else np.zeros((0, 64), np.int16))
    print("wrote alf stream", tag, len(bs), "bytes; ALF on:", [int(a[0][4]) for a in A], "luma APSs:", [int(a[0][7]) for a in A], "APSs written per picture:",
          [sum(int(r[0][0]) == i for r in P) for i in range(len(ts))])


def tiles(W, H, depth, qp, ts, cols, rows, crc_only=False, split=None):
    """A -p 1 --tiles <cols>x<rows> --wpp stream (the source pictures: helpers.varied_picture of ts): the .266, every substream in the order
    of the bitstream (per picture: tile after tile in raster order, a tile's WPP rows in order) and the pictures the encoder returned.
    Records are tile-local (ctu_dump.c reads state->tile->frame), so the per-CTU items stay out: the .266 holds every coded decision, the
    output pictures every filtered sample.  crc_only: lengths and CRCs instead of the bytes (BASELINE's sizes)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{cols}x{rows}_{len(ts)}frames" + ("_split" if split else "")
    # split = (column boundaries, row boundaries) in samples: --tiles-width-split / --tiles-height-split instead of the uniform grid
    grid_opts = ["tiles", f"{cols}x{rows}"] if not split else ["tiles-width-split", ",".join(map(str, split[0])), "tiles-height-split", ",".join(map(str, split[1]))]
    yuv = f"/tmp/gold_tiles_{tag}.yuv"
    crcs = []
    with open(yuv, "wb") as f:
        for t in ts:
            y, u, v = helpers.varied_picture(W, H, t, depth)
            crcs.append(zlib.crc32(y.tobytes() + u.tobytes() + v.tobytes()))
            for p in (y, u, v):
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_tiles_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(len(ts)), out,
                           "preset", "medium", "period", "1", "qp", str(qp)] + grid_opts + ["wpp", "1"], stderr=subprocess.DEVNULL)
    recs = read_records(out + ".bin")
    R = [r for n, r in recs if n == "row"]
    F = [r for n, r in recs if n == "final"]
    bs = open(out + ".266", "rb").read()
    wc, hc = (W + 63) // 64, (H + 63) // 64
    n_sub = hc * cols          # every tile row's CTU rows, once per tile column
    assert len(R) == n_sub * len(ts) and len(F) == len(ts)
    # the records come in the order of the bitstream: the substreams follow each other inside every slice NAL
    at = 0
    for r in R:
        at2 = bs.find(r[1].tobytes(), at)
        assert at2 >= 0, "a substream is not where the order of the records says"
        at = at2 + len(r[1])
    head = bs.find(b"\x00\x00\x01\x00\x41")
    assert head > 0
    row_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in R])]).astype(np.int64)
    finals = [np.concatenate([f[1], f[2], f[3]]) for f in F]
    more = dict(bitstream=np.frombuffer(bs, np.uint8), row_bytes=np.concatenate([r[1] for r in R]), final=np.stack(finals))
    if crc_only:
        more = dict(bitstream_head=np.frombuffer(bs[:head], np.uint8), bitstream_tail_len=np.int64(len(bs) - head), bitstream_tail_crc=np.uint32(zlib.crc32(bs[head:])),
                    row_crc=np.array([zlib.crc32(r[1].tobytes()) for r in R], np.uint32), final_crc=np.array([zlib.crc32(f.tobytes()) for f in finals], np.uint32))
        tag += "_crc"
    if split:          # the columns' widths / rows' heights in CTUs (encoder.c:452-478)
        edges = lambda b, n: np.diff([0] + [v // 64 for v in b] + [n]).astype(np.int32)
        more.update(col_ctus=edges(split[0], wc), row_ctus=edges(split[1], hc))
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_tiles_{tag}.npz"), meta=np.array([W, H, depth, qp, cols, rows], np.int32), ts=np.array(ts, np.int32),
                        src_crc=np.array(crcs, np.uint32), row_off=row_off, **more)
    print("wrote tiles", tag, len(bs), "bytes,", n_sub, "substreams per picture")


def helpers_varied():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    return helpers.varied_picture


def moving_picture(W, H, t, depth):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    return helpers.moving_picture(W, H, t, depth)


def inter(W, H, depth, qp, frames, extra=(), suffix="", with_levels=True, out_dir=None, clip=False, alf=False):
    """Inter encode -- low delay (--gop lp-g4d3t1, BASELINE configs[2]) unless `extra` names another GOP ("gop", "16": the random-access
    structure --preset medium / slow run with by default): per picture the reference lists and the picture after the in-loop
    filters, per CTU the side information incl. motion, the levels and the reconstruction before the filters -- what a reconstruction
    of the encoder's decisions (motion compensation + residual) needs.  Every per-picture array is in CODING order; `display[f]` is the
    display index (= the source picture) of coded picture f.  clip: sources from helpers.clip_picture (any length) instead of moving_picture.
    alf: the run has --alf full on (one worker thread, no frames in flight: see full()).  Every CTU is then coded twice -- simulated during the
    search, for real after uvg_alf_enc_process (encoderstate.c:1040-1052) --, and the "coded" / "row" items kept are the second pass: the
    bitstream.  Per coded picture the file also holds the decisions ALF took and the picture it received (record "alf": alf_meta, alf_flags,
    alf_set_idx, alf_luma_aps, alf_chroma_aps, alf_cc_coeff, alf_pre_y / u / v) and, in the order they were written, the APS NAL units
    (record "aps": aps_meta -- [0] = the coded picture they precede --, aps_luma, aps_chroma, aps_cc), named as stream_alf() names them.
    `final_*` is then the picture ALF left."""
    if alf:
        extra = tuple(extra) + ("alf", "full", "threads", "1", "owf", "0")
        suffix += "_alf"
    if clip:          # True / 1: helpers.clip_picture; 2: helpers.plateau_picture (helpers.CLIP_GENERATORS)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import helpers
        moving_picture = getattr(helpers, helpers.CLIP_GENERATORS[int(clip)])
    else:
        moving_picture = globals()["moving_picture"]
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{frames}frames{suffix}"
    yuv = f"/tmp/gold_inter_{tag}.yuv"
    with open(yuv, "wb") as f:
        for t in range(frames):
            for p in moving_picture(W, H, t, depth):
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_inter_{tag}"
    opt = dict(zip(extra[0::2], extra[1::2]))
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(frames), out,
                           "preset", "medium"] + ([] if "gop" in opt else ["gop", "lp-g4d3t1"]) + ["qp", str(qp)] + list(extra), stderr=subprocess.DEVNULL,
                          env=dict(os.environ, CTU_DUMP_CU_INTER="1"))
    recs = read_records(out + ".bin")
    S = [r for n, r in recs if n == "search"]
    F = sorted([r for n, r in recs if n == "final"], key=lambda r: int(r[0][0]))
    CD = {(int(r[0][0]), int(r[0][1]), int(r[0][2])): r for nm, r in recs if nm == "coded"}
    CI = [r for nm, r in recs if nm == "cuinter"]
    ROWS = [r for nm, r in recs if nm == "row"]                        # in coding order: picture by picture, row by row
    wc, hc = (W + 63) // 64, (H + 63) // 64
    n = frames * wc * hc
    meta = np.zeros((n, 8), np.int32)
    lam = np.zeros((n, 6), np.float64)
    sao = np.zeros((n, 2, 17), np.int32)
    SA = {(int(r[0][0]), int(r[0][1]), int(r[0][2])): r for nm, r in recs if nm == "sao"}
    cu = np.zeros((n, 256, 12), np.uint8)
    mot = np.zeros((n, 256, 8), np.int32)
    refs = np.zeros((n, 52), np.int32)
    rec = [np.zeros((frames, H, W), px), np.zeros((frames, H // 2, W // 2), px), np.zeros((frames, H // 2, W // 2), px)]
    coeff = np.zeros((n, 6144), np.int16)
    trees = np.zeros((n, 256, 2), np.uint32)
    models = np.zeros((n, 3, 1286), np.uint8)            # at the CTU's start / after its search / after the coder (257 models: state0, state1, rate)
    models_inter = np.zeros((n, 3, 90), np.uint8)        # the 18 models of the inter syntax beside them
    sao_models = np.zeros((n, 6), np.uint16)             # the two SAO models after the CTU's SAO syntax
    if alf:
        # per picture the rows of the simulated pass, then those of the real one (one worker thread: picture after picture)
        assert len(ROWS) == 2 * frames * hc and len([1 for nm, r in recs if nm == "coded"]) == 2 * len(S)
        assert [int(r[0][0]) for r in ROWS] == list(range(hc)) * (2 * frames)
        ROWS = [r for k, r in enumerate(ROWS) if (k // hc) & 1]
        at, bs = 0, open(out + ".266", "rb").read()
        for r in ROWS:          # ... which are the bitstream's, in this order
            at2 = bs.find(r[1].tobytes(), at)
            assert at2 >= 0, "a row of the second pass is not in the .266"
            at = at2 + len(r[1])
    assert len(ROWS) == frames * hc
    row_off = np.concatenate([[0], np.cumsum([len(r[1]) for r in ROWS])]).astype(np.int64).reshape(-1)
    row_bytes = np.concatenate([r[1] for r in ROWS])     # every WPP row's substream (emulation prevention included), pictures in coding order
    for k, s in enumerate(S):
        fr, x, y = int(s[0][0]), int(s[0][1]), int(s[0][2])
        hh, ww = min(64, H - y), min(64, W - x)
        meta[k], cu[k], mot[k], refs[k], lam[k] = s[0], s[4].reshape(256, 12), s[11].reshape(256, 8), s[12], s[1]
        trees[k] = s[5].reshape(256, 2)
        models[k, 0], models[k, 1], models[k, 2] = s[2], s[3], CD[(fr, x, y)][2]
        models_inter[k, 0], models_inter[k, 1], models_inter[k, 2] = s[13], s[14], CD[(fr, x, y)][7]
        sao_models[k] = CD[(fr, x, y)][3]
        if (fr, x // 64, y // 64) in SA:
            sao[k, 0], sao[k, 1] = SA[(fr, x // 64, y // 64)][5], SA[(fr, x // 64, y // 64)][6]
        rec[0][fr, y:y + hh, x:x + ww] = s[6].reshape(64, 64)[:hh, :ww]
        rec[1][fr, y // 2:(y + hh) // 2, x // 2:(x + ww) // 2] = s[7].reshape(32, 32)[:hh // 2, :ww // 2]
        rec[2][fr, y // 2:(y + hh) // 2, x // 2:(x + ww) // 2] = s[8].reshape(32, 32)[:hh // 2, :ww // 2]
        coeff[k, :4096] = s[9]
        coeff[k, 4096:] = s[10]
    # the encoder returns its pictures in display order ("final" is keyed by pts); the search records are in coding order: display[f] =
    # pts of coded picture f = (pts of its intra period's I picture) + its POC
    display, base = np.zeros(frames, np.int32), 0
    for k in range(len(S)):
        fr = int(meta[k][0])
        if int(meta[k][6]) == 2 and int(refs[k][51]) == 0:         # (an IDR picture restarts the count; the I picture of a later intra period of a --gop 16 run keeps its POC)
            base = fr
        display[fr] = base + int(refs[k][51])
    assert sorted(display.tolist()) == list(range(frames)), display
    final = [np.stack([F[display[f]][1 + c].reshape(H >> (c > 0), W >> (c > 0)) for f in range(frames)]) for c in range(3)]
    src_crc = np.array([zlib.crc32(b"".join(p.tobytes() for p in moving_picture(W, H, t, depth))) for t in range(frames)], np.uint32)
    more, keep_rec = {}, None
    if alf:
        keep_rec = 0          # (the reconstruction before the filters stays out: alf_pre_* and final_* are what these files are for, and each stays below 1 MB)
        A = sorted([r for nm, r in recs if nm == "alf"], key=lambda r: int(r[0][0]))
        P = [r for nm, r in recs if nm == "aps"]
        assert [int(a[0][0]) for a in A] == list(range(frames)) and all(0 <= int(r[0][0]) < frames for r in P)
        assert [int(r[0][0]) for r in P] == sorted(int(r[0][0]) for r in P)
        more = dict(alf_meta=np.stack([a[0] for a in A]), alf_flags=np.stack([a[7].reshape(7, wc * hc) for a in A]), alf_set_idx=np.stack([a[8] for a in A]),
                    alf_luma_aps=np.stack([a[9].reshape(8, -1) for a in A]), alf_chroma_aps=np.stack([a[10] for a in A]), alf_cc_coeff=np.stack([a[11].reshape(2, 4, 8) for a in A]),
                    alf_pre_y=np.stack([a[1].reshape(H, W) for a in A]), alf_pre_u=np.stack([a[2].reshape(H // 2, W // 2) for a in A]),
                    alf_pre_v=np.stack([a[3].reshape(H // 2, W // 2) for a in A]),
                    aps_meta=np.stack([r[0] for r in P]) if P else np.zeros((0, 16), np.int32), aps_luma=np.stack([r[1] for r in P]) if P else np.zeros((0, 675), np.int16),
                    aps_chroma=np.stack([r[2] for r in P]) if P else np.zeros((0, 112), np.int16), aps_cc=np.stack([r[3] for r in P]) if P else np.zeros((0, 64), np.int16))
        print("alf", tag, "on:", [a[0][4:7].tolist() for a in A], "luma APSs:", [int(a[0][7]) for a in A], "cc:", [a[0][17:19].tolist() for a in A],
              "APSs per picture:", [sum(int(r[0][0]) == i for r in P) for i in range(frames)], "slice types:", [int(a[0][26]) for a in A])
    np.savez_compressed(os.path.join(out_dir or os.path.join(ROOT, "tests/golden"), f"ref_inter_{tag}.npz"), **more, dims=np.array([W, H, depth, qp, frames], np.int32), meta=meta, cu=cu, lam=lam, sao=sao, src_crc=src_crc,
                        motion=mot, refs=refs, rec_y=rec[0][:keep_rec], rec_u=rec[1][:keep_rec], rec_v=rec[2][:keep_rec], coeff=coeff if with_levels else coeff[:0], final_y=final[0], final_u=final[1],
                        final_v=final[2], trees=trees, models=models if with_levels else models[:0], models_inter=models_inter if with_levels else models_inter[:0],
                        # every call of uvg_search_cu_inter in coding order: frame, x, y, w, h, then the decided cu_info_t fields; its two costs
                        cuinter_i=np.stack([r[0] for r in CI]).astype(np.int32) if with_levels else np.zeros((0, 20), np.int32),
                        cuinter_d=np.stack([r[1] for r in CI]) if with_levels else np.zeros((0, 2)),
                        display=display, clip=np.int32(int(clip)), gop_len=np.int32(int(opt["gop"]) if opt.get("gop", "").isdigit() else 0),      # (0: a low-delay structure)
                        sao_models=sao_models, row_bytes=row_bytes, row_off=row_off, bitstream=np.frombuffer(open(out + ".266", "rb").read(), np.uint8),
                        # the tools the run had on, for the tests' frame state: tmvp, max_merge, merge_level, bipred, fme_level, early_skip
                        cfg=np.array([int(opt.get("tmvp", 1)), int(opt.get("max-merge", 6)), 2, int(opt.get("bipred", 1)), {0: 0, 1: 1, 2: 2, 3: 3, 4: 4}[int(opt.get("subme", 4))],
                                      int(opt.get("early-skip", 1)), int(opt.get("rd", 0)), int(opt.get("owf", 0))], np.int32))
    if not out_dir: print("wrote inter", tag, n, "CTU records")
    return tag


def inter_crcs(W, H, depth, qp, frames, extra=(), suffix="", clip=False):
    """A low-delay encode at a size whose records are too large to keep (BASELINE configs[2]: 1080p): per picture its frame-level state
    and CRC-32s -- of the picture after the in-loop filters, of the reconstruction before them, of every WPP row's bytes -- and per CTU the
    CRC of its reconstruction (to localise a difference)."""
    import tempfile
    tmp = tempfile.mkdtemp()
    tag = inter(W, H, depth, qp, frames, extra=extra, suffix=suffix, out_dir=tmp, clip=clip)
    with np.load(os.path.join(tmp, f"ref_inter_{tag}.npz")) as z:
        g = {k: z[k] for k in z.files}          # (every access to the archive itself inflates the array again)
    wc, hc = (W + 63) // 64, (H + 63) // 64
    c = np.ascontiguousarray
    final_crc = np.array([zlib.crc32(c(g["final_y"][f]).tobytes() + c(g["final_u"][f]).tobytes() + c(g["final_v"][f]).tobytes()) for f in range(frames)], np.uint32)
    rec_crc = np.array([zlib.crc32(c(g["rec_y"][f]).tobytes() + c(g["rec_u"][f]).tobytes() + c(g["rec_v"][f]).tobytes()) for f in range(frames)], np.uint32)
    row_off, row_bytes = g["row_off"], g["row_bytes"]
    row_crc = np.array([zlib.crc32(row_bytes[row_off[k]:row_off[k + 1]].tobytes()) for k in range(frames * hc)], np.uint32)
    ctu_crc = np.zeros((frames, wc * hc), np.uint32)
    frame_meta, frame_lam, frame_refs = np.zeros((frames, 8), np.int32), np.zeros((frames, 6)), np.zeros((frames, 52), np.int32)
    types = np.zeros((frames, 3), np.int64)            # 4x4 units per CU type (0 outside, 1 intra, 2 inter)
    for k in range(len(g["meta"])):
        fr, x, y = (int(a) for a in g["meta"][k][:3])
        hh, ww = min(64, H - y), min(64, W - x)
        ctu_crc[fr, (y // 64) * wc + x // 64] = zlib.crc32(c(g["rec_y"][fr][y:y + hh, x:x + ww]).tobytes() + c(g["rec_u"][fr][y // 2:(y + hh) // 2, x // 2:(x + ww) // 2]).tobytes() +
                                                           c(g["rec_v"][fr][y // 2:(y + hh) // 2, x // 2:(x + ww) // 2]).tobytes())
        frame_meta[fr], frame_lam[fr], frame_refs[fr] = g["meta"][k], g["lam"][k], g["refs"][k]
        types[fr] += np.bincount(g["cu"][k][:, 0].reshape(16, 16)[:hh // 4, :ww // 4].ravel(), minlength=3)[:3]
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_intercrc_{tag}.npz"), dims=g["dims"], src_crc=g["src_crc"], meta=frame_meta, lam=frame_lam, refs=frame_refs,
                        display=g["display"], clip=g["clip"], final_crc=final_crc, rec_crc=rec_crc, row_crc=row_crc, row_len=np.diff(row_off).astype(np.int64), ctu_crc=ctu_crc, types=types,
                        bitstream_crc=np.uint32(zlib.crc32(g["bitstream"].tobytes())), bitstream_len=np.int64(len(g["bitstream"])))
    print("wrote inter crc", tag, "unit types per picture", types.tolist())


def lowdelay_states(qp, frames, extra=(), name="lowdelay"):
    """The frame-level state of a --gop lp-g4d3t1 --preset medium run (BASELINE configs[2]) picture by picture: slice type, QP, lambdas, the
    reference lists.  None of it depends on the picture size or content (no rate control): taken from a 136x72 run and used by bench.py to
    drive ONE long clip at 1080p (extra_workloads.c3_clip), for which full records would be far too large to keep."""
    import tempfile
    tmp = tempfile.mkdtemp()
    tag = inter(136, 72, 8, qp, frames, extra=extra, out_dir=tmp, with_levels=False, clip=True)
    with np.load(os.path.join(tmp, f"ref_inter_{tag}.npz")) as z:
        meta, lam, refs, display = z["meta"], z["lam"], z["refs"], z["display"]
    fm, fl, fr = np.zeros((frames, 8), np.int32), np.zeros((frames, 6)), np.zeros((frames, 52), np.int32)
    for k in range(len(meta)):
        f = int(meta[k][0])
        fm[f], fl[f], fr[f] = meta[k], lam[k], refs[k]
    # (display: the source picture of coded picture f -- the identity for a low-delay run; extra=("gop", "16"), name="gop16": --preset
    # medium's own random-access structure, bench.py's ra_clip)
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_{name}_states_qp{qp}_{frames}frames.npz"), dims=np.array([qp, frames], np.int32), meta=fm, lam=fl, refs=fr,
                        display=display)
    print("wrote", name, "states", qp, frames)


def alf(W, H, depth, qp, frames, t0, kind, threads=1):
    """All-intra encode with --alf full: around every uvg_alf_enc_process (alf.c:5193) the picture it got (deblocked + SAO) and the
    picture it left, and the decisions the reconstruction half and the syntax work from (tools/refcheck/ctu_dump.c, record "alf"):
    slice flags and APS ids, the APSs' coded coefficients, per CTU enable flags / filter set index / chroma alternative / CC-ALF control,
    the CC-ALF coefficients.  Source: helpers.varied_picture(kind * 1000 + t0 + t)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{frames}frames"
    yuv = f"/tmp/gold_alf_{tag}.yuv"
    src = [helpers.varied_picture(W, H, kind * 1000 + t0 + t, depth) for t in range(frames)]
    with open(yuv, "wb") as f:
        for pic in src:
            for p in pic:
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_alf_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(frames), out,
                           "preset", "medium", "period", "1", "qp", str(qp), "alf", "full", "threads", str(threads)], stderr=subprocess.DEVNULL)
    A = sorted([r for n, r in read_records(out + ".bin") if n == "alf"], key=lambda r: int(r[0][0]))
    assert len(A) == frames
    planes = lambda k: [np.stack([a[k + c].reshape(H >> (c > 0), W >> (c > 0)) for a in A]) for c in range(3)]
    pre, post = planes(1), planes(4)
    n = ((W + 63) // 64) * ((H + 63) // 64)
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_alf_{tag}.npz"), dims=np.array([W, H, depth, qp, frames, t0, kind], np.int32),
                        src_crc=np.array([zlib.crc32(b"".join(p.tobytes() for p in pic)) for pic in src], np.uint32),
                        meta=np.stack([a[0] for a in A]), pre_y=pre[0], pre_u=pre[1], pre_v=pre[2], post_y=post[0], post_u=post[1], post_v=post[2],
                        flags=np.stack([a[7].reshape(7, n) for a in A]), set_idx=np.stack([a[8] for a in A]), luma_aps=np.stack([a[9].reshape(8, -1) for a in A]),
                        chroma_aps=np.stack([a[10] for a in A]), cc_coeff=np.stack([a[11].reshape(2, 4, 8) for a in A]),
                        cls=np.stack([a[13].reshape((H + 3) // 4, (W + 3) // 4) for a in A]),          # the classification the luma filter worked from (zeros: no CTU filtered)
                        # the frame statistics alf_derive_stats_for_filtering gathered, per luma class / chroma plane summed over the CTUs in
                        # uvghip_alf_cov_reduce's layout (meta[29]: taken, i.e. some CTU was filtered)
                        cov_luma=np.stack([a[14].reshape(25, 1509) for a in A]), cov_chroma=np.stack([a[15].reshape(2, 1509) for a in A]),
                        bitstream=np.frombuffer(open(out + ".266", "rb").read(), np.uint8))
    fixed = A[0][12]
    np.save(os.path.join(ROOT, "tests/golden", "ref_alf_fixed.npy"), fixed.astype(np.int16))          # alf.h:46-133: 64 x 13 coefficients, 16 x 25 class -> filter
    print("wrote alf", tag, "pictures with ALF on:", [int(a[0][4]) for a in A], "CC-ALF:", [a[0][17:19].tolist() for a in A])


def merge(W, H, depth, qp, frames, every, amvp_step=4):
    """Calls of uvg_inter_get_merge_cand during a low-delay encode (every `every`-th one): everything the function reads and what it
    returned (tools/refcheck/ctu_dump.c, record "merge")."""
    px = np.uint8 if depth == 8 else np.uint16
    tag = f"{W}x{H}_{depth}_qp{qp}_{frames}frames"
    yuv = f"/tmp/gold_merge_{tag}.yuv"
    with open(yuv, "wb") as f:
        for t in range(frames):
            for p in moving_picture(W, H, t, depth):
                f.write(p.astype(px).tobytes())
    out = f"/tmp/gold_merge_{tag}"
    subprocess.check_call([os.path.join(ROOT, "tools/refcheck/ctu_dump.sh"), str(depth), yuv, str(W), str(H), str(frames), out,
                           "preset", "medium", "gop", "lp-g4d3t1", "qp", str(qp)], stderr=subprocess.DEVNULL, env=dict(os.environ, CTU_DUMP_MERGE_EVERY=str(every)))
    recs = read_records(out + ".bin")
    R = [r for n, r in recs if n == "merge"]
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_merge_{tag}.npz"), ctx=np.stack([r[0] for r in R]), lcu=np.stack([r[1].reshape(-1, 8) for r in R]),
                        col=np.stack([r[2] for r in R]), hmvp=np.stack([r[3] for r in R]), out=np.stack([r[4].reshape(6, 7) for r in R]))
    A = [r for n, r in recs if n == "amvp"][::amvp_step]
    np.savez_compressed(os.path.join(ROOT, "tests/golden", f"ref_amvp_{tag}.npz"), ctx=np.stack([r[0] for r in A]), lcu=np.stack([r[1].reshape(-1, 8) for r in A]),
                        col=np.stack([r[2] for r in A]), hmvp=np.stack([r[3] for r in A]), out=np.stack([r[4] for r in A]))
    print("wrote merge", tag, len(R), "calls; amvp", len(A), "calls")


if __name__ == "__main__":
    full(832, 480, 8, 22)
    full(416, 240, 10, 37)
    full(320, 192, 8, 42, t=5)           # high QP: empty blocks, 64x64 CUs
    full(192, 128, 10, 12, t=9)          # low QP: dense blocks, the regular-bin budget runs out
    full(256, 128, 8, 7, t=2)
    full(264, 136, 10, 32, t=26)         # 8-sample CTUs at both edges; a 64x64 CU with mode 66 (the smoothing filter's span is the CU's)
    crcs(1920, 1080, 8, 22)
    crcs(1920, 1080, 10, 27, t=3)
    crcs(3840, 2160, 10, 22)
    stream(192, 128, 8, 27, (3, 4, 5))          # three pictures of one -p 1 stream: POC, NAL types, start codes of the later pictures
    stream(136, 72, 10, 32, tuple(range(18)))   # eighteen: the 4-bit POC wraps
    inter(192, 128, 8, 17, 5)
    inter(136, 72, 10, 22, 4)
    inter(264, 136, 8, 32, 9)            # nine pictures: three reference pictures per list, a whole GOP of QP offsets
    merge(192, 128, 8, 17, 6, 3)
    inter_crcs(1920, 1080, 8, 27, 5)     # BASELINE configs[2] at full size
    inter_crcs(1920, 1080, 10, 32, 3)    # ... and at 10 bit
    inter_crcs(3840, 2160, 10, 27, 3)    # ... and at the size / depth of configs[3]
    alf(320, 192, 10, 27, 3, 7, 2)       # --alf full: new filters, chroma alternatives, CC-ALF with per-CTU controls
    alf(192, 128, 8, 27, 3, 0, 1, threads=0)    # ... a picture left alone, one on a new APS, one on the fixed filter sets only (the job order of a run without
                                                # threads leads to other decisions than the threaded flow; the process itself is the same function of its inputs)
    alf(192, 128, 10, 23, 2, 30, 1)      # ... 10 bit where the activity shift matters (cfg.input_bitdepth + 4, alf.c:5185: the runs leave it at 8 + 4)
    full(320, 192, 10, 27, t=2007, picture=helpers_varied(), alf=True)        # whole pictures of --alf full runs with everything the coder and the NAL writer need
    full(192, 128, 8, 22, t=1001, picture=helpers_varied(), alf=True)
    full(256, 128, 10, 27, t=2003, picture=helpers_varied(), alf="no-cc")      # --alf no-cc: no CC-ALF fields anywhere
    stream_alf(192, 128, 8, 27, (1000, 1001, 1002, 1003))      # four pictures of one --alf full stream: APSs of earlier pictures reused, NAL order of later access units
    merge(136, 72, 10, 27, 8, 2)
    inter(192, 128, 8, 32, 5, extra=("sao", "off"), suffix="_nosao", with_levels=False)        # final picture = the deblocked picture
    inter(136, 72, 10, 22, 4, extra=("sao", "off"), suffix="_nosao", with_levels=False)
    inter(136, 72, 8, 27, 4, extra=("bipred", "0", "tmvp", "0"), suffix="_p_notmvp")           # P pictures only, no temporal candidate
    inter(192, 128, 10, 24, 4, extra=("subme", "0", "early-skip", "0"), suffix="_subme0_noskip")   # integer motion only, no early skip
    stream_alf(3840, 2160, 10, 22, [0], crc_only=True)      # one --alf full picture at configs[3]'s size: the decisions, the .266 by CRC (bench.py 2160p10_closed_loop's ALF stage)
    lowdelay_states(27, 120)             # the frame-level state of a 120-picture low-delay clip (bench.py c3_clip)
    lowdelay_states(27, 65, extra=("gop", "16"), name="gop16")      # ... of a 65-picture random-access clip (bench.py ra_clip)
    inter_crcs(1920, 1080, 8, 27, 17, extra=("gop", "16"), suffix="_ra16", clip=True)      # the same structure at BASELINE's size, by CRC
    inter_crcs(3840, 2160, 10, 27, 17, extra=("gop", "16"), suffix="_ra16", clip=True)    # ... and at configs[3]'s size and depth
    inter_crcs(136, 72, 8, 27, 65, extra=("gop", "16"), suffix="_ra16", clip=True)        # four GOPs and the I picture of the second intra period (POC 64, coded before POC 49..63)
    inter_crcs(1920, 1080, 8, 27, 65, extra=("gop", "16"), suffix="_ra16", clip=True)     # ... bench.py's ra_clip, picture by picture
    inter(136, 72, 8, 27, 17, extra=("gop", "16"), suffix="_ra16", clip=True)      # random access, --preset medium's own GOP: coding order 0 16 8 4 2 1 3 6 5 7 12 ..., future references, five temporal layers
    inter(136, 72, 10, 22, 17, extra=("gop", "16"), suffix="_ra16", clip=True)     # ... at 10 bit, QP 22
    inter(136, 72, 8, 27, 9, extra=("gop", "8"), suffix="_ra8", clip=True)         # the 8-picture random-access GOP (what the presets up to "faster" run with): five POC bits
    inter(136, 200, 8, 27, 11, extra=("owf", "1"), suffix="_owf1", clip=3)             # frames in flight: the vectors restricted to what is final in the reference picture; content that rises ever faster
    inter(136, 72, 8, 27, 5, extra=("rd", "1"), suffix="_rd1", clip=2)                 # --preset slow = medium + rd 1 (a P / B CU never skips its intra search on a low inter cost); plateau content
    inter(136, 72, 8, 27, 33, extra=("gop", "16", "period", "16"), suffix="_ra16p16", clip=True)      # three intra periods of an open GOP: CRA pictures at POC 16 and 32, RASL pictures behind them
    tiles(264, 136, 8, 27, (3,), 2, 2)                 # --tiles 2x2 --wpp: four tiles of four sizes (2 / 3 CTU columns, 1 / 2 CTU rows), partial CTUs at the picture's edges
    tiles(416, 240, 10, 32, (2007, 11), 3, 2)          # ... 10 bit, two pictures of one stream, six tiles (2 / 2 / 3 columns: two sizes share a plan)
    tiles(320, 192, 8, 22, (1004,), 5, 1)              # ... a row of one-CTU-wide tiles: every CTU starts its row's substream... and 1 x 3:
    tiles(192, 192, 8, 37, (9,), 1, 3)                 # ... tiles one above the other, one WPP row each
    tiles(456, 264, 8, 27, (1004,), 3, 2, split=((64, 320), (192,)))      # --tiles-width-split 64,320 --tiles-height-split 192: columns of 1 / 4 / 3 CTUs, rows of 3 / 2
    tiles(1920, 1080, 8, 22, (0, 1), 2, 2, crc_only=True)      # BASELINE configs[1]'s picture in 2 x 2 tiles (bench.py tiles_clip), by CRC
    tiles(1920, 1080, 8, 22, (0, 1), 6, 4, crc_only=True)      # ... bench.py's tiles_clip: 24 tiles of 5 x 4 / 5 x 5 CTUs
    tiles(3840, 2160, 10, 22, (0,), 4, 2, crc_only=True)       # ... configs[3]'s size and depth in 4 x 2 tiles: one tile per GPU of the node
    # the QP and content extremes, and pictures smaller than one CTU
    full(136, 72, 10, 0, t=3005, picture=helpers_varied())       # white noise, 10 bit, QP 0: the largest levels, escape codes, the int16 coefficient clip
    full(200, 136, 8, 51, t=4003, picture=helpers_varied())      # lone impulses on grey at QP 51
    full(40, 24, 8, 22, t=1002, picture=helpers_varied())        # one partial CTU
    full(24, 136, 10, 37, t=7)                                   # one partial CTU column, three WPP rows
    inter(136, 72, 8, 0, 5, clip=4, suffix="_noise")              # lp-g4d3t1 at base QP 0 on full-range noise with plateaus at 0 / max
    inter(136, 72, 10, 0, 4, clip=4, suffix="_noise")             # ... at 10 bit
    inter(136, 72, 8, 51, 5, clip=True, suffix="_clip")           # every P / B picture clipped to QP 51 (rate_control.c CLIP_TO_QP)
    inter(136, 72, 10, 48, 9, extra=("gop", "8"), suffix="_ra8", clip=True)      # random access at a high QP, the QP offsets clipped
    inter(40, 24, 8, 27, 5, clip=True, suffix="_clip")            # a one-CTU picture: one partial CTU, the wavefront of one CTU (vectors leave it at the bottom)
    # --alf full in the P / B picture loop (BASELINE configs[3] as written: --gop 16 with ALF on every picture).  No clip with a partial CTU
    # had ALF on in any picture: the third one keeps the case "the SPS says ALF, every slice header says no" at such a size
    inter(192, 128, 8, 22, 17, extra=("gop", "16"), suffix="_ra16", clip=True, alf=True, with_levels=False)      # new APSs in front of P / B pictures (the ids 7..0 wrap), 2 - 3 luma APSs of earlier pictures, chroma alternatives, a picture left alone
    inter(192, 128, 10, 24, 9, clip=True, alf=True, with_levels=False)                                            # low delay, 10 bit: CC-ALF with per-CTU controls, 4 luma APSs, fixed filter sets, stale CTU flags under a slice that has ALF off
    inter(136, 72, 8, 27, 17, extra=("gop", "16"), suffix="_ra16", clip=True, alf=True, with_levels=False)       # ALF off in every picture
    if not os.environ.get("GOLDENS_SKIP_CLIP120"):      # (ten minutes and 4 GB of records by itself)
        inter_crcs(1920, 1080, 8, 27, 120, extra=("owf", "1"), suffix="_owf1", clip=True)     # bench.py's c3_clip, picture by picture: BASELINE configs[2] as written, --owf 1 (frames in flight), crosses the second intra period at POC 64
