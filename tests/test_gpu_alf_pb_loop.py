"""ALF in the P / B picture loop (BASELINE configs[3] as written: --gop 16 --alf full): api.LowDelayLoop(alf=decide) -- every picture's loop
(search -> deblocking -> SAO) followed by its ALF stage (uvghip_loop_plan_alf_stage for an I picture, uvghip_loop_pb_alf_stage for P / B
pictures) before anything that references it is issued, the slice data coded with the CTU-level ALF syntax in P / B slices
(uvghip_encode_slice_rows_pb_alf), the NAL units from uvghip_write_picture_nals_gop_alf.  `decide` replays the decisions of real runs
(tests/golden/ref_inter_*_alf.npz): the derivation itself is not part of the library.

Pictures of 3 x 2 CTUs.  No golden exercises ALF at a partial CTU (every clip with partial CTUs that was tried kept ALF off in all pictures):
the 136x72 golden runs the partial-CTU geometry with ALF on in the SPS and off in every slice."""
import ctypes

import numpy as np
import pytest

import alf_pb_helpers as A
import helpers as H

pytestmark = pytest.mark.gpu


def frame_rows(g):
    ks = [g["_first"][f] for f in range(int(g["dims"][4]))]
    return g["meta"][ks], g["lam"][ks], g["refs"][ks]


def replay(g, calls):
    def decide(f, s, stats):
        calls.append((f, s))
        p = A.picture_decisions(g, f)
        m = p["meta"]
        return dict(alf_type=int(m[3]), enabled=[int(a) for a in m[4:7]], n_luma_aps=int(m[7]), luma_aps=p["luma_aps"], chroma_aps=p["chroma_aps"],
                    cc_enabled=[int(a) for a in m[17:19]], cc_filter_count=[int(a) for a in m[19:21]], cc_coeff=p["cc_coeff"], ctu_flags=p["flags"], filter_set_idx=p["set_idx"])
    return decide


def device_sources(g, n_seq):
    import torch
    pics = H.golden_sources(A.Files(g))
    return [[tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pics[f]) for f in range(len(pics))] for _ in range(n_seq)]


@pytest.mark.parametrize("name,n_seq,by_level", [(A.GOLDENS[0], 1, False), (A.GOLDENS[1], 1, False), (A.GOLDENS[2], 1, False), (A.GOLDENS[0], 2, True)])
def test_a_stream_with_alf_in_its_p_and_b_pictures_through_the_loop(hip, name, n_seq, by_level):
    """Per coded picture: the picture ALF got, the picture it left (what later pictures predict from: the first B picture differs otherwise),
    the rows, and -- from device outputs only -- the NAL units; with the encoder's parameter sets they are its .266.  by_level: the P / B
    pictures of a DAG level share one loop call and one stage call.  The rows are those of the encoder's SECOND coding pass (after ALF), whose
    history tables start from what the first pass left (uvghip_slice_pb_t::second_pass): without that, picture 1's first row is 3 bytes longer."""
    import torch
    from uvg266_amd import api
    g = A.golden(name)
    W, Hh, depth, qp0, frames = (int(a) for a in g["dims"])
    hc = (Hh + 63) // 64
    states = H.frame_states_from_records(*frame_rows(g))
    src = device_sources(g, n_seq)
    calls = []
    loop = api.LowDelayLoop(W, Hh, depth, n_seq, states, src, by_level=by_level, alf=replay(g, calls), alf_shift=int(g["alf_meta"][0][28]) + 4)
    loop.run()
    torch.cuda.synchronize()
    assert sorted(calls) == [(f, s) for f in range(frames) for s in range(n_seq)]
    stream = g["bitstream"].tobytes()
    mine, irap_poc = b"", 0
    for f in range(frames):
        rows, nb = loop.rows[f].cpu().numpy(), loop.row_bytes[f].cpu().numpy()
        off = g["row_off"][f * hc:f * hc + hc + 1]
        for s in range(n_seq):
            for c, k in enumerate(("alf_pre_y", "alf_pre_u", "alf_pre_v")):
                assert np.array_equal(loop.sao_out[f][s][c].cpu().numpy(), g[k][f]), (name, f, s, "the picture ALF gets", k)
            for c, k in enumerate(("final_y", "final_u", "final_v")):
                assert np.array_equal(loop.out[f][s][c].cpu().numpy(), g[k][f]), (name, f, s, "the picture ALF leaves", k)
            for r in range(hc):
                want = g["row_bytes"][off[r]:off[r + 1]]
                assert nb[s, r] == len(want) and np.array_equal(rows[s, r, :nb[s, r]], want), (name, f, s, "row", r, int(nb[s, r]), len(want))
        s = n_seq - 1
        sums = api.picture_checksum(*loop.out[f][s]).cpu().numpy().view(np.uint32)
        sizes = np.ascontiguousarray(nb[s], np.int32)
        mine += A.write_picture(hip, g, f, np.ascontiguousarray(rows[s, :, :int(sizes.max())]), sizes, sums, irap_poc)
        if states[f]["slice_type"] == 2:
            irap_poc = states[f]["poc"]
    at = A.parameter_sets_end(stream)
    assert stream[:at] + mine == stream, "the encoder's parameter sets + the device's pictures (APS, slice, hash SEI) = the encoder's .266"


def test_all_zero_decisions_code_the_rows_of_the_plain_p_b_coder(hip):
    """uvghip_encode_slice_rows_pb_alf with nothing enabled (and no flag arrays at all) on a B picture of a run WITHOUT ALF: no ALF bin, the
    golden's rows.  (second_pass stays 0: that run coded its CTUs once.  The stage sets it for every picture of an --alf run, whose rows the
    136x72 golden holds with ALF off in every slice.)"""
    import torch
    from uvg266_amd import api, lib
    name = "ref_inter_192x128_8_qp17_5frames"
    g = A.golden(name)
    W, Hh, depth, qp0, frames = (int(a) for a in g["dims"])
    hc = (Hh + 63) // 64
    states = H.frame_states_from_records(*frame_rows(g))[:2]
    src = [device_sources(g, 1)[0][:2]]
    loop = api.LowDelayLoop(W, Hh, depth, 1, states, src)
    loop.run()
    torch.cuda.synchronize()
    kind, arr, ws, bufs = loop.steps[1]
    assert kind == "PB" and states[1]["slice_type"] != 2
    s = arr[0].search
    pb = lib.SlicePb()
    pb.slice_type, pb.poc, pb.n_refs, pb.tmvp, pb.max_merge, pb.merge_level, pb.frame_qp = s.slice_type, s.poc, s.n_refs, s.tmvp, s.max_merge, s.merge_level, s.frame_qp
    for i in range(16):
        pb.ref_pocs[i], pb.l[0][i], pb.l[1][i] = s.ref_pocs[i], s.l[0][i], s.l[1][i]
    pb.l_size[0], pb.l_size[1] = s.l_size[0], s.l_size[1]
    pb.col, pb.col_stride, pb.inter4, pb.models_inter = s.ref_motion[s.l[0][0]], s.ref_motion_stride, s.inter4, s.models_inter
    alf = lib.SliceAlf()
    alf.alf_type = 2
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    lib.check(hip.uvghip_loop_pb_results(depth, 1, W, Hh, ws.data_ptr(), ctypes.byref(a), ctypes.byref(b), None, None, None, None), "uvghip_loop_pb_results")
    row_cap = 3 * 64 * W
    out = torch.zeros((hc, row_cap), dtype=torch.uint8, device="cuda")
    nbytes = torch.zeros(hc, dtype=torch.int32, device="cuda")
    cws = torch.zeros(hip.uvghip_slice_rows_pb_alf_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    assert cws.numel() > 0
    pic = s.pic
    lib.check(hip.uvghip_encode_slice_rows_pb_alf(depth, ctypes.byref(s.params), ctypes.byref(pic), ctypes.byref(pb), ctypes.byref(alf), 1, a, b, cws.data_ptr(), out.data_ptr(),
                                                  row_cap, nbytes.data_ptr(), torch.cuda.current_stream().cuda_stream), "uvghip_encode_slice_rows_pb_alf")
    torch.cuda.synchronize()
    rows, nb = out.cpu().numpy(), nbytes.cpu().numpy()
    off = g["row_off"][hc:2 * hc + 1]
    for r in range(hc):
        want = g["row_bytes"][off[r]:off[r + 1]]
        assert nb[r] == len(want) and np.array_equal(rows[r, :nb[r]], want), (name, "row", r, int(nb[r]), len(want))
    assert np.array_equal(rows[:, :int(nb.max())], loop.rows[1][0].cpu().numpy()[:, :int(nb.max())])          # ... which uvghip_encode_slice_rows_pb wrote too


def test_alf_with_pictures_in_flight_is_refused():
    """The derivation needs the whole picture's statistics, and later pictures predict from the ALF output: no picture can start on CTUs of a
    reference whose ALF stage has not run."""
    from uvg266_amd import api
    g = A.golden(A.GOLDENS[2])
    states = H.frame_states_from_records(*frame_rows(g))
    with pytest.raises(ValueError, match="whole picture"):
        api.LowDelayLoop(int(g["dims"][0]), int(g["dims"][1]), int(g["dims"][2]), 1, states, None, inflight=True, inflight_margin=11, alf=lambda f, s, stats: None)
