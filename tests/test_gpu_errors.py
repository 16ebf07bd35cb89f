"""Error behaviour of the batched C ABI on a GPU box: invalid arguments return a non-zero code and leave a message in
uvghip_last_error (the strategy typedefs have no error channel, the batched ABI does); empty batches are a successful
no-op that touches no output; nothing falls back to a CPU path."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def test_invalid_arguments_are_reported(hip):
    from uvg266_amd import api
    y = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    blks = api.make_blocks([[0, 0]], [[0, 0]])
    bad = [
        ("uvghip_sad_batch", (8, _p(y), 64, _p(y), 64, 64, 64, 0, 16, _p(blks), 1, _p(out), None)),            # width 0
        ("uvghip_satd_batch", (8, _p(y), 64, _p(y), 64, 64, 64, 6, 8, _p(blks), 1, _p(out), None)),            # width % 4
        ("uvghip_transform_batch", (8, 0, 0, 0, 3, 8, 0, 0, _p(y), _p(y), 1, None)),                            # 3-point transform
        ("uvghip_mc_batch", (8, _p(y), 64, 64, 64, 0, 65, 8, _p(blks), 1, 0, _p(out), None)),                   # block wider than 64
        ("uvghip_deblock_frame", (8, _p(y), 64, None, None, 0, 62, 64, _p(blks), 16, 0, 0, 0, 22, None, None)),  # width % 4
        ("uvghip_crc32c_batch", (8, _p(y), 64, 5, _p(blks), 1, _p(out), None)),                                 # only 4x4 / 8x8
    ]
    for name, args in bad:
        fn = getattr(hip, name)
        assert len(args) == len(fn.argtypes), name
        rc = fn(*args)
        assert rc != 0, name
        assert hip.uvghip_last_error(), name
    torch.cuda.synchronize()
    assert torch.all(out == 77)                      # a refused call launched nothing


def test_intra_search_argument_checks(hip):
    from uvg266_amd import api
    y = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    blks = api.make_intra_blocks(np.array([[0, 0, 0, 0]], np.int32))
    modes = api.make_modes(list(range(67)))
    best = torch.zeros(1, dtype=torch.int8, device="cuda")
    cost = torch.zeros(1, dtype=torch.int32, device="cuda")
    f = hip.uvghip_intra_search_best_batch
    assert f(8, _p(y), 64, _p(y), 64, 12, _p(blks), 1, _p(modes), 67, _p(best), _p(cost), None, None) != 0      # 12x12 blocks
    assert f(8, _p(y), 64, _p(y), 64, 8, _p(blks), 1, _p(modes), 0, _p(best), _p(cost), None, None) != 0        # no candidates
    assert f(8, _p(y), 64, _p(y), 64, 8, _p(blks), 1, _p(modes), 67, None, _p(cost), None, None) != 0           # no output
    assert f(8, _p(y), 64, _p(y), 64, 8, _p(blks), 1, _p(modes), 67, _p(best), _p(cost), None, None) == 0
    torch.cuda.synchronize()


def test_empty_batches_are_noops(hip):
    from uvg266_amd import api
    y = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((4,), 55, dtype=torch.int32, device="cuda")
    blks = api.make_blocks([[0, 0]], [[0, 0]])
    modes = api.make_modes([0, 1])
    assert hip.uvghip_sad_batch(8, _p(y), 64, _p(y), 64, 64, 64, 16, 16, _p(blks), 0, _p(out), None) == 0
    assert hip.uvghip_satd_batch(8, _p(y), 64, _p(y), 64, 64, 64, 16, 16, _p(blks), 0, _p(out), None) == 0
    assert hip.uvghip_mc_batch(8, _p(y), 64, 64, 64, 0, 8, 8, _p(blks), 0, 0, _p(out), None) == 0
    assert hip.uvghip_intra_search_best_batch(8, _p(y), 64, _p(y), 64, 8, _p(blks), 0, _p(modes), 2, _p(out), _p(out), None, None) == 0
    assert hip.uvghip_alf_stats_batch(8, _p(y), 64, _p(y), 64, 64, 64, 0, _p(blks), 0, None, 0, _p(out), _p(out), _p(out), None) == 0
    torch.cuda.synchronize()
    assert torch.all(out == 55)


def test_unsupported_bit_depth_is_refused(hip):
    """Every entry point that picks the pixel type from `bitdepth` refuses anything but 8 and 10 (12 used to be treated as 10)."""
    from uvg266_amd import api
    y = torch.zeros((64, 64), dtype=torch.uint8, device="cuda")
    out = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    blks = api.make_blocks([[0, 0]], [[0, 0]])
    ib = api.make_intra_blocks([[0, 0, 0, 0]])
    modes = api.make_modes([0])
    calls = [
        ("uvghip_sad_batch", (12, _p(y), 64, _p(y), 64, 64, 64, 8, 8, _p(blks), 1, _p(out), None)),
        ("uvghip_satd_batch", (12, _p(y), 64, _p(y), 64, 64, 64, 8, 8, _p(blks), 1, _p(out), None)),
        ("uvghip_ssd_batch", (9, _p(y), 64, _p(y), 64, 8, 8, _p(blks), 1, _p(out), None)),
        ("uvghip_mc_batch", (12, _p(y), 64, 64, 64, 0, 8, 8, _p(blks), 1, 0, _p(out), None)),
        ("uvghip_intra_pred_batch", (12, _p(y), 64, 0, 8, 8, _p(ib), 1, _p(modes), 1, _p(out), None)),
        ("uvghip_deblock_frame", (12, _p(y), 64, None, None, 0, 64, 64, _p(blks), 16, 0, 0, 0, 22, None, None)),
        ("uvghip_transform_batch", (12, 0, 0, 0, 8, 8, 0, 0, _p(y), _p(y), 1, None)),
        ("uvghip_sao_stats_batch", (12, _p(y), 64, _p(y), 64, _p(blks), 1, _p(out), _p(out), None)),
        ("uvghip_alf_classify_frame", (12, _p(y), 64, 64, 64, 12, _p(out), 16, None)),
    ]
    for name, args in calls:
        fn = getattr(hip, name)
        assert len(args) == len(fn.argtypes), name
        assert fn(*args) != 0, name
    torch.cuda.synchronize()
    assert torch.all(out == 77)


def test_tiny_quant_blocks_are_refused(hip):
    """Blocks of fewer than 8 coefficients make the dequantiser's rounding shift non-positive."""
    c = torch.zeros((4, 2, 2), dtype=torch.int16, device="cuda")
    assert hip.uvghip_quant_batch(8, _p(c), _p(c), 2, 2, 4, 22, 0, 1, None) != 0
    assert hip.uvghip_dequant_batch(8, _p(c), _p(c), 1, 2, 4, 22, 0, None) != 0


# ---- the descriptor checks of the CTU search hosts and the loops on top of them ---------------------------------------------------------
_RW, _RH, _RWC, _RHC = 136, 72, 3, 2          # 3 x 2 CTUs, the last column and row partial


class _Desc:
    """One valid 136x72 8-bit descriptor for `entry` over zero-filled device buffers: `outer` is what the entry point takes, params / pic /
    pb are views of its parts (ctypes sub-structures share the outer structure's memory)."""

    def __init__(self, entry, bufs):
        from uvg266_amd import api, lib
        ptr = lambda t: t.data_ptr()
        self.ref_in_call = (ctypes.c_int32 * 16)(*([-1] * 16))
        self.pb = None
        if entry == "uvghip_ctu_plan_create":
            self.outer = self.pic = lib.CtuPicture()
        elif entry == "uvghip_loop_plan_create":
            self.outer = lib.LoopPicture()
            self.pic = self.outer.search
        elif entry == "uvghip_ctu_search_pb":
            self.outer = self.pb = lib.CtuPbPicture()
        else:
            self.outer = lib.LoopPbPicture()
            self.pb = self.outer.search
        if self.pb is not None:
            self.pb.params = api.ctu_params(_RW, _RH, 27)
            self.params, self.pic, p = self.pb.params, self.pb.pic, self.pb
            p.slice_type, p.poc, p.n_refs, p.frame_qp = 1, 1, 1, 27
            p.l_size[0], p.l_size[1] = 1, 0
            p.tmvp, p.max_merge, p.merge_level, p.bipred, p.fme_level, p.early_skip, p.depth_inter_min, p.depth_inter_max = 0, 6, 2, 0, 4, 1, 0, 3
            p.ref_stride, p.ref_stride_c, p.ref_motion_stride, p.inflight_margin = _RW, _RW // 2, _RWC * 16, 0
            p.ref_y[0], p.ref_u[0], p.ref_v[0], p.ref_motion[0] = ptr(bufs["ref"][0]), ptr(bufs["ref"][1]), ptr(bufs["ref"][2]), ptr(bufs["ref_mot"])
            p.inter4, p.models_inter, p.trees, p.motion_out = ptr(bufs["i4"]), ptr(bufs["mi"]), None, ptr(bufs["mot"])
        else:
            self.params = api.ctu_params(_RW, _RH, 27)
        c = self.pic
        c.src_y, c.src_u, c.src_v = (ptr(t) for t in bufs["src"])
        c.rec_y, c.rec_u, c.rec_v = (ptr(t) for t in bufs["rec"])
        c.src_stride, c.src_stride_c, c.rec_stride, c.rec_stride_c = _RW, _RW // 2, _RW, _RW // 2
        c.cu, c.cu_stride, c.coeff, c.models = ptr(bufs["scu"]), _RWC * 16, ptr(bufs["co"]), ptr(bufs["mo"])
        if hasattr(self.outer, "out_y"):
            self.outer.out_y, self.outer.out_u, self.outer.out_v = (ptr(t) for t in bufs["out"])
            self.outer.out_stride, self.outer.out_stride_c = _RW, _RW // 2


def _set(path, value):
    """A case: set one field, named by its path from the _Desc (an index in brackets is spelled as a tuple element)."""
    def breaker(d):
        obj = d
        for name in path[:-1]:
            obj = obj[name] if isinstance(name, int) else getattr(obj, name)
        if isinstance(path[-1], int):
            obj[path[-1]] = value(d) if callable(value) else value
        else:
            setattr(obj, path[-1], value(d) if callable(value) else value)
    return breaker


_BREAK = {
    "rec_y NULL": _set(("pic", "rec_y"), None),
    "src_stride": _set(("pic", "src_stride"), _RW - 8),
    "cu_stride": _set(("pic", "cu_stride"), 16 * _RWC - 1),
    "pic_w 132": _set(("params", "pic_w"), 132),
    "depth_max 3": _set(("params", "depth_max"), 3),
    "qp_c": _set(("params", "qp_c"), lambda d: d.params.qp + 1),
    "out_y NULL": _set(("outer", "out_y"), None),
    "out_stride": _set(("outer", "out_stride"), _RW - 8),
    "frame_qp": _set(("pb", "frame_qp"), lambda d: d.params.qp + 1),
    "l[0][0]": _set(("pb", "l", 0, 0), lambda d: d.pb.n_refs),
    "ref_y[0] NULL": _set(("pb", "ref_y", 0), None),
    "inflight_margin 65": _set(("pb", "inflight_margin"), 65),
    "ref_in_call[0] 0": _set(("ref_in_call", 0), 0),
}
_PLAN, _PB = "uvghip_ctu_plan_create: ", "uvghip_ctu_search_pb: "
_PLAN_CASES = [("rec_y NULL", _PLAN + "picture descriptor"), ("src_stride", _PLAN + "a sample stride is smaller than the picture"), ("cu_stride", _PLAN + "picture descriptor"),
               ("pic_w 132", _PLAN + "picture size"), ("depth_max 3", None)]          # (None: accepted -- the all-intra plan takes pu-depth-intra 1-3)
_PB_CASES = [("rec_y NULL", _PB + "picture descriptor"), ("src_stride", _PB + "picture descriptor"), ("cu_stride", _PB + "picture descriptor"), ("pic_w 132", _PB + "picture size"),
             ("depth_max 3", _PB + "configuration outside the supported subset"), ("l[0][0]", _PB + "a reference list entry is out of range"),
             ("ref_y[0] NULL", _PB + "a reference picture is missing"), ("inflight_margin 65", _PB + "inflight_margin")]
_REFUSALS = {
    "uvghip_ctu_plan_create": _PLAN_CASES,
    "uvghip_loop_plan_create": _PLAN_CASES + [("qp_c", "uvghip_loop_plan_create: qp_c != qp needs a chroma QP table"), ("out_y NULL", "uvghip_loop_plan_create: output planes"),
                                              ("out_stride", "uvghip_loop_plan_create: output strides")],
    "uvghip_ctu_search_pb": _PB_CASES,
    "uvghip_loop_pb_run": _PB_CASES + [("qp_c", "uvghip_loop_pb_run: qp_c != qp needs a chroma QP table"), ("out_y NULL", "uvghip_loop_pb_run: output planes"),
                                       ("out_stride", "uvghip_loop_pb_run: output planes"), ("frame_qp", "uvghip_loop_pb_run: params.qp differs from frame_qp")],
    "uvghip_loop_pb_run_inflight": _PB_CASES + [("qp_c", "uvgi_search_pb_inflight: qp_c != qp or params.qp != frame_qp"), ("out_y NULL", "uvghip_loop_pb_run_inflight: output planes"),
                                                ("out_stride", "uvghip_loop_pb_run_inflight: output planes"),
                                                ("frame_qp", "uvgi_search_pb_inflight: qp_c != qp or params.qp != frame_qp"),
                                                ("ref_in_call[0] 0", "uvgi_search_pb_inflight: a reference inside the call must be an earlier picture of it")],
}


def _call(hip, entry, d, ws):
    """The entry point on the descriptor; a plan that was created is dropped again."""
    ref = ctypes.byref
    if entry in ("uvghip_ctu_plan_create", "uvghip_loop_plan_create"):
        plan = ctypes.c_void_p()
        if entry == "uvghip_ctu_plan_create":
            rc = hip.uvghip_ctu_plan_create(8, ref(d.params), ref(d.outer), 1, _p(ws), ref(plan))
        else:
            rc = hip.uvghip_loop_plan_create(8, ref(d.params), ref(d.outer), 1, 3, _p(ws), ref(plan))
        assert bool(plan.value) == (rc == 0), entry
        if plan.value:
            (hip.uvghip_ctu_plan_destroy if entry == "uvghip_ctu_plan_create" else hip.uvghip_loop_plan_destroy)(plan)
        return rc
    if entry == "uvghip_ctu_search_pb":
        return hip.uvghip_ctu_search_pb(8, ref(d.outer), 1, _p(ws), None)
    if entry == "uvghip_loop_pb_run":
        return hip.uvghip_loop_pb_run(8, ref(d.outer), 1, 3, _p(ws), None)
    return hip.uvghip_loop_pb_run_inflight(8, ref(d.outer), 1, 3, ref(d.ref_in_call), _p(ws), None)


@pytest.mark.parametrize("entry", list(_REFUSALS))
def test_descriptor_refusals_of_the_search_hosts_and_loops(hip, entry):
    """One valid descriptor per entry point, one field broken per case: the call is refused by host code, before any launch, with the text
    the entry point has always given for it; then the valid descriptor still runs in the workspace the refused calls were given (a call
    refused half-way would have left work enqueued on it)."""
    z = lambda shape, dt=torch.uint8: torch.zeros(shape, dtype=dt, device="cuda")
    planes = lambda: [z((_RH >> c, _RW >> c)) for c in (0, 1, 1)]
    ctus, n4 = _RWC * _RHC, _RHC * 16 * _RWC * 16
    bufs = dict(src=planes(), rec=planes(), out=planes(), ref=planes(), scu=z(n4 * 32), co=z(ctus * 6144, torch.int16), mo=z(ctus * 3 * 257, torch.int32),
                mi=z(ctus * 3 * 18, torch.int32), i4=z(n4 * 8), mot=z(n4 * 8, torch.int32), ref_mot=z(n4 * 8, torch.int32))
    size = {"uvghip_ctu_plan_create": lambda: hip.uvghip_ctu_search_workspace_bytes(1, _RW, _RH),
            "uvghip_loop_plan_create": lambda: hip.uvghip_loop_workspace_bytes(8, 1, _RW, _RH),
            "uvghip_ctu_search_pb": lambda: hip.uvghip_ctu_search_pb_workspace_bytes(1, _RW, _RH),
            "uvghip_loop_pb_run": lambda: hip.uvghip_loop_pb_workspace_bytes(8, 1, _RW, _RH),
            "uvghip_loop_pb_run_inflight": lambda: hip.uvghip_loop_pb_inflight_workspace_bytes(8, 1, _RW, _RH)}[entry]()
    assert size > 0
    ws = z(size)
    for case, text in _REFUSALS[entry]:
        d = _Desc(entry, bufs)
        _BREAK[case](d)
        rc = _call(hip, entry, d, ws)
        if text is None:
            assert rc == 0, (entry, case, hip.uvghip_last_error().decode())
        else:
            assert rc != 0, (entry, case)
            assert text in hip.uvghip_last_error().decode(), (entry, case, hip.uvghip_last_error().decode())
    assert _call(hip, entry, _Desc(entry, bufs), ws) == 0, (entry, hip.uvghip_last_error().decode())
    torch.cuda.synchronize()
