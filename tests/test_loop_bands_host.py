"""The row-sharded closed loop without a GPU: the hand-over list of a band (bands.BandLayout.halo_loop) executed by 2 and 3 gloo processes
on CPU tensors, its bytes against what include/uvg266_hip.h documents for uvghip_loop_plan_halo_bytes, and what the new entry points
refuse without a device.  (The bands against the encoder's records: tests/test_gpu_loop_bands.py.)"""
import ctypes
import os
import socket
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("y", "u", "v", "scu", "models", "dbk_y", "dbk_u", "dbk_v", "sao_info", "sao_models")


def documented_halo_bytes(bitdepth, n_pictures, pic_w, sao_type):
    """include/uvg266_hip.h, uvghip_loop_plan_halo_bytes -- restated, not imported."""
    b, wc = (1 if bitdepth == 8 else 2), (pic_w + 63) // 64
    return n_pictures * (b * 24 * pic_w + 2048 * wc + 4 * 257 + (b * 5 * pic_w + 136 * wc + 12 if sao_type else 0))


def tables(torch, W, height, bitdepth, fill):
    """The named 2-D tensors of one picture as the device holds them (element types of the real buffers), every element `fill`."""
    wc, hc = (W + 63) // 64, (height + 63) // 64
    px = torch.uint8 if bitdepth == 8 else torch.int16
    mk = lambda shape, dt: torch.full(shape, fill, dtype=dt)
    return dict(y=mk((height, W), px), u=mk((height // 2, W // 2), px), v=mk((height // 2, W // 2), px), scu=mk((hc * 16, wc * 16 * 32), torch.uint8),
                models=mk((3 * wc * hc, 257), torch.int32), dbk_y=mk((height, W), px), dbk_u=mk((height // 2, W // 2), px), dbk_v=mk((height // 2, W // 2), px),
                sao_info=mk((hc, wc * 34), torch.int32), sao_models=mk((wc * hc, 6), torch.int16))


def expected_rows(b, wc, sao_type):
    """What a band whose first CTU row is b reads of the band above, per table: [row0, row1) -- from the kernels, not from halo_loop:
    the tile starts 16 luma rows up (ctu_filter.h), its edges read the units of those rows, the output rows start 10 up and the edge
    classes look one row further, the band's own deblocked rows start 8 up; decisions of the CTU row above; models of its first CTU."""
    Y, k = 64 * b, (b - 1) * wc
    rows = dict(y=(Y - 16, Y), u=(Y // 2 - 8, Y // 2), v=(Y // 2 - 8, Y // 2), scu=(Y // 4 - 4, Y // 4), models=(3 * k + 2, 3 * k + 3))
    if sao_type:
        rows.update(dbk_y=(Y - 11, Y - 8), dbk_u=((Y - 11) // 2, (Y - 8) // 2), dbk_v=((Y - 11) // 2, (Y - 8) // 2), sao_info=(b - 1, b), sao_models=(k, k + 1))
    return rows


def _worker(rank, nranks, port, W, height, bitdepth, sao_type, q):
    import torch
    import torch.distributed as dist
    from uvg266_amd import bands
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=nranks)
    try:
        wc = (W + 63) // 64
        lay = bands.BandLayout(height, nranks, rank)
        t = tables(torch, W, height, bitdepth, rank + 1)          # everything this rank holds carries rank + 1
        ops = lay.halo_loop(*(t[k] for k in NAMES), wc, sao_type=sao_type)
        sent, received = bands.spec_bytes(ops)
        want = documented_halo_bytes(bitdepth, 1, W, sao_type)
        ok = sent == (want if rank + 1 < nranks else 0) and received == (want if rank else 0)
        ok &= bands.halo_loop_bytes(bitdepth, 1, W, sao_type) == want
        bands.TorchTransport(dist).exchange(ops)
        exp = expected_rows(lay.ctu_row0, wc, sao_type) if rank else {}
        for name in NAMES:
            a, b = exp.get(name, (0, 0))
            ok &= bool((t[name][a:b] == rank).all())                                             # every listed row arrived from the band above
            ok &= bool((t[name][:a] == rank + 1).all() and (t[name][b:] == rank + 1).all())      # and nothing else changed
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("nranks,W,height,bitdepth,sao_type", [(2, 200, 136, 8, 3), (3, 832, 480, 10, 3), (2, 416, 240, 10, 0), (3, 24, 192, 8, 1)])
def test_loop_halo_goes_down_one_band_over_gloo(nranks, W, height, bitdepth, sao_type):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, nranks, port, W, height, bitdepth, sao_type, q)) for r in range(nranks)]
    for p in ps:
        p.start()
    got = sorted(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(60)
    assert got == [(r, True) for r in range(nranks)]


def test_the_documented_bytes_of_the_two_sizes_of_the_design_note():
    """DESIGN.md section 6 quotes these: one boundary, one picture."""
    assert documented_halo_bytes(8, 1, 1920, 3) == 122240
    assert documented_halo_bytes(10, 1, 3840, 3) == 354800
    assert documented_halo_bytes(8, 1, 1920, 0) == 108548


def test_what_needs_no_plan_is_refused_without_a_device():
    from uvg266_amd import lib
    L = lib.load_library()
    n, a, b = ctypes.c_int(-5), ctypes.c_int(), ctypes.c_int()
    piece = (lib.HaloPiece * 1)()
    assert L.uvghip_loop_plan_halo(None, 0, piece, 1, ctypes.byref(n)) != 0 and b"uvghip_loop_plan_halo" in L.uvghip_last_error()
    assert L.uvghip_loop_plan_out_rows(None, ctypes.byref(a), ctypes.byref(b)) != 0 and b"uvghip_loop_plan_out_rows" in L.uvghip_last_error()
    assert L.uvghip_loop_plan_halo_bytes(None) == 0


def test_no_device_is_an_error_of_the_band_entry_points():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    from uvg266_amd import api, lib
    L = lib.load_library()
    P = api.ctu_params(200, 136, 27)
    pics = (lib.LoopPicture * 1)()
    plan = ctypes.c_void_p()
    ws = ctypes.create_string_buffer(64)
    assert L.uvghip_loop_plan_create_rows(8, ctypes.byref(P), pics, 1, 3, 1, 2, ws, ctypes.byref(plan)) != 0
    assert b"uvghip_loop_plan_create_rows" in L.uvghip_last_error() and not plan.value
    for fn in ("uvghip_loop_plan_halo_pack", "uvghip_loop_plan_halo_unpack"):
        assert getattr(L, fn)(None, ws, None) != 0 and fn.encode() in L.uvghip_last_error()


class RecordedBand:
    """What api.ClosedLoop(rows=...).substreams() returns for a band, cut out of the encoder's own record (no GPU): the band's slice rows
    and the checksum terms of the output rows it writes (position-dependent: the mask takes the sample's place in the PICTURE)."""
    sao_type = 3

    def __init__(self, g, hc):
        self.g, self.hc = g, hc

    def substreams(self, rows):
        import numpy as np
        g, (r0, r1) = self.g, rows
        Hh, depth = int(g["meta"][1]), int(g["meta"][2])
        y0, y1 = (64 * r0 - 10 if r0 else 0), (Hh if r1 == self.hc else 64 * r1 - 10)
        off = g["row_off"]
        lens = np.zeros((1, self.hc), np.int32)
        lens[0, r0:r1] = np.diff(off)[r0:r1]
        sums = np.zeros((1, 3), np.uint32)
        for c, k in enumerate(("final_y", "final_u", "final_v")):
            sh = 1 if c else 0
            v = g[k].astype(np.int64)[y0 >> sh:y1 >> sh]
            ys, xs = np.mgrid[y0 >> sh:y1 >> sh, 0:v.shape[1]]
            m = (xs ^ ys ^ (xs >> 8) ^ (ys >> 8)) & 0xFF
            sums[0, c] = int(((v & 0xFF) ^ m).sum() + (((v >> 8) & 0xFF) ^ m).sum() * (depth > 8)) & 0xFFFFFFFF
        return lens, np.ascontiguousarray(g["row_bytes"][off[r0]:off[r1]]), sums


def _gather_worker(rank, nranks, port, name, q):
    import numpy as np
    import torch.distributed as dist
    from uvg266_amd import bands
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=nranks)
    try:
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        Hh = int(g["meta"][1])
        lay = bands.BandLayout(Hh, nranks, rank)
        nals = bands.gather_band_nals(RecordedBand(g, (Hh + 63) // 64), (lay.ctu_row0, lay.ctu_row1))
        assert (nals is None) == (rank != 0)
        if rank == 0:
            q.put(b"".join(nals))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name,nranks", [("ref_ctu_416x240_10_qp37", 2), ("ref_ctu_832x480_8_qp22", 3)])
def test_the_bands_rows_and_checksum_terms_make_up_the_encoders_file(name, nranks):
    """bands.gather_band_nals over gloo: every rank contributes its band's rows and the checksum terms of the output rows it writes (the
    rectangles of uvghip_loop_plan_out_rows tile the picture), rank 0 writes the NAL units: the tail of the encoder's .266."""
    import numpy as np
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gather_worker, args=(r, nranks, port, name, q)) for r in range(nranks)]
    for p in ps:
        p.start()
    got = q.get(timeout=120)
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    stream = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))["bitstream"].tobytes()
    assert stream[stream.find(b"\x00\x00\x01\x00\x41"):] == got
