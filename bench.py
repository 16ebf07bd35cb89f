#!/usr/bin/env python3
"""bench.py -- uvg266's per-CTU hot path on MI355X: closed-loop all-intra encode rate and the kernels under it.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times the K steps and prints the result line: `value`, `ms_per_step`, `roofline` (from the HIP events
of the timed steps).  --dump-outputs DIR also writes what the last timed step computed (dump_outputs).  Everything else below --
the parity check against the reference encoder's record, extra_workloads, cpu_baseline, and with --gpus N > 1 row_sharded_rccl --
runs only with --full.

One "step" = one synthetic 1920x1080 8-bit yuv420p picture (BASELINE.json configs[1]: -p 1 --preset medium, QP 22), already
resident in HBM, taken through the CLOSED loop the reference runs per CTU: uvghip_ctu_search_intra (one workgroup per CTU on
the WPP wavefront: rough intra search with the reference's candidate schedule, reconstruction from the reconstructed
neighbours, RDOQ, CABAC bit costs on evolving models, split / no-split RD decisions over depths 1-4 plus the 64x64 candidate,
the coder's model adaptation) -> deblocking on the side information the search wrote -> SAO statistics / offsets / apply.
The decisions, levels and reconstruction are bit-identical with the reference encoder's (tests/golden/ref_ctu*).  Pictures of
an all-intra encode are independent: K pictures are issued `--in-flight` at a time (the reference's --owf), their wavefronts
interleaved on the device.  The arithmetic coder runs on the device as the last thing of every group (uvghip_encode_slice_rows: the
slice data of the encoder's .266, byte for byte); the parameter sets and NAL framing are host code (uvghip_write_picture_nals).

`value` = pictures/s of that closed loop.  The open-loop throughput of the same block kernels (every block size of every
picture, no decisions: the previous rounds' headline) is reported under "open_loop"; "extra_workloads" holds the 2160p 10-bit closed
loop and BASELINE configs[2] -- low-delay P / B sequences through the closed loop with the inter search on the device
(c3_low_delay_closed_loop, parity-checked against the reference's own 1080p run) beside the open-loop motion search kernels; and
reference_cli_frame_handover: the reference encoder's own CLI (oracle/_ref/uvg266_8_hip) on cpu_baseline's pictures with its all-intra frames
handed to uvghip_frame_pool_* (UVG266_HIP_FRAME=1), its .266 compared with the CPU run's.  --gpus N > 1: ranks take whole pictures (no data-path collective; "weak"); the CTU-row sharded filter
chain over RCCL (uvghip_band_plan) is timed in the same run on 2160p10alf and reported under "row_sharded_rccl".
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from uvg266_amd import api, bands, layout, lib, pipeline  # noqa: E402
from uvg266_amd.pipeline import MODES, SIZES, WORKLOADS  # noqa: E402

QP = 22
HBM_PEAK_GBS = 8000.0             # MI355X_MICROARCH.md: 8 TB/s spec (6.3 TB/s achievable)
N_SIMD, CLOCK_GHZ = 1024, 2.4     # 256 CUs x 4 SIMDs; peak engine clock
# Integer VALU issue: one wave64 instruction per 4 cycles per SIMD for the full-rate integer ops the search kernel is
# made of (v_add3 / v_perm / v_sad / v_pk_* : tools/dev/valu_rate.hip, profiles/r02_microbench.txt; fp32 FMA is 2).
CYC_PER_INT_VALU = 4
VALU_PEAK_GINST = N_SIMD * CLOCK_GHZ / CYC_PER_INT_VALU          # 614.4 G wave-instructions/s


def _load_json(name):
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            return json.load(f)
    except OSError:
        return {}


TRAFFIC = _load_json("hbm_traffic_latest.json")   # HBM bytes per launch: PMC passes (FETCH_SIZE doubled per the guide + WRITE_SIZE)
VALU = _load_json("valu_latest.json")             # SQ_INSTS_VALU per launch


def workload_text(wl, shard, world):
    alf = ("-> ALF classification -> ALF covariance statistics per CTU and class (i8 MFMA, compact records) + per-class frame "
           "sums -> ALF 7x7 luma / 5x5 chroma filters " if wl["alf"] else "")
    sh = "" if world == 1 else (f"; each picture sharded over {world} ranks by CTU rows, halos + reconstructed bands over RCCL"
                                if shard == "rows" else f"; whole pictures sharded over {world} ranks")
    return (f"{wl['W']}x{wl['H']} {wl['depth']}-bit yuv420p, all-intra medium hot path per frame: for N in 32,16,8,4 "
            "{luma rough search 67 modes min(SATD,2SAD) on all NxN blocks with fused arg-min -> luma predict -> TU round trip "
            + ("residual/DCT-2 -> RDOQ (uvg_rdoq, synthetic context snapshot) -> dequant/IDCT/recon" if wl.get("rdoq") else
               "fused residual/DCT-2/quant/dequant/IDCT/recon") +
            "; N>=8: chroma (N/2) predict U,V with the derived mode -> chroma TU round trip U,V}; then deblock (Y,U,V; seeded random quad-tree partition) -> SAO statistics / offsets / apply (Y,U,V) "
            f"{alf}; open-loop references (source picture); CABAC bitstream writing excluded (out of hot-path scope){sh}")


class KernelClock:
    """Per-kernel HIP-event timing on the stream the kernel is launched on.  `only` restricts the instrumentation to
    kernel families in the set (None = all).  Events are recycled: a few hundred live timing events make every later
    HIP call slow on this runtime."""

    def __init__(self):
        self.ms, self.pending, self.pool, self.only = {}, {}, [], None

    def _event(self):
        return self.pool.pop() if self.pool else torch.cuda.Event(enable_timing=True)

    def launch(self, name, fn, args, stream, slot=0):
        timed = self.only is None or family(name) in self.only
        if timed:
            e0, e1 = self._event(), self._event()
            e0.record(stream)
        rc = fn(*args, stream.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"{name} failed ({rc}): {lib.load_library().uvghip_last_error().decode()}")
        if timed:
            e1.record(stream)
            self.pending.setdefault(slot, []).append((name, e0, e1))

    def harvest(self, slot=None):
        for k in ([slot] if slot is not None else list(self.pending)):
            for name, e0, e1 in self.pending.pop(k, []):
                t = self.ms.setdefault(name, [0.0, 0])
                t[0] += e0.elapsed_time(e1); t[1] += 1
                self.pool += [e0, e1]

    def totals(self):
        self.harvest()
        return {k: (v[0], v[1]) for k, v in self.ms.items()}


def family(name):
    return name.rsplit("_", 1)[0]


def algorithmic_bytes(fr, name, group=1):
    """SURVEY.md 8(d) per-unit figures x the units this launch processes (b = bytes per sample)."""
    kern, n = name.rsplit("_", 1)
    n = int(n)
    if kern in GROUP_KERNELS or (kern.startswith("sao_") and fr.nranks == 1):   # one launch over the group's pictures
        return group * _picture_bytes(fr, kern, n)
    return _picture_bytes(fr, kern, n)


# kernels that take block lists run once per block shape over all pictures of a group (pipeline.FrameGroup)
GROUP_KERNELS = {"rdoq", "dequant", "rdoq_chroma", "dequant_chroma", "tu_forward", "tu_forward_chroma", "tu_inverse", "tu_inverse_chroma",
                 "intra_search", "intra_pred_plane", "intra_pred_chroma", "tu_roundtrip", "tu_roundtrip_chroma"}


def _picture_bytes(fr, kern, n):
    if kern in ("rdoq", "dequant", "rdoq_chroma", "dequant_chroma"):       # int16 in, int16 out
        c = n // 2 if kern.endswith("chroma") else n
        return fr.tables[n][2] * c * c * 4
    if kern in ("tu_forward", "tu_forward_chroma", "tu_inverse", "tu_inverse_chroma"):   # two planes touched + int16 coefficients
        c = n // 2 if kern.endswith("chroma") else n
        return fr.tables[n][2] * c * c * (2 * (1 if fr.depth == 8 else 2) + 2)
    b = 1 if fr.depth == 8 else 2
    rows = fr.band.y1 - fr.band.y0
    W = fr.W
    cnt = fr.tables[n][2] if n else fr.n_ctu
    luma, chroma = W * rows * b, (W // 2) * ((rows + 1) // 2) * b
    if kern == "intra_search":        # refs (4N+1) + original NxN read, best mode + cost written (fused arg-min)
        return cnt * ((4 * n + 1) * b + n * n * b + 5)
    if kern == "intra_pred_plane":    # refs read, NxN written
        return cnt * ((4 * n + 1) * b + n * n * b)
    if kern == "tu_roundtrip":        # orig + pred read, levels (int16) + recon written
        return cnt * n * n * (2 * b + 2 + b)
    if kern == "intra_pred_chroma":
        c = n // 2
        return cnt * ((4 * c + 1) * b + c * c * b)
    if kern == "tu_roundtrip_chroma":
        c = n // 2
        return cnt * c * c * (2 * b + 2 + b)
    if kern in ("deblock_v", "deblock_h"):   # one direction: planes read + written once, 32 B side info per 4x4
        return int(2 * (luma + 2 * chroma) + 32 * W * rows / 16)
    if kern.startswith("sao_stats"):   # orig + rec read, 104 counters per CTU written
        return 2 * (luma if kern.endswith("_y") else chroma) + cnt * 104 * 4
    if kern.startswith("sao_offsets"):
        return (3 if kern.endswith("_yuv") else 1) * cnt * (40 + 8) * 4
    if kern.startswith("sao_apply"):
        return 2 * (luma if kern.endswith("_y") else chroma) + cnt * 32
    if kern == "alf_classify":
        return luma + W * rows // 16
    if kern == "alf_stats":           # orig + rec read; ~12 of 25 classes present per CTU: the records actually written are counted by the caller
        return 2 * luma + fr.alf_records_bytes()
    if kern == "alf_cov_reduce":
        return fr.alf_records_bytes() + 25 * 1509 * 8
    if kern.startswith("alf_filter"):
        return 2 * (luma if kern.endswith("_y") else chroma)
    if kern in ("halo_dbk", "halo_alf", "gather", "allreduce_cov"):
        cb = fr.comm_bytes()
        key = {"halo_dbk": "halo_deblock", "halo_alf": "halo_alf", "gather": "gather", "allreduce_cov": "allreduce_cov"}[kern]
        return sum(cb[key])
    raise KeyError(kern)


def _alf_records_bytes(self):
    if not hasattr(self, "_alf_rb"):
        m = self.alf_present.cpu().numpy().astype(np.int64) & 0xffffffff
        self._alf_rb = int(sum(bin(int(x)).count("1") for x in m)) * 1484 * 8 + 4 * len(m)
    return self._alf_rb


pipeline.BandFrame.alf_records_bytes = _alf_records_bytes


class Slot:
    """One resident GROUP of pictures (pipeline.FrameGroup): the eager head (the searches, which carry the roofline's events)
    and the rest of the plan as hipGraph segments between the exchanges."""

    def __init__(self, L, grp, capture_stream, use_graphs, side_streams=None):
        self.grp = grp
        self.searches = grp.searches()
        frs = grp.frames
        # kernel segments between exchanges: [everything before the filters + vertical deblocking of every picture], then per
        # picture [x_dbk] stage_b [x_alf] stage_c [reduce, gather]; neighbouring kernel segments merge when no exchange separates them
        # the quantiser launches (RDOQ per block shape over the group) stay eager between two graphs: they are
        # the long kernels, and the roofline's HIP events go around them when they are the dominant family
        self.plan = []      # ("kernels", launches) | ("eager", launches) | ("comm", launches)
        if grp.mid:
            self.plan += [("kernels", grp.heads_rest()), ("eager", grp.mid)]
            acc = grp.tails()
        else:
            acc = grp.before_filters()
        if grp.sao:         # whole pictures per rank: no exchange inside the filters, SAO once over the group
            acc, frs = acc + grp.filters(), []
        else:
            acc = acc + [l for fr in frs for l in fr.stage_a]
        for fr in frs:
            for seg, comm in ((fr.xchg_dbk, True), (fr.stage_b, False), (fr.xchg_alf, True), (fr.stage_c, False), (fr.reduce + fr.xchg_gather, True)):
                if comm:
                    if seg:
                        if acc:
                            self.plan.append(("kernels", acc)); acc = []
                        self.plan.append(("comm", seg))
                else:
                    acc = acc + seg
        if acc:
            self.plan.append(("kernels", acc))
        self.graphs = {}
        if use_graphs:
            for i, (kind, ls) in enumerate(self.plan):
                if kind == "kernels":
                    self.graphs[i] = pipeline.Graph(L, ls, capture_stream)
        self.ev_done = torch.cuda.Event()
        self.ev_done.record()

    def issue(self, clock, stream, timed_heads):
        self.ev_done.synchronize()              # at most n_resident groups in flight; this slot's previous use has retired
        clock.harvest(id(self))
        for name, fn, args in self.searches:
            if timed_heads:
                clock.launch(name, fn, args, stream, id(self))
            else:
                pipeline.run([(name, fn, args)], stream.cuda_stream)
        for i, (kind, ls) in enumerate(self.plan):
            if i in self.graphs:
                self.graphs[i].launch(stream.cuda_stream)
            elif kind == "eager" and timed_heads:
                for name, fn, args in ls:
                    clock.launch(name, fn, args, stream, id(self))
            else:
                pipeline.run(ls, stream.cuda_stream)
        self.ev_done.record(stream)

    def issue_profiled(self, clock, stream):
        """Everything eager, every launch bracketed by events (untimed profile pass)."""
        self.ev_done.synchronize()
        clock.harvest(id(self))
        for name, fn, args in self.grp.all_launches():
            clock.launch(name, fn, args, stream, id(self))
        self.ev_done.record(stream)


def cpu_baseline(fr_host_y, fr_host_u, fr_host_v, W, H, DEPTH):
    """The oracle (C restatement, OpenMP over blocks) on the host cores, on a bounded sample: slabs of the top 256 luma
    rows of one frame, repeated until about 10 s of wall time have passed.  Luma chains + deblock (Y,U,V) + luma SAO: the
    chroma predict / TU / SAO launches of the GPU step are NOT in the CPU sample (the CPU figure is the more favourable
    for it)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    orc = Hh.load_oracle()
    rows = 256
    y = np.ascontiguousarray(fr_host_y[:rows])
    modes = np.asarray(MODES, np.int8)
    tables = {n: layout.intra_availability(layout.block_grid(W, rows, n), n, W, rows) for n in SIZES}
    u0, v0 = np.ascontiguousarray(fr_host_u[:rows // 2]), np.ascontiguousarray(fr_host_v[:rows // 2])
    scu = layout.quadtree_scu_table(W, rows, seed=0, qp=QP)
    scu_bytes = np.ascontiguousarray(scu.view(np.uint8).reshape(scu.shape[0], -1))
    rects = np.ascontiguousarray(np.asarray(layout.ctu_rects(W, rows), np.int32).reshape(-1, 4))

    def one_slab():
        for n in SIZES:
            blks = tables[n]
            costs = np.zeros((len(blks), len(modes)), np.uint32)
            orc.fn(DEPTH, "intra_search_frame", None)(Hh.ptr(y), W, Hh.ptr(y), W, W, rows, n, Hh.ptr(blks), len(blks),
                                                      Hh.ptr(modes), len(modes), Hh.ptr(costs))
            best = np.ascontiguousarray(modes[np.argmin(costs, 1)])
            pred = np.zeros_like(y)
            orc.fn(DEPTH, "intra_pred_plane_frame", None)(Hh.ptr(y), W, W, rows, n, Hh.ptr(blks), len(blks),
                                                          Hh.ptr(best), Hh.ptr(pred), W)
            rec = np.zeros_like(y)
            coeff = np.zeros(len(blks) * n * n, np.int16)
            tus = np.ascontiguousarray(blks[:, :2])
            orc.fn(DEPTH, "tu_roundtrip_frame", None)(DEPTH, n, n, QP, 1, Hh.ptr(y), Hh.ptr(pred), Hh.ptr(rec), W,
                                                      Hh.ptr(tus), len(tus), Hh.ptr(coeff))
        ur, vr = u0.copy(), v0.copy()
        orc.deblock_frame(DEPTH, rec, ur, vr, W, rows, scu_bytes, scu.shape[1], 0, 0, False, QP, None)
        edge, band = orc.sao_stats_rects(DEPTH, y, rec, rects)
        params, dd = np.zeros((len(rects), 8), np.int32), np.zeros(len(rects), np.int32)
        orc.lib.orc_sao_edge_offsets(Hh.ptr(edge), None, len(rects), Hh.ptr(params), Hh.ptr(dd))
        out = rec.copy()
        for (fx, fy, w_, h_), p_ in zip(rects, params):
            orc.sao_reconstruct_rect(DEPTH, rec, out, W, rows, int(fx), int(fy), int(w_), int(h_), int(p_[0]), int(p_[1]),
                                     [0, 0], list(p_[3:]) + [0] * 5, False)

    slabs = 0
    t0 = time.perf_counter()
    while slabs < 1 or (time.perf_counter() - t0 < 10.0 and slabs < 64):
        one_slab()
        slabs += 1
    dt = time.perf_counter() - t0
    frames = slabs * rows / H
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count()
    return {"value": round(frames / dt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"{slabs} x the top {rows} of {H} luma rows of a 1080p frame ({frames:.3f} frame): luma search/predict/TU round "
                      f"trip for four block sizes, deblock (Y,U,V), luma SAO statistics/offsets/apply -- the GPU step's chroma "
                      f"predict/TU/SAO launches are not in the CPU sample; oracle C -O2, OpenMP over blocks on {cores} threads "
                      f"except deblocking (serial) ({dt:.1f} s).  This scalar restatement with numpy glue is slower than the real "
                      f"encoder: BASELINE.md has the reference's full 1080p medium encode at 2.2 fps on 8 vCPU (AVX2)"}


def coeff_cost_probe(L, fr, reps=5):
    """CABAC bit cost (uvg_get_coeff_cost's CABAC branch, count-mode coefficient coder: what the RD search prices every
    candidate with) of all the levels one group of pictures produced -- one launch per block shape and plane over the group.
    Reported per picture; not part of the step (the step has no RD mode decision)."""
    import ctypes
    models = lib.CabacModels()
    rng = np.random.default_rng(5)
    for i in range(244):                     # a plausible adapted state: both estimators near the same probability
        p = int(rng.integers(2000, 30000))
        models.state0[i], models.state1[i], models.rate[i] = p & 0x7fe0, p & 0x7ffe, (4 << 4) | 7
    jobs = fr.pool.jobs
    st = torch.cuda.current_stream().cuda_stream
    outs = {k: (torch.empty(j["lev"].shape[0] * j["cnt"], dtype=torch.float64, device=j["lev"].device)) for k, j in jobs.items()}

    def once():
        for (n, color), j in jobs.items():
            F = j["lev"].shape[0]
            lib.check(L.uvghip_coeff_cost_batch(j["lev"].data_ptr(), j["c"], j["c"], F * j["cnt"], color, ctypes.byref(models),
                                                outs[(n, color)].data_ptr(), None, st), "uvghip_coeff_cost_batch")
    once()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        once()
    e1.record()
    torch.cuda.synchronize()
    F = next(iter(jobs.values()))["lev"].shape[0]
    blocks = sum(j["cnt"] for j in jobs.values())
    ms = e0.elapsed_time(e1) / reps / F
    bits = sum(float(o.sum()) for o in outs.values()) / F
    return {"ms_per_picture": round(ms, 4), "blocks_per_picture": blocks, "launches_per_group": len(jobs), "pictures_per_group": F,
            "kbits_per_picture": round(bits / 1e3, 1),
            "note": "uvghip_coeff_cost_batch on the levels RDOQ produced (all block sizes of the step: the same picture is coded four "
                    "times over, once per block size), synthetic adapted context models; one lane per block"}


def ctu_search_traffic(pictures):
    """HBM bytes per launch of the search kernel from the committed PMC passes (profiles/hbm_traffic_latest.json) -- only if they were
    taken on the kernel sources this run uses (a stale capture is not reported)."""
    import hashlib
    t = TRAFFIC.get("ctu_search")
    if not isinstance(t, dict):
        return None
    here = os.path.dirname(os.path.abspath(__file__))
    sha = hashlib.sha1(b"".join(open(os.path.join(here, "uvg266_amd", "csrc", f), "rb").read() for f in ("ctu_core.h", "ctu_leaf4.h", "ctu_search.hip"))).hexdigest()
    return t["bytes_per_picture"] * pictures if t.get("source_sha1") == sha else None


def ctu_search_bytes(W, H, depth):
    """Algorithmic bytes of one picture through uvghip_ctu_search_intra (SURVEY.md 8(d) style, b = bytes per sample): the source read
    once (1.5 W H b), the reconstruction written once (1.5 W H b), the levels written once (1.5 W H x 2), the side information
    (32 B per 4x4) and the three model checkpoints per CTU."""
    b = 1 if depth == 8 else 2
    ctus = ((W + 63) // 64) * ((H + 63) // 64)
    return int(1.5 * W * H * b * 2 + 1.5 * W * H * 2 + (W // 4) * (H // 4) * 32 + ctus * 3 * 257 * 4)


class ClosedLoop:
    """One group of `in_flight` pictures on its own stream: one uvghip_loop_plan_run per issue = the closed-loop CTU search
    (uvghip_ctu_plan_run), the in-loop filters on the reference's schedule (encoderstate.c:841-853 per CTU, the frame's
    uvg_sao_reconstruct afterwards: snapshot deblocking -> SAO statistics -> the SAO decision of every CTU -> deblocking -> SAO
    apply) and the arithmetic coder (uvghip_encode_slice_rows: every WPP row's substream), strung together in C
    (csrc/loop_plan.hip); outputs: the picture the encoder returns and the slice data of its .266, bit for bit
    (tests/test_gpu_sao_decide.py, tests/test_gpu_slice_coder.py)."""

    def __init__(self, wl, first_t, in_flight, device, step=1):
        from concurrent.futures import ThreadPoolExecutor
        self.W, self.H, self.depth = wl["W"], wl["H"], wl["depth"]
        self.P = api.ctu_params(self.W, self.H, QP)
        self.ts = [first_t + k * step for k in range(in_flight)]
        # a 1080p picture is ~0.1 s of numpy on one core and a group has hundreds: made side by side (numpy's array work releases
        # the GIL; every picture has its own seeded generator, so the pictures are the same as one after the other)
        with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
            self.host = list(ex.map(lambda t: layout.synthetic_yuv420(self.W, self.H, t, self.depth), self.ts))
        src = [tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in yuv) for yuv in self.host]
        self.cs = api.ClosedLoop(self.P, src)
        self.stream = torch.cuda.Stream(device=device)
        self.ev = []                    # (start, end) of every timed search launch, on this group's stream
        self.done = torch.cuda.Event()

    def issue(self, timed=True):
        with torch.cuda.stream(self.stream):
            if timed:               # the plan's two halves with HIP events around the search kernel's launch, on its own stream
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.cs.run_search()
                e1.record()
                self.cs.run_filters()
                self.ev.append((e0, e1))
            else:
                self.cs.run()
            self.done.record()

    def search_ms(self):
        return sum(a.elapsed_time(b) for a, b in self.ev), len(self.ev)


DUMP_BUDGET = 64_000_000            # bytes of .npy data that --dump-outputs may write


def dump_outputs(group, out_dir):
    """What the last timed step handed its caller -- the output pictures (after deblocking + SAO) and the slice data of every WPP row --
    as out_dir/<name>.npy.  All of it would be gigabytes in float32, so: row_bytes of every picture of the step, and the whole output
    pictures and slice data of a seeded sample of them (as many as fit in 40 MB, at least one; picture_t = their numbers in the synthetic
    sequence).  The sample depends on the arguments only, so two builds of the project can be compared output for output."""
    cs, n = group.cs, group.cs.n
    per_picture = sum(p.numel() for p in cs.out[0]) * 4
    k = max(1, min(n, int(40e6 // per_picture)))
    pick = np.sort(np.random.default_rng(0).choice(n, size=k, replace=False))
    torch.cuda.synchronize()
    rows, nbytes = cs.slice_data()
    nb = nbytes.cpu().numpy()
    arrays = {"picture_t": np.array([group.ts[i] for i in pick], np.float64), "row_bytes": nb.astype(np.float64)}
    for c, name in enumerate(("final_y", "final_u", "final_v")):
        arrays[name] = np.stack([cs.out[i][c].cpu().numpy() for i in pick]).astype(np.float32)
    data = []
    for i in pick:                  # picture after picture, each one's rows in order (row_bytes splits them)
        r = rows[i].cpu().numpy()
        data += [r[j, :nb[i, j]] for j in range(nb.shape[1])]
    arrays["slice_data"] = np.concatenate(data).astype(np.float32)
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_BUDGET:
        raise SystemExit(f"--dump-outputs: {total} bytes exceed the {DUMP_BUDGET}-byte budget")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def alf_stage_timing(group, reps=2):
    """The ALF stage of BASELINE configs[3] (--alf full) behind a group of the 2160p 10-bit closed loop: api.ClosedLoop.alf_stage over the
    group's pictures -- per picture the frame statistics the reference's derivation reads (classification; the luma covariance per class
    summed over the CTUs; the chroma and CC-ALF covariances per CTU), then the decisions, uvghip_alf_reconstruct_picture and, for the group,
    the slice data with the ALF syntax.  The DERIVATION is not timed: `decide` returns the decisions the reference encoder made for picture 0
    of this workload (tests/golden/ref_stream_3840x2160_10_qp22_1frames_alf_crc.npz) for every picture -- the host work SURVEY.md keeps on
    the host.  Picture 0's output goes through the library's NAL writer and is compared with the encoder's --alf full .266 (length + CRC
    of everything behind the parameter sets).  -> None without the golden."""
    import zlib
    path = os.path.join(ROOT, "tests", "golden", "ref_stream_3840x2160_10_qp22_1frames_alf_crc.npz")
    if not os.path.exists(path):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_alf_syntax import write_alf_picture_nals
    g = np.load(path)
    cs = group.cs
    assert [int(a) for a in g["meta"]] == [group.W, group.H, group.depth, QP]
    pic = {k[4:]: g[k][0] for k in ("alf_meta", "alf_flags", "alf_set_idx", "alf_luma_aps", "alf_chroma_aps", "alf_cc_coeff")}
    m = pic["meta"]
    scratch = {}

    def decide(i, stats):
        stats.luma_frame(scratch); stats.chroma(1); stats.chroma(2); stats.cc(1); stats.cc(2)
        return dict(alf_type=int(m[3]), enabled=[int(a) for a in m[4:7]], n_luma_aps=int(m[7]), luma_aps=pic["luma_aps"], chroma_aps=pic["chroma_aps"],
                    cc_enabled=[int(a) for a in m[17:19]], cc_filter_count=[int(a) for a in m[19:21]], cc_coeff=pic["cc_coeff"], ctu_flags=pic["flags"], filter_set_idx=pic["set_idx"])
    best = None
    for k in range(reps + 1):                 # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alf_out, rows, nbytes = cs.alf_stage(decide, source=cs.src, classification_shift=int(m[28]) + 4)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if k and (best is None or dt < best) else best
    nb = np.ascontiguousarray(nbytes[0].cpu().numpy(), np.int32)
    r = np.ascontiguousarray(rows[0, :, :int(nb.max())].cpu().numpy())
    sums = api.picture_checksum(*alf_out[0]).cpu().numpy().view(np.uint32)
    nals = write_alf_picture_nals(cs.L, dict(alf_meta=m, aps_meta=g["aps_meta"], aps_luma=g["aps_luma"], aps_chroma=g["aps_chroma"], aps_cc=g["aps_cc"]), r, nb, sums)
    if len(nals) != int(g["bitstream_tail_len"]) or zlib.crc32(nals) != int(g["bitstream_tail_crc"]):
        return {"ms_per_group": round(1e3 * best, 1), "pictures": cs.n, "parity_checked": False,
                "error": "picture 0 behind the ALF stage is NOT the reference encoder's --alf full picture"}
    return {"ms_per_group": round(1e3 * best, 1), "pictures": cs.n, "parity_checked": True,
            "parity": "picture 0: APS NAL units + slice (ALF syntax) + hash SEI of the picture ALF leaves == the reference encoder's --alf full .266 behind its parameter sets (length + CRC)",
            "note": "statistics (classification, frame luma covariance, chroma and CC-ALF covariances) + reconstruction + the coder with the ALF syntax, run AFTER the loop's own pass; the "
                    "derivation of the decisions (alf_encoder / alf_encoder_ctb / derive_cc_alf_filter) stays on the host behind the callback and is NOT timed -- picture 0's recorded "
                    "decisions are replayed for every picture"}


def c2_clip(wl, device, frames=60, reps=2):
    """What BASELINE configs[1] itself would see: its 60-picture clip from HOST memory to the `.266` bytes of its pictures in HOST memory,
    wall clock -- upload of the source planes (pageable host memory, the default stream), one uvghip_loop_plan_run over the 60 pictures
    (search -> filters -> slice data), then uvghip_loop_plan_group_nals: the checksums of the output pictures, ONE download of the group's rows
    and the NAL assembly (slice NAL + hash SEI per picture).  60 pictures put ~660 CTUs in flight, below the device's 1024
    workgroup slots, and nothing overlaps the fill and drain of the single launch: this is the latency of ONE clip, the judged `value`
    is the throughput of many.  The plan and its buffers exist before the clock starts (an encoder keeps them).  Not part of `value`."""
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    P = api.ctu_params(W, H, QP)
    host = [tuple(np.ascontiguousarray(p) for p in layout.synthetic_yuv420(W, H, t, depth)) for t in range(frames)]
    src = [tuple(torch.empty(p.shape, dtype=torch.uint8 if depth == 8 else torch.uint16, device=device) for p in yuv) for yuv in host]
    cs = api.ClosedLoop(P, src)
    best, nbytes = None, 0
    for _ in range(reps + 1):                     # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for yuv, dst in zip(host, src):
            for p, d in zip(yuv, dst):
                d.copy_(torch.from_numpy(p), non_blocking=True)
        cs.run()
        out = cs.group_nals(0)
        dt = time.perf_counter() - t0
        nbytes = sum(len(b) for b in out)
        best = dt if best is None or dt < best else best
    # one picture alone: the three launches one after the other / beside each other (uvghip_loop_plan_run_overlapped)
    one = {}
    c1 = api.ClosedLoop(P, src[:1])
    for name, fn in (("run", c1.run), ("run_overlapped", c1.run_overlapped)):
        fn(); c1.group_nals(0)
        b1 = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            c1.group_nals(0)
            dt = time.perf_counter() - t0
            b1 = dt if b1 is None or dt < b1 else b1
        one[name] = round(1e3 * b1, 1)
    del c1
    return {"value": round(frames / best, 2), "unit": "frames/s (one 60-picture clip, host memory to .266 bytes in host memory)", "frames": frames, "one_picture_ms": one,
            "wall_ms": round(1e3 * best, 1), "bytes_out": int(nbytes), "upload_mb": round(frames * W * H * 1.5 * (1 if depth == 8 else 2) / 1e6, 1),
            "note": "one launch of 60 pictures: the wavefronts' fill and drain are not hidden by a second launch, 660 of 1024 workgroup slots busy at best; "
                    "the NAL units of the group come over in one download (uvghip_loop_plan_group_nals)"}


def tiles_clip(wl, device, frames=60, grid=(6, 4), with_cpu=True):
    """BASELINE configs[1]'s 60-picture clip under --tiles <grid> --wpp (uvghip_tiles_plan_*: csrc/tiles.hip), host memory to `.266` bytes in
    host memory like c2_clip, and ONE picture alone with and without tiles.  Tiles are the reference's independent rectangles (no neighbour in
    the search, no sample in the filters, own context models): the stream is the one the reference writes with the same --tiles, not c2_clip's
    -- the first two pictures' NAL units are held to its run (tests/golden/ref_tiles_1920x1080_8_qp22_6x4_2frames_crc.npz) inside this
    line.  What tiles buy is latency: a 1080p picture is 62 WPP diagonals, in 6 x 4 tiles 24 wavefronts of 13 side by side."""
    import zlib
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    P = api.ctu_params(W, H, QP)
    host = [tuple(np.ascontiguousarray(p) for p in layout.synthetic_yuv420(W, H, t, depth)) for t in range(frames)]
    src = [tuple(torch.empty(p.shape, dtype=torch.uint8 if depth == 8 else torch.uint16, device=device) for p in yuv) for yuv in host]
    tl = api.TiledLoop(P, src, grid)
    best, out = None, None
    for _ in range(3):                            # the first pass is the warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for yuv, dst in zip(host, src):
            for p, d in zip(yuv, dst):
                d.copy_(torch.from_numpy(p), non_blocking=True)
        tl.run()
        out = tl.nals(0)
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    res = {"value": round(frames / best, 2), "unit": f"frames/s (one 60-picture clip under --tiles {grid[0]}x{grid[1]} --wpp, host memory to .266 bytes in host memory)",
           "frames": frames, "wall_ms": round(1e3 * best, 1), "bytes_out": int(sum(len(b) for b in out)), "tiles": f"{grid[0]}x{grid[1]}", "size_classes": tl.n_classes,
           "substreams_per_picture": tl.n_substreams, "parity_checked": False}
    name = f"ref_tiles_{W}x{H}_{depth}_qp{QP}_{grid[0]}x{grid[1]}_2frames_crc"
    g = None
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if os.path.exists(path):
        g = np.load(path)
        two = out[0] + out[1]
        ok = len(two) == int(g["bitstream_tail_len"]) and zlib.crc32(two) == int(g["bitstream_tail_crc"])
        finals = [zlib.crc32(np.concatenate([p.cpu().numpy().reshape(-1) for p in tl.out[i]]).tobytes()) == int(g["final_crc"][i]) for i in range(2)]
        res["parity_checked"] = bool(ok and all(finals))
        res["parity"] = {"golden": name, "items": "slice NAL + hash SEI of pictures 0 and 1 (length + CRC-32) and the CRC-32 of their output pictures vs the reference encoder's run "
                                                  "with the same --tiles"}
    del tl
    # one picture alone: the latency tiles are for
    one = {}
    for gr in ((1, 1), grid):
        t1 = api.TiledLoop(P, src[:1], gr)
        t1.run(); t1.nals(0)
        b1 = None
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t1.run()
            t1.nals(0)
            dt = time.perf_counter() - t0
            b1 = dt if b1 is None or dt < b1 else b1
        one["no_tiles" if gr == (1, 1) else f"tiles_{gr[0]}x{gr[1]}"] = round(1e3 * b1, 1)
        del t1
    res["one_picture_ms"] = one
    res["note"] = ("the reference's tiles: independent rectangles, so the bytes differ from c2_clip's stream (the reference's with the same --tiles); one loop plan per tile size "
                   "on its own stream, the tiles of a picture side by side on the device")
    if with_cpu:
        res["cpu_baseline"] = cpu_baseline_reference(wl, frames=frames, extra=("--tiles", f"{grid[0]}x{grid[1]}", "--wpp"))
    return res


def c4_clip(device, frames=60, with_cpu=True):
    """The 60-picture 3840x2160 10-bit clip of BASELINE configs[3]'s geometry, all-intra (-p 1 --preset medium at the bench's QP; the P / B
    + ALF combination of configs[3] as written is not built: DESIGN.md section 7), host memory to `.266` bytes in host memory as c2_clip:
    once as ONE uvghip_loop_plan_run over the 60 pictures, once as TWO plans of 30 on two streams (the second launch's thin first
    diagonals overlap the first one's drain).  The reference encoder's CLI (oracle/_ref/uvg266_10, host cores) on the same clip beside it."""
    wl = WORKLOADS["2160p10alf"]
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    P = api.ctu_params(W, H, QP)
    host = [tuple(torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in layout.synthetic_yuv420(W, H, t, depth)) for t in range(frames)]
    src = [tuple(torch.empty_like(p, device=device) for p in yuv) for yuv in host]
    res = {}
    for n_groups in (1, 2):
        per = frames // n_groups
        loops = [api.ClosedLoop(P, src[g * per:(g + 1) * per]) for g in range(n_groups)]
        streams = [torch.cuda.Stream() for _ in range(n_groups)]
        best, nbytes = None, 0
        for _ in range(2):                        # the first pass is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for g, (cs, st) in enumerate(zip(loops, streams)):
                with torch.cuda.stream(st):
                    for yuv, dst in zip(host[g * per:(g + 1) * per], src[g * per:(g + 1) * per]):
                        for p, d in zip(yuv, dst):
                            d.copy_(p, non_blocking=True)
                    cs.run(st.cuda_stream)
            out = []
            for g, (cs, st) in enumerate(zip(loops, streams)):
                with torch.cuda.stream(st):
                    out += cs.group_nals(g * per)
            dt = time.perf_counter() - t0
            nbytes = sum(len(b) for b in out)
            best = dt if best is None or dt < best else best
        res[f"{n_groups}_launch" + ("es" if n_groups > 1 else "")] = {"value": round(frames / best, 2), "wall_ms": round(1e3 * best, 1), "bytes_out": int(nbytes)}
        del loops
    out = {"value": max(v["value"] for v in res.values()), "unit": "frames/s (one 60-picture 2160p 10-bit all-intra clip, host memory to .266 bytes in host memory)",
           "frames": frames, "variants": res, "upload_mb": round(frames * W * H * 1.5 * 2 / 1e6, 1),
           "workload": f"{W}x{H} {depth}-bit yuv420p, -p 1 --preset medium at QP {QP}, {frames} pictures: upload -> closed-loop CTU search -> deblocking -> SAO -> arithmetic coder -> "
                       "per picture checksum, row download, NAL assembly",
           "note": "the latency of ONE clip: a 2160p picture has 93 diagonals of at most 34 CTUs, 60 pictures keep the 1024 workgroup slots busy only in the middle of the launch"}
    if with_cpu:
        out["cpu_baseline"] = cpu_baseline_reference(wl, frames=16)          # a bounded sample: the first 16 pictures of the clip (~15 s at ~1.1 frames/s; all 60 took 54 s of the run)
    return out


def parity_check(group, golden):
    """Picture 0 of a group AFTER the timed region -- the buffers hold what its last timed pass wrote, with the other group's launch
    sharing the device -- against the record of the real encoder's run on the same picture (tests/golden/<golden>.npz, data only):
    per-CTU CRCs of side information + trees / reconstruction / levels / the models after the coder, the SAO decisions and models,
    per-CTU CRCs of the output picture, every WPP row's substream (length and CRC).  Raises on any difference."""
    import zlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    g = Hh.ctu_golden(golden)
    W, H, depth, qp, t = (int(a) for a in g["meta"][:5])
    cs = group.cs
    assert (W, H, depth, qp) == (group.W, group.H, group.depth, QP), "golden and workload disagree"
    y, u, v = group.host[0]
    if zlib.crc32(y.tobytes() + u.tobytes() + v.tobytes()) != int(g["src_crc"]):
        raise SystemExit(f"parity check: picture 0 of the group is not the golden's source picture ({golden})")
    torch.cuda.synchronize()
    ry, ru, rv = (x.cpu().numpy() for x in cs.out[0])
    # the reconstruction before the filters was deblocked in place by the loop plan: what remains comparable of the search are the
    # side information, the levels and the models; the pictures are compared after the filters
    scu = cs.cu[0].cpu().numpy().reshape(-1).view(Hh.SCU_NP)
    res = Hh.search_result_from_device_layout(W, H, ry, ru, rv, scu, cs.coeff[0].cpu().numpy(), cs.models[0].cpu().numpy().view(np.uint32))
    crc = Hh.ctu_crcs(res, W, H)
    bad = {}
    for col, what in ((0, "cu+trees"), (2, "levels"), (3, "models")):
        n = int((crc[:, col] != g["crc"][:, col]).sum())
        if n:
            bad[what] = n
    info, models = cs.results()
    if not np.array_equal(Hh.sao_info_comparable(info[0]), Hh.sao_info_comparable(g["sao"])):
        bad["sao"] = 1
    if not np.array_equal(models[0], g["sao_models"]):
        bad["sao_models"] = 1
    fin = Hh.filter_crcs(dict(snap_y=ry, snap_u=ru, snap_v=rv, final_y=ry, final_u=ru, final_v=rv), W, H)[:, 1]
    n = int((fin != g["filter_crc"][:, 1]).sum())
    if n:
        bad["output picture"] = n
    rows, nbytes = cs.slice_data()
    nb = nbytes[0].cpu().numpy()
    if not np.array_equal(np.concatenate([[0], np.cumsum(nb)]), g["row_off"]):
        bad["row lengths"] = 1
    else:
        rc = np.array([zlib.crc32(rows[0, r, :nb[r]].cpu().numpy().tobytes()) for r in range(len(nb))], np.uint32)
        n = int((rc != g["row_crc"]).sum())
        if n:
            bad["slice data rows"] = n
    if bad:
        raise SystemExit(f"parity check FAILED against {golden}: {bad}")
    return {"golden": golden, "ctus": int(len(crc)), "rows": int(len(nb)),
            "items": "per-CTU CRC of cu fields + trees, levels, models after the coder; SAO decisions + models; per-CTU CRC of the output picture; "
                     "every WPP row's slice data (length + CRC) -- picture 0 of group 0 after the timed region vs the reference encoder's record"}


def inter_hot_path(device, reps=5):
    """BASELINE.json configs[2] (1920x1080 8-bit, --gop lp-g4d3t1 --preset medium): the inter search's hot path on the device, OPEN LOOP --
    for every prediction unit of every size (64, 32, 16, 8: 510 + 2040 + 8100 + 32400 units) and each of two reference pictures the whole
    motion search of search_pu_inter_ref + search_frac (uvghip_me_search_batch: starting point, early termination, hexagon search on SAD,
    four fractional steps on SATD), then the bi-prediction of the two results against the source (uvghip_inter_pred_satd_batch: two
    interpolations, average, SATD).  Open loop: the references are source pictures, the AMVP predictors zero, no merge candidates -- the
    closed loop (search_cu's inter / intra competition on reconstructed references) is the oracle's so far.  Not part of `value`."""
    W, H, depth = 1920, 1080, 8
    cur = torch.from_numpy(np.ascontiguousarray(layout.synthetic_yuv420(W, H, 4, depth)[0])).to(device)
    refs = [torch.from_numpy(np.ascontiguousarray(layout.synthetic_yuv420(W, H, t, depth)[0])).to(device) for t in (3, 2)]
    tab = api.ref_table(refs)
    lam_sqrt = float(np.sqrt(0.57 * 2.0 ** ((QP + 5 - 12) / 3.0)))
    jobs, bi, n_units = {}, {}, 0
    for size in (64, 32, 16, 8):
        xs, ys = np.arange(0, W - size + 1, size), np.arange(0, H - size + 1, size)
        gx, gy = np.meshgrid(xs, ys)
        n = gx.size
        j = np.zeros(2 * n, api.ME_JOB_NP)
        j["x"], j["y"] = np.tile(gx.ravel(), 2), np.tile(gy.ravel(), 2)
        j["ref"] = np.repeat([0, 1], n)
        jobs[size] = torch.from_numpy(j.view(np.uint8)).to(device)
        m = np.zeros(n, api.MOTION_NP)
        m["x"], m["y"], m["dir"], m["ref"] = gx.ravel(), gy.ravel(), 3, [0, 1]
        bi[size] = m
        n_units += n
    st = torch.cuda.current_stream()

    def one(timed=None):
        res = {}
        for size in (64, 32, 16, 8):
            if timed is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            res[size] = api.me_search_batch(cur, refs, tab, jobs[size], size, lam_sqrt, 4)
            if timed is not None:
                e1.record()
                timed.setdefault(size, []).append((e0, e1))
        return res
    res = one()
    torch.cuda.synchronize()
    # the bi-prediction candidates from the first pass's vectors (fixed for the timed passes)
    cands = {}
    for size in (64, 32, 16, 8):
        r = res[size].cpu().numpy().view(api.ME_RESULT_NP)
        n = len(r) // 2
        m = bi[size]
        m["mv"][:, 0], m["mv"][:, 1] = r["mv"][:n], r["mv"][n:]
        cands[size] = torch.from_numpy(m.view(np.uint8)).to(device)
    frac = float(np.mean([((res[s].cpu().numpy().view(api.ME_RESULT_NP)["mv"] & 15) != 0).any(axis=1).mean() for s in (64, 32, 16, 8)]))
    ev = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        one(ev)
        for size in (64, 32, 16, 8):
            api.inter_pred_satd_batch(cur, refs, tab, cands[size], size)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    per_size = {str(s): round(sum(a.elapsed_time(b) for a, b in ev[s]) / len(ev[s]), 3) for s in ev}
    b = 1
    alg = 2 * 2 * W * H * b                                  # ME of one size against R references reads (1 + 1) W H b per reference ideally
    me_ms = sum(per_size.values())
    return {"value": round(1.0 / dt, 2), "unit": "pictures/s (open loop)", "ms_per_picture": round(1e3 * dt, 3), "prediction_units": n_units, "references": 2,
            "me_search_ms_by_size": per_size, "units_per_s": round(2 * n_units / (me_ms * 1e-3)),
            "roofline": {"bound": "hbm", "kernel": "me_search_kernel", "achieved": round(4 * alg / (me_ms * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(4 * alg / (me_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "traffic": None,
                         "note": "algorithmic bytes: (source + reference) once per size and reference = 4 sizes x 2 references x 2 W H; the search is a chain of "
                                 "dependent steps per unit (one wave each), latency-bound on the small units"},
            "fractional_vectors": round(frac, 3),
            "workload": "1920x1080 8-bit, configs[2] geometry: motion search (hexagon + 4 fractional steps) of every 8..64 unit against 2 reference pictures + "
                        "bi-prediction SATD of the two results; open loop (source pictures as references, zero predictors)"}


def low_delay_closed_loop(device, n_seq=8, reps=2):
    """BASELINE.json configs[2] (1920x1080 8-bit, --gop lp-g4d3t1 --preset medium, QP 27): n_seq independent sequences of 5 pictures
    (I B B B B, up to four reference pictures) through the CLOSED loop on the device, picture group after picture group
    (api.LowDelayLoop): the I pictures through uvghip_loop_plan_run, every B picture group through uvghip_loop_pb_run -- the CTU search
    with the inter search inside (uvghip_ctu_search_pb: merge / AMVP candidates, hexagon + fractional motion search, bi-prediction, early
    skip, inter / intra competition, 64x64 CUs, history table) on the device's OWN earlier output pictures, deblocking with boundary
    strengths from the stored motion, SAO with the slice type's models, the arithmetic coder.  Parity: before the timed passes the output
    picture and every WPP row's slice data of every picture of sequence 0 and of the last sequence are compared (CRC) with the reference
    encoder's own run on the same source (tests/golden/ref_intercrc_1920x1080_8_qp27_5frames.npz).  Not part of `value`."""
    import zlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    golden = "ref_intercrc_1920x1080_8_qp27_5frames"
    g = np.load(os.path.join(ROOT, "tests", "golden", golden + ".npz"))
    W, H, depth, qp0, frames = (int(a) for a in g["dims"])
    hc = (H + 63) // 64
    states = Hh.frame_states_from_records(g["meta"], g["lam"], g["refs"])
    pics = [Hh.moving_picture(W, H, t, depth) for t in range(frames)]
    for t in range(frames):
        if zlib.crc32(b"".join(p.tobytes() for p in pics[t])) != int(g["src_crc"][t]):
            raise SystemExit("c3 parity check: the sequence generator drifted from the golden's source")
    one = [tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in pics[f]) for f in range(frames)]
    src = [one for _ in range(n_seq)]                     # (the sequences read the same source planes; every other buffer is their own)
    loop = api.LowDelayLoop(W, H, depth, n_seq, states, src)
    loop.run()
    torch.cuda.synchronize()
    bad = {}
    for f in range(frames):
        rows, nb = loop.rows[f].cpu().numpy(), loop.row_bytes[f].cpu().numpy()
        for s in sorted({0, n_seq - 1}):
            planes = [a.cpu().numpy() for a in loop.out[f][s]]
            if zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in planes)) != int(g["final_crc"][f]):
                bad[f"picture {f} sequence {s}"] = "output picture"
            for r in range(hc):
                if nb[s, r] != int(g["row_len"][f * hc + r]) or zlib.crc32(rows[s, r, :nb[s, r]].tobytes()) != int(g["row_crc"][f * hc + r]):
                    bad[f"picture {f} sequence {s} row {r}"] = "slice data"
    if bad:
        raise SystemExit(f"c3 parity check FAILED against {golden}: {dict(list(bad.items())[:6])}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loop.run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    n_pic = n_seq * frames
    return {"value": round(n_pic / dt, 2), "unit": "frames/s (closed loop, low delay)", "ms_per_sequence_group": round(1e3 * dt, 1), "sequences": n_seq, "pictures_per_sequence": frames,
            "mpixels_per_s": round(n_pic / dt * W * H / 1e6, 2), "parity_checked": True,
            "parity": {"golden": golden, "pictures": frames, "sequences_checked": sorted({0, n_seq - 1}),
                       "items": "CRC of every output picture (after deblocking + SAO) and length + CRC of every WPP row's slice data vs the reference encoder's run"},
            "workload": f"{W}x{H} {depth}-bit yuv420p, --gop lp-g4d3t1 --preset medium at QP {qp0} (BASELINE.json configs[2]): {n_seq} sequences x {frames} pictures (I B B B B), "
                        "per picture group one call: closed-loop CTU search with the inter search (device references) -> deblocking -> SAO -> arithmetic coder",
            "note": "one wave per CTU walks the CTU in the reference's own order; the pictures of a sequence are a dependency chain, parallelism comes from the "
                    "sequences and the 2-CTU-lag wavefront inside a picture (DESIGN.md 4.12)"}


def c3_clip(device, frames=120, with_cpu=True):
    """BASELINE.json configs[2] as BASELINE defines it: ONE 1920x1080 8-bit clip of 120 pictures, --gop lp-g4d3t1 --preset medium at QP 27
    (intra period 64: I pictures at 0 and 64), host memory to slice data: the sources are uploaded inside the timed region, ALL
    pictures go through ONE uvghip_loop_pb_run_inflight_ext (the two I pictures searched by the all-intra kernel on a second stream and
    filtered inside the in-flight launch) -- the encoder's --owf schedule
    (encoderstate.c:1060-1116): CTU (x, y) of a picture starts when CTU (x + 2, y + 1) of the pictures it reads is final, deblocking and
    SAO run per CTU inside the persistent search kernel, the vectors keep to what is final in a reference still being coded
    (inflight_margin 11 = cfg.owf != 0).  Every picture and every WPP row's bytes are compared with the reference encoder's --owf 1 run of
    this clip (tests/golden/ref_intercrc_1920x1080_8_qp27_120frames_owf1.npz, which also holds the frame-level state: slice types, QPs,
    lambdas, reference lists).  The reference encoder's CLI on the host cores runs the same clip beside it (cpu_baseline)."""
    import zlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    golden = "ref_intercrc_1920x1080_8_qp27_120frames_owf1"
    g = np.load(os.path.join(ROOT, "tests", "golden", golden + ".npz"))
    W, H, depth, qp, total = (int(a) for a in g["dims"])
    frames = min(frames, total)
    hc = (H + 63) // 64
    states = Hh.frame_states_from_records(g["meta"], g["lam"], g["refs"])[:frames]
    host = [[torch.from_numpy(np.ascontiguousarray(p)).pin_memory() for p in Hh.clip_picture(W, H, t, depth)] for t in range(frames)]
    src = [[tuple(torch.empty_like(p, device=device) for p in host[t]) for t in range(frames)]]
    loop = api.LowDelayLoop(W, H, depth, 1, states, src, inflight=True, inflight_margin=11, intra_in_flight=True)

    def run():
        for t in range(frames):
            for d, h in zip(src[0][t], host[t]):
                d.copy_(h, non_blocking=True)
        loop.run()
    run()                                                 # warm-up (plans, first-touch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = int(sum(int(loop.row_bytes[f].sum().item()) for f in range(frames)))
    bad = []
    for f in range(frames):
        planes = [a.cpu().numpy() for a in loop.out[f][0]]
        if zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in planes)) != int(g["final_crc"][f]):
            bad.append(f"picture {f}")
        rows, nb = loop.rows[f].cpu().numpy(), loop.row_bytes[f].cpu().numpy()
        for r in range(hc):
            if int(nb[0, r]) != int(g["row_len"][f * hc + r]) or zlib.crc32(rows[0, r, :nb[0, r]].tobytes()) != int(g["row_crc"][f * hc + r]):
                bad.append(f"picture {f} row {r}")
    n_pb = sum(1 for fs in states if fs["slice_type"] != 2)
    out = {"value": round(frames / dt, 3), "unit": "frames/s (one low-delay clip, host memory -> slice data, pictures in flight on the encoder's --owf schedule)",
           "frames_timed": frames, "clip_frames": total, "wall_ms": round(1e3 * dt, 1), "slice_data_bytes": nbytes, "parity_checked": not bad,
           "parity": {"golden": golden, "pictures": frames, "mismatches": bad[:8],
                      "items": "CRC of every output picture (after deblocking + SAO) and length + CRC of every WPP row's slice data vs the reference encoder's --owf 1 run of this clip"},
           "launches": {"inflight_calls": 1, "pictures_in_the_inflight_call": frames, "of_them_searched_by_the_all_intra_kernel_beside_it": frames - n_pb},
           "workload": f"{W}x{H} {depth}-bit yuv420p, ONE clip of {frames} pictures, --gop lp-g4d3t1 --preset medium --owf 1 at QP {qp} (BASELINE.json configs[2]); upload -> every "
                       "picture in ONE persistent launch: closed-loop CTU search with the inter search on the device's own reference pictures while they are still being coded "
                       "(four waves per CTU; the I pictures' search by the all-intra kernel on a second stream), per-CTU deblocking + SAO, cross-picture CTU flags -> the arithmetic coder",
           "note": "a picture follows its reference four wavefront diagonals behind (cx + 2 cy; one flag per reference, final_done(x + 1, y + 1), covers what a restricted vector "
                   "can reach): a chain of dependent pictures costs four CTU times per picture instead of a picture's 62 diagonals; the two intra periods of the clip are "
                   "independent and run side by side"}
    del loop
    if with_cpu:
        out["cpu_baseline"] = cpu_baseline_low_delay(W, H, depth, qp, total)
    return out


def ra_clip(device, frames=65, with_cpu=True):
    """ONE 1920x1080 8-bit clip with --preset medium's own GOP (random access, --gop 16: hierarchical B pictures, references in the future;
    what BASELINE.json configs[3] / [4] run with): pictures in CODING order through api.LowDelayLoop(inflight=True, intra_in_flight=True): the whole clip is ONE
    uvghip_loop_pb_run_inflight_ext, a CTU starts when the CTUs a restricted vector can reach in its reference pictures are final
    (DESIGN.md 4.15), the I pictures searched by the all-intra kernel beside it.  Frame-level state (slice types, the hierarchical QPs / lambdas, reference lists, coding order) from
    tests/golden/ref_gop16_states_qp27_65frames.npz (the reference encoder's own, independent of the picture size); the coded pictures
    are compared with the reference encoder's run of this clip (tests/golden/ref_intercrc_1920x1080_8_qp27_65frames_ra16.npz: all 65,
    incl. the I picture of the second intra period at POC 64 and the pictures before it in display order that are coded after it)."""
    import zlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_gop16_states_qp27_65frames.npz"))
    W, H, depth, qp = 1920, 1080, 8, int(g["dims"][0])
    total = int(g["dims"][1])
    frames = min(frames, total)
    states = Hh.frame_states_from_records(g["meta"], g["lam"], g["refs"])[:frames]
    display = [int(a) for a in g["display"][:frames]]
    shown = {t: tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in Hh.clip_picture(W, H, t, depth)) for t in sorted(set(display))}
    src = [[shown[display[f]] for f in range(frames)]]
    loop = api.LowDelayLoop(W, H, depth, 1, states, src, inflight=True, inflight_margin=11, intra_in_flight=True)
    loop.run()                                            # warm-up (plans, first-touch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nbytes = int(sum(int(loop.row_bytes[f].sum().item()) for f in range(frames)))
    # parity: every coded picture the golden holds against the reference encoder's record of the same clip
    golden = "ref_intercrc_1920x1080_8_qp27_65frames_ra16"          # (every picture of the clip incl. the second intra period; the 17-picture golden where it is absent)
    if not os.path.exists(os.path.join(ROOT, "tests", "golden", golden + ".npz")):
        golden = "ref_intercrc_1920x1080_8_qp27_17frames_ra16"
    ref = np.load(os.path.join(ROOT, "tests", "golden", golden + ".npz"))
    n_chk, hc = min(frames, int(ref["dims"][4])), (H + 63) // 64
    ok = [int(a) for a in ref["display"][:n_chk]] == display[:n_chk]
    for f in range(n_chk):
        planes = [a.cpu().numpy() for a in loop.out[f][0]]
        ok = ok and zlib.crc32(b"".join(np.ascontiguousarray(a).tobytes() for a in planes)) == int(ref["final_crc"][f])
        rows, nb = loop.rows[f].cpu().numpy(), loop.row_bytes[f].cpu().numpy()
        for r in range(hc):
            ok = ok and int(nb[0, r]) == int(ref["row_len"][f * hc + r]) and zlib.crc32(rows[0, r, :nb[0, r]].tobytes()) == int(ref["row_crc"][f * hc + r])
    out = {"value": round(frames / dt, 3), "unit": "frames/s (one random-access clip, pictures in flight along the reference DAG)", "frames_timed": frames, "wall_ms": round(1e3 * dt, 1),
           "slice_data_bytes": nbytes, "dependency_levels": 1 + max(loop.level), "launches": len(loop.order), "parity_checked": bool(ok),
           "parity": {"golden": golden, "pictures": n_chk,
                      "items": "CRC of every output picture (after deblocking + SAO) and length + CRC of every WPP row's slice data vs the reference encoder's run of this clip"},
           "workload": f"{W}x{H} {depth}-bit yuv420p, ONE clip, --preset medium as it stands (--gop 16: coding order 0 16 8 4 2 1 3 6 5 7 12 ..., five temporal layers, up to five "
                       f"reference pictures in both directions) at QP {qp}; per picture: closed-loop CTU search with the inter search on the device's own reference pictures -> "
                       "per-CTU deblocking + SAO -> arithmetic coder",
           "note": "the whole clip is one persistent launch: hand-out key cx + 2 cy + 4 x depth in the reference DAG, cross-picture per-CTU flags; the longest chain of "
                   "dependent pictures (11 levels for 65 pictures), not the picture count, bounds the wall time"}
    del loop
    if with_cpu:
        out["cpu_baseline"] = cpu_baseline_low_delay(W, H, depth, qp, total, gop="16")
    return out


def cpu_baseline_low_delay(W, H, depth, qp, frames, gop="lp-g4d3t1"):
    """The reference encoder's CLI (oracle/_ref, AVX2 strategies, its own thread pool at the defaults) on the same clip: --gop lp-g4d3t1
    (or the given GOP) --preset medium -q <qp>, all `frames` pictures, wall clock incl. reading the input."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    exe = os.path.join(ROOT, "oracle", "_ref", "uvg266_8" if depth == 8 else "uvg266_10")
    if not os.access(exe, os.X_OK):
        return None
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count()
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "in.yuv")
        with open(yuv, "wb") as f:
            for t in range(frames):
                for pl in Hh.clip_picture(W, H, t, depth):
                    f.write(np.ascontiguousarray(pl).tobytes())
        cmd = [exe, "-i", yuv, "--input-res", f"{W}x{H}", "-n", str(frames), "--preset", "medium", "--gop", gop, "-q", str(qp), "-o", os.path.join(tmp, "out.266")]
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        except (OSError, subprocess.TimeoutExpired):
            return None
        dt = time.perf_counter() - t0
        if r.returncode != 0 or not os.path.getsize(os.path.join(tmp, "out.266")):
            return None
    return {"value": round(frames / dt, 3), "unit": "frames/s", "cores": cores, "kind": "reference",
            "sample": f"the whole {frames}-picture {W}x{H} clip through the reference encoder's CLI (--preset medium --gop {gop} -q {qp}, --threads / --owf auto on "
                      f"{cores} host threads, AVX2 strategies), wall time {dt:.1f} s incl. reading the input"}


def tiles_sharded(device, rank, world, dist, n_pic=8, steps=3, grid=(4, 2)):
    """ONE stream's pictures with every picture's TILES spread over the ranks (uvg266_amd/tiles.py): 3840x2160 10-bit under
    --tiles 4x2 --wpp (a tile per GPU at 8 ranks), `n_pic` pictures per step.  A step = every rank's uvghip_tiles_plan_run over the tiles it
    owns of all pictures -- no halo, nothing exchanged while it runs -- then tiles.gather_nals: two all-gathers (substream lengths +
    checksum terms; the bytes) that leave the pictures' NAL units on rank 0.  Strong scaling: the pictures per step do not grow with the
    ranks.  Picture 0's NAL units are held to the reference's run with the same --tiles.  Not part of `value`."""
    import zlib
    from uvg266_amd import tiles as T
    wl = WORKLOADS["2160p10alf"]
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    P = api.ctu_params(W, H, QP)
    rects, _ = api.tile_grid(W, H, *grid)
    owner = T.assign(rects, world)
    src = [tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in layout.synthetic_yuv420(W, H, t % 4, depth)) for t in range(n_pic)]
    tl = api.TiledLoop(P, src, grid, owned=owner == rank)

    def step():
        tl.run()
        part = tl.substreams()
        if dist:
            return T.gather_nals(part, 0, True), part
        return T.write_nals(part[0][None], [part[1]], part[2][None], 0, True), part
    nals, part = step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        nals, part = step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    out = {"value": round(steps * n_pic / elapsed, 2), "unit": "frames/s", "ranks": world, "scaling": "strong", "steps": steps, "pictures_per_step": n_pic,
           "tiles": f"{grid[0]}x{grid[1]}", "tiles_of_rank0": int((owner == 0).sum()),
           "comm_bytes_per_step_rank0": {"sent": int(part[0].nbytes + part[2].nbytes * 2 + 8 + len(part[1])), "collectives": "2 x all_gather (lengths + checksum terms; bytes)"},
           "workload": f"{W}x{H} {depth}-bit, -p 1 --preset medium --tiles {grid[0]}x{grid[1]} --wpp at QP {QP}: every picture's tiles over {world} rank(s), "
                       "search + in-loop filters + slice data per tile, NAL units gathered on rank 0",
           "parity_checked": False}
    if rank == 0:
        path = os.path.join(ROOT, "tests", "golden", f"ref_tiles_{W}x{H}_{depth}_qp{QP}_{grid[0]}x{grid[1]}_1frames_crc.npz")
        if os.path.exists(path):
            g = np.load(path)
            out["parity_checked"] = bool(len(nals[0]) == int(g["bitstream_tail_len"]) and zlib.crc32(nals[0]) == int(g["bitstream_tail_crc"]))
            out["parity"] = "picture 0's slice NAL + hash SEI (length + CRC-32) vs the reference encoder's run with the same --tiles"
    return out


def search_rows(wl, device, rank, world, dist, transport, n_pic=64, steps=3):
    """The closed-loop CTU search with every picture sharded over the ranks by CTU rows (uvghip_ctu_plan_create_rows):
    a step = one launch of this rank's band of `n_pic` pictures, between the halo it receives from the band above (last reconstruction
    line, last side-information row, WPP models of each picture) and the halo it sends down -- grouped ncclSend / ncclRecv on the launch's
    stream, so rank r works on step s while rank r + 1 works on step s - 1.  Picture 0's band is compared with the reference encoder's
    record (per-CTU CRCs of the rows this rank owns) after the timed steps.  Not part of `value`."""
    import zlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    wc, hc = (W + 63) // 64, (H + 63) // 64
    lay = bands.BandLayout(H, world, rank)
    P = api.ctu_params(W, H, QP)
    host = layout.synthetic_yuv420(W, H, 0, depth)
    one = tuple(torch.from_numpy(np.ascontiguousarray(p)).to(device) for p in host)
    cs = api.CtuSearch(P, [one] * n_pic, rows=(lay.ctu_row0, lay.ctu_row1))
    up, down = [], []
    for i in range(n_pic):
        spec = lay.halo_search(cs.rec[i][0], cs.rec[i][1], cs.rec[i][2], cs.cu[i].view(hc * 16, wc * 16 * 32), cs.models[i].view(wc * hc, 3 * 257), wc)
        up += [o for o in spec if o[0] == lay.up and o[2]]
        down += [o for o in spec if o[0] == lay.down and o[1]]
    st = torch.cuda.current_stream().cuda_stream

    def step():
        if up:
            transport.exchange(up, st)
        cs.run()
        if down:
            transport.exchange(down, st)
    step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    # parity of this rank's band of picture 0 against the reference's record
    g = Hh.ctu_golden("ref_ctucrc_1920x1080_8_qp22" if (W, H, depth) == (1920, 1080, 8) else "ref_ctucrc_3840x2160_10_qp22")
    parity = None
    if zlib.crc32(b"".join(p.tobytes() for p in host)) == int(g["src_crc"]):
        ry, ru, rv = (x.cpu().numpy() for x in cs.rec[0])
        res = Hh.search_result_from_device_layout(W, H, ry, ru, rv, cs.cu[0].cpu().numpy().reshape(-1).view(Hh.SCU_NP), cs.coeff[0].cpu().numpy(),
                                                  cs.models[0].cpu().numpy().view(np.uint32))
        k0, k1 = lay.ctu_row0 * wc, lay.ctu_row1 * wc
        bad = int((Hh.ctu_crcs(res, W, H)[k0:k1] != g["crc"][k0:k1]).any(axis=1).sum())
        if bad:
            raise SystemExit(f"row-sharded search: {bad} CTUs of rank {rank}'s band differ from the reference's record")
        parity = {"ctus": k1 - k0, "items": "per-CTU CRC of side information + trees, reconstruction, levels, models: this rank's rows of picture 0"}
    sent, recv = bands.spec_bytes(down)[0], bands.spec_bytes(up)[1]
    return {"value": round(n_pic * steps / elapsed, 2), "unit": "frames/s", "ranks": world, "scaling": "strong", "pictures_per_step": n_pic, "steps": steps,
            "ctu_rows_of_rank0": [lay.ctu_row0, lay.ctu_row1], "halo_bytes_per_step": {"sent": int(sent), "received": int(recv)}, "parity_rank0_band": parity,
            "note": "the search only (the filters' row sharding is the open-loop line's); a band launch is a narrower wavefront than a whole picture, so "
                    "pictures per step matter more than on one GPU"}


def closed_loop(wl, steps, warmup, in_flight, device, rank, world, dist, groups=2):
    """`steps` timed launches of `in_flight` pictures each (a step = one group of pictures through search -> deblock -> SAO) after
    `warmup` untimed ones; `groups` launches are in flight at a time on their own streams, so the thin start of one launch's
    wavefronts overlaps the drain of the previous one.  -> (groups, pictures per step, elapsed seconds)"""
    F = max(1, in_flight)
    G = max(1, min(groups, steps))
    cls = [ClosedLoop(wl, (rank * G + g) * F, F, device) for g in range(G)]
    for k in range(warmup):
        cls[k % G].done.synchronize()
        cls[k % G].issue(False)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        g = cls[k % G]
        g.done.synchronize()            # the group's previous pass has retired (its buffers are reused)
        g.issue(True)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms = [c.search_ms() for c in cls]
    return cls, F, elapsed, sum(m[0] for m in ms), sum(m[1] for m in ms)


def cpu_baseline_reference(wl, frames=96, extra=(), dropin=None):
    """The reference encoder itself (oracle/_ref/uvg266_8: /root/reference built by oracle/build_ref.sh with plain gcc, AVX2 strategies
    and its own thread pool) on the GPU box's host cores: `frames` synthetic pictures of the workload, -p 1 --preset medium at the
    bench's QP, threads and frame parallelism at the encoder's defaults (auto).  A WHOLE encode (search, filters, bitstream): what the
    device's closed loop + coder replaces.  -> None when the binary is not there (then the oracle port is timed instead)."""
    import subprocess
    import tempfile
    exe = os.path.join(ROOT, "oracle", "_ref", "uvg266_8" if wl["depth"] == 8 else "uvg266_10")
    if not os.access(exe, os.X_OK):
        return None
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count()
    with tempfile.TemporaryDirectory() as tmp:
        yuv = os.path.join(tmp, "in.yuv")
        with open(yuv, "wb") as f:
            for t in range(frames):
                for pl in layout.synthetic_yuv420(W, H, t, depth):
                    f.write(np.ascontiguousarray(pl).tobytes())
        cmd = [exe, "-i", yuv, "--input-res", f"{W}x{H}", "-n", str(frames), "-p", "1", "--preset", "medium", "-q", str(QP), "-o", os.path.join(tmp, "out.266")] + list(extra)
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240)
        except (OSError, subprocess.TimeoutExpired):
            return None
        dt = time.perf_counter() - t0
        if r.returncode != 0 or not os.path.getsize(os.path.join(tmp, "out.266")):
            return None
        if dropin is not None:
            # the SAME encoder with the frame-level hand-over (oracle/_ref/uvg266_*_hip, UVG266_HIP_FRAME=1: DESIGN 4.19) on the same
            # file: its all-intra frames go through uvghip_frame_pool_* on this GPU, everything else of the encode is its own code
            try:
                import hashlib
                hip = exe + "_hip"
                if os.access(hip, os.X_OK):
                    out2 = os.path.join(tmp, "out_hip.266")
                    cmd2 = [hip if c == exe else out2 if c == os.path.join(tmp, "out.266") else c for c in cmd] + ["--threads", "8", "--owf", "63"]
                    env = dict(os.environ, UVG266_HIP_FRAME="1")
                    t1 = time.perf_counter()
                    r2 = subprocess.run(cmd2, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=240, env=env)
                    dt2 = time.perf_counter() - t1
                    md5 = [hashlib.md5(open(f_, "rb").read()).hexdigest() for f_ in (os.path.join(tmp, "out.266"), out2)] if r2.returncode == 0 else None
                    dropin.update({"value": round(frames / dt2, 3) if r2.returncode == 0 else None, "unit": "frames/s", "parity_checked": bool(md5 and md5[0] == md5[1]),
                                   "workload": f"the reference encoder's own CLI on the same {frames} pictures with its all-intra frames handed to the device (UVG266_HIP_FRAME=1 "
                                               f"--owf 63 --threads 8: uvg_encode_one_frame -> uvghip_frame_pool_begin, its bitstream job <- uvghip_frame_pool_finish); wall time of the "
                                               f"process {dt2:.1f} s incl. reading the input, HIP start-up and the pool's creation; parity = the .266 is byte for byte the file of the CPU "
                                               f"run beside it (cpu_baseline)"})
                    if r2.returncode != 0:
                        dropin["error"] = r2.stderr.decode(errors="replace")[-300:]
            except Exception as e:      # a side line: never in the way of the baseline
                dropin["error"] = repr(e)
    return {"value": round(frames / dt, 4), "unit": "frames/s", "cores": cores, "kind": "reference",
            "sample": f"{frames} synthetic {W}x{H} {depth}-bit pictures through the reference encoder's CLI (-p 1 --preset medium -q {QP}{''.join(' ' + e for e in extra)}, --threads / --owf auto "
                      f"on {cores} host threads, AVX2 strategies), wall time {dt:.1f} s incl. reading the input: a whole encode"}


def cpu_baseline_search(wl, seconds=12.0):
    """The same closed loop (search + coder model adaptation; no filters) by the oracle -- the C restatement of the reference's
    uvg_search_lcu / uvg_encode_coding_tree path that reproduces the reference-run goldens -- on the host cores: whole pictures in
    parallel threads (pictures are independent; inside a picture the CTUs are a dependency chain), repeated for about `seconds`."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers as Hh
    from concurrent.futures import ThreadPoolExecutor
    orc = Hh.load_oracle()
    W, H, depth = wl["W"], wl["H"], wl["depth"]
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count()
    threads = max(1, min(cores, 32))
    prm = Hh.search_params(W, H, QP)
    pics = [layout.synthetic_yuv420(W, H, t, depth) for t in range(threads)]
    done = 0
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        while done == 0 or time.perf_counter() - t0 < seconds:
            list(ex.map(lambda yuv: Hh.oracle_search_picture(orc, depth, prm, *yuv)["rec_y"][0, 0], pics))
            done += threads
    dt = time.perf_counter() - t0
    return {"value": round(done / dt, 4), "unit": "frames/s", "cores": threads, "kind": "port",
            "sample": f"{done} whole {W}x{H} pictures, {threads} at a time on {threads} of {cores} host threads ({dt:.1f} s): the closed-loop "
                      "CTU search + coder model adaptation of the step (no deblocking / SAO), oracle C -O2 single-threaded per picture.  "
                      "BASELINE.md has the reference's own full 1080p medium encode at 2.2 fps on 8 vCPU (AVX2)"}


def measure(args, wl_name, L, device, rank, local_rank, world, dist, transport, steps, warmup, n_resident, want_tables):
    wl = WORKLOADS[wl_name]
    shard_rows = world > 1 and args.shard == "rows"
    modes_dev = api.make_modes(MODES, device)
    F = max(1, args.group)
    while steps % F:                         # K pictures are timed exactly: the group size divides K
        F -= 1
    if shard_rows:
        groups = [pipeline.FrameGroup(L, wl, k * F, F, device, modes_dev, rank=rank, nranks=world, qp=QP, transport=transport,
                                      gather=not args.no_gather) for k in range(n_resident)]
    else:       # whole pictures per rank: rank r takes pictures r, r + world, ...
        groups = [pipeline.FrameGroup(L, wl, rank + k * F * world, F, device, modes_dev, step=world, qp=QP) for k in range(n_resident)]
    frames = [fr for g in groups for fr in g.frames]
    main_stream = torch.cuda.current_stream()
    streams = [torch.cuda.Stream(device=device) for _ in range(1 if args.serial else args.streams)]
    cap = torch.cuda.Stream(device=device)
    # one eager pass first: lazy per-kernel initialisation (function attributes) must not happen inside a capture
    for g in groups:
        pipeline.run(g.all_launches(), main_stream.cuda_stream)
    torch.cuda.synchronize()
    slots = [Slot(L, g, cap, use_graphs=not args.no_graphs) for g in groups]
    torch.cuda.synchronize()
    clock = KernelClock()

    def step(s, timed):       # one call = one GROUP of F pictures
        slots[s % n_resident].issue(clock, streams[s % len(streams)], timed)

    n_groups = steps // F
    clock.only = set()                       # warm-up: no events at all
    for s in range((warmup + F - 1) // F):
        step(s, False)
    torch.cuda.synchronize()

    # untimed profile pass: every kernel bracketed by HIP events, one stream, nothing concurrent
    prof = KernelClock()
    prof_groups = (args.profile_steps + F - 1) // F if want_tables else 0
    for s in range(prof_groups):
        slots[s % n_resident].issue_profiled(prof, main_stream)
    torch.cuda.synchronize()
    prof_tot = prof.totals()
    fam_ms = {}
    for name, (ms, _) in prof_tot.items():
        fam_ms[family(name)] = fam_ms.get(family(name), 0.0) + ms
    dom_family = max(fam_ms, key=fam_ms.get) if fam_ms else "intra_search"

    clock.only = {k for k in fam_ms if k.split("_chroma")[0] == dom_family.split("_chroma")[0]} if dom_family in ("intra_search", "rdoq", "rdoq_chroma") else {"intra_search"}
    for s in range(2):                       # back to the streamed plan after the serial pass
        step(s, False)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(n_groups):
        step(s, True)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    pics = steps if shard_rows else steps * world
    res = {"fps": pics / elapsed, "elapsed": elapsed, "frames": frames, "prof": prof_tot, "live": clock.totals(),
           "dom_family": dom_family, "shard_rows": shard_rows, "wl": wl, "prof_pics": prof_groups * F, "group": F}
    for sl in slots:
        for g in sl.graphs.values():
            g.destroy()
    return res


def kernel_table(fr, totals, pictures, group):
    """name -> per-launch average, per-picture total, share of a picture's kernel time, algorithmic bytes and GB/s."""
    t = {}
    for name, (ms, launches) in totals.items():
        byts = algorithmic_bytes(fr, name, group)
        avg_ms = ms / launches
        t[name] = {"avg_ms": round(avg_ms, 4), "per_step_ms": round(ms / max(1, pictures), 4), "share": 0.0, "alg_bytes": byts,
                   "launches": launches, "gbs": round(byts / (avg_ms * 1e-3) / 1e9, 2)}
    tot = sum(v["per_step_ms"] for v in t.values())
    for v in t.values():
        v["share"] = round(v["per_step_ms"] / tot, 3) if tot else 0.0
    return t, tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6, help="timed steps; a step is one group of --in-flight pictures through the closed loop")
    ap.add_argument("--warmup", type=int, default=2, help="untimed steps")
    ap.add_argument("--in-flight", type=int, default=224, help="pictures per step = per uvghip_ctu_plan_run launch (the reference's --owf)")
    ap.add_argument("--groups", type=int, default=2, help="launches in flight at a time, each on its own stream")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the post-run check of picture 0 against the reference encoder's record")
    ap.add_argument("--open-loop", action="store_true", help="also time the open-loop block-kernel path (rounds 1-2's headline; NOT an encode rate: off by default since round 6)")
    ap.add_argument("--no-open-loop", action="store_true", help="(accepted for old command lines; the open-loop measurement is off unless --open-loop)")
    ap.add_argument("--open-loop-steps", type=int, default=40)
    ap.add_argument("--serial", action="store_true", help="open loop: one stream, no overlap between pictures")
    ap.add_argument("--no-graphs", action="store_true", help="open loop: issue every launch eagerly instead of replaying hipGraph segments")
    ap.add_argument("--resident", type=int, default=0)
    ap.add_argument("--group", type=int, default=10, help="open loop: pictures per group")
    ap.add_argument("--streams", type=int, default=4, help="open loop: groups in flight")
    ap.add_argument("--profile-steps", type=int, default=4, help="open loop: untimed, fully instrumented steps for the per-kernel table")
    ap.add_argument("--shard", choices=("rows", "frames"), default="rows",
                    help="--gpus N > 1, open-loop / filter chain: rows = every picture split over the ranks by CTU rows with RCCL halo "
                         "exchanges (the secondary line \"row_sharded_rccl\"); the closed loop always shards whole pictures")
    ap.add_argument("--rccl-timeout", type=float, default=300.0, help="--gpus N > 1: seconds the row-sharded RCCL side measurement may take")
    ap.add_argument("--no-gather", action="store_true", help="--shard rows: skip the all-to-all of reconstructed bands")
    ap.add_argument("--workload", choices=("1080p8", "2160p10alf"), default="1080p8",
                    help="1080p8 = BASELINE.json configs[1] (the judged line); 2160p10alf = configs[3] geometry")
    ap.add_argument("--only-search-rows", action="store_true", help="time only the row-sharded closed-loop search (one rank: a band = the whole picture; development)")
    ap.add_argument("--only-clip", action="store_true", help="time only extra_workloads.c2_clip (development)")
    ap.add_argument("--only-c3", action="store_true", help="time only extra_workloads.c3_low_delay_closed_loop and print it (development)")
    ap.add_argument("--c3-clip-frames", type=int, default=120, help="extra_workloads.c3_clip: pictures of the ONE 120-picture low-delay clip that are timed (0: skip; 120: the whole clip)")
    ap.add_argument("--only-c3-clip", action="store_true", help="time only extra_workloads.c3_clip and print it (development)")
    ap.add_argument("--ra-clip-frames", type=int, default=65, help="extra_workloads.ra_clip: coded pictures of the ONE random-access (--gop 16) clip that are timed (0: skip)")
    ap.add_argument("--no-c4-clip", dest="c4_clip", action="store_false", help="skip extra_workloads.c4_clip (the 60-picture 2160p 10-bit clip and its CPU baseline)")
    ap.add_argument("--no-tiles-clip", dest="tiles_clip", action="store_false", help="skip extra_workloads.tiles_clip (the 60-picture clip under --tiles 6x4 --wpp and its CPU baseline)")
    ap.add_argument("--only-tiles-sharded", action="store_true", help="time only the tile-sharded 2160p 10-bit stream (every picture's tiles over the ranks; with one rank: all tiles here) and print it (development)")
    ap.add_argument("--only-tiles-clip", action="store_true", help="time only extra_workloads.tiles_clip and print it (development)")
    ap.add_argument("--only-c4-clip", action="store_true", help="time only extra_workloads.c4_clip and print it (development)")
    ap.add_argument("--only-2160p", action="store_true", help="time only extra_workloads.2160p10_closed_loop (with its ALF stage) and print it (development)")
    ap.add_argument("--only-ra-clip", action="store_true", help="time only extra_workloads.ra_clip and print it (development)")
    ap.add_argument("--c3-sequences", type=int, default=96, help="extra_workloads.c3_low_delay_closed_loop: independent low-delay sequences side by side")
    ap.add_argument("--no-extra", action="store_true", help="--full: do not also time the 2160p 10-bit closed loop (extra_workloads)")
    ap.add_argument("--full", action="store_true",
                    help="after the judged line also run the parity check against the reference encoder's record, extra_workloads, cpu_baseline "
                         "and (--gpus N > 1) row_sharded_rccl; a plain run times the judged line only")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist, transport = None, None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=device)
    L = lib.init(local_rank)
    if args.only_search_rows:
        print(json.dumps({"row_sharded_closed_loop_search": search_rows(WORKLOADS[args.workload], device, rank, world, dist, None)}), flush=True)
        return
    if args.only_clip:
        print(json.dumps({"c2_clip": c2_clip(WORKLOADS[args.workload], device)}), flush=True)
        return
    if args.only_2160p:
        # the 2160p 10-bit extra workload alone, as the full run measures it: closed loop, parity of picture 0, the ALF stage behind it
        ewl = WORKLOADS["2160p10alf"]
        ek, eF = 8, max(1, args.in_flight // 2)
        ecl, eF, eel, ems, eln = closed_loop(ewl, ek, 2, eF, device, 0, 1, None, args.groups)
        par = parity_check(ecl[0], "ref_ctucrc_3840x2160_10_qp22")
        alf_t = alf_stage_timing(ecl[0])
        out = {"value": round(ek * eF / eel, 3), "unit": "frames/s", "steps": ek, "pictures_per_step": eF, "ms_per_step": round(1e3 * eel / ek, 2),
               "search_launch_ms": round(ems / max(1, eln), 2), "parity": par, "alf_stage": alf_t}
        if alf_t and alf_t.get("parity_checked"):
            out["value_with_alf_stage"] = round(ek * eF / (eel + ek * alf_t["ms_per_group"] * 1e-3), 3)
        print(json.dumps({"2160p10_closed_loop": out}), flush=True)
        return
    if args.only_c4_clip:
        print(json.dumps({"c4_clip": c4_clip(device, with_cpu=not args.no_cpu_baseline)}), flush=True)
        return
    if args.only_tiles_sharded:
        if world == 1 and os.environ.get("RANK") is not None:          # under torchrun with ONE rank: the collectives through RCCL all the same
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=device)
        r = tiles_sharded(device, rank, world, dist)
        if rank == 0:
            print(json.dumps({"tiles_sharded": r}), flush=True)
        if dist:
            dist.destroy_process_group()
        return
    if args.only_tiles_clip:
        print(json.dumps({"tiles_clip": tiles_clip(WORKLOADS["1080p8"], device, with_cpu=not args.no_cpu_baseline)}), flush=True)
        return
    if args.only_ra_clip:
        print(json.dumps({"ra_clip": ra_clip(device, frames=args.ra_clip_frames or 65, with_cpu=not args.no_cpu_baseline)}), flush=True)
        return
    if args.only_c3_clip:
        print(json.dumps({"c3_clip": c3_clip(device, frames=args.c3_clip_frames or 120, with_cpu=not args.no_cpu_baseline)}), flush=True)
        return
    if args.only_c3:
        print(json.dumps({"c3_low_delay_closed_loop": low_delay_closed_loop(device, n_seq=args.c3_sequences)}), flush=True)
        return

    wl_name = args.workload
    wl = WORKLOADS[wl_name]
    # ---- the judged line: closed loop, K steps of F pictures per rank ----
    steps = args.steps
    cl, F, elapsed, search_ms, launches = closed_loop(wl, steps, args.warmup, args.in_flight, device, rank, world, dist, args.groups)
    n_groups = len(cl)
    if rank == 0 and args.dump_outputs:
        dump_outputs(cl[(steps - 1) % n_groups], args.dump_outputs)
    parity = None
    if args.full and rank == 0 and not args.no_parity:
        parity = [parity_check(cl[0], {"1080p8": "ref_ctucrc_1920x1080_8_qp22", "2160p10alf": "ref_ctucrc_3840x2160_10_qp22"}[wl_name])]
    del cl
    pics = steps * F * world
    fps = pics / elapsed
    extra = None
    if args.full and not args.no_extra and wl_name == "1080p8":
        ewl = WORKLOADS["2160p10alf"]
        ek, eF = 8, max(1, args.in_flight // 2)          # (a 4K picture has 93 diagonals of at most 34 CTUs: 112 pictures keep the 1024 workgroup slots fed)
        ecl, eF, eel, ems, eln = closed_loop(ewl, ek, 2, eF, device, rank, world, dist, args.groups)
        if parity is not None:
            parity.append(parity_check(ecl[0], "ref_ctucrc_3840x2160_10_qp22"))
        alf_t = None
        if rank == 0 and not args.no_parity:
            try:
                alf_t = alf_stage_timing(ecl[0])
            except Exception as e:          # noqa: BLE001 -- a side measurement must not take the judged line down with it
                alf_t = {"error": f"{type(e).__name__}: {e}"}
        del ecl
        extra = {"value": round(ek * eF * world / eel, 3), "unit": "frames/s", "steps": ek, "pictures_per_step": eF, "ms_per_step": round(1e3 * eel / ek, 2),
                 "mpixels_per_s": round(ek * eF * world / eel * ewl["W"] * ewl["H"] / 1e6, 1),
                 "search_launch_ms": round(ems / max(1, eln), 2),
                 "workload": "3840x2160 10-bit yuv420p, QP 22: the same closed loop (search -> deblock -> SAO -> slice data); alf_stage: the ALF stage of configs[3] behind it"}
        if eln:
            e_ms = ems / eln
            e_bytes = ctu_search_bytes(ewl["W"], ewl["H"], ewl["depth"]) * eF
            e_gbs = e_bytes / (e_ms * 1e-3) / 1e9
            extra["roofline"] = {"bound": "hbm", "kernel": "ctu_search_kernel<uint16_t>", "achieved": round(e_gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": round(e_gbs / HBM_PEAK_GBS, 6), "traffic": None, "avg_launch_ms": round(e_ms, 3), "alg_bytes_per_launch": e_bytes,
                                 "launches_timed": eln,
                                 "note": "as the headline's: algorithmic bytes of the search launch (source in; reconstruction, levels, side information, models out) / its "
                                         "average duration from HIP events on the launch's stream; an instruction chain per CTU, not a streaming kernel (no PMC pass at this size)"}
        if alf_t is not None:
            extra["alf_stage"] = alf_t
        if alf_t is not None and "ms_per_group" in alf_t and alf_t.get("parity_checked"):
            extra["value_with_alf_stage"] = round(ek * eF * world / (eel + ek * alf_t["ms_per_group"] * 1e-3), 3)        # (sequential: nothing of the stage overlaps the loop)
    c3 = c3_loop = clip = c3_one = ra_one = c4_one = tiles_one = None
    if args.full and not args.no_extra and wl_name == "1080p8" and rank == 0:
        def side(fn, *a, **k):          # a side workload must not take the judged line down with it
            try:
                return fn(*a, **k)
            except (Exception, SystemExit) as e:          # noqa: BLE001
                return {"error": f"{type(e).__name__}: {e}", "parity_checked": False}
        clip = side(c2_clip, wl, device)
        tiles_one = side(tiles_clip, wl, device, with_cpu=not args.no_cpu_baseline) if args.tiles_clip else None
        c3 = side(inter_hot_path, device)
        c3_loop = side(low_delay_closed_loop, device, n_seq=args.c3_sequences)
        c4_one = side(c4_clip, device, with_cpu=not args.no_cpu_baseline) if args.c4_clip else None
        c3_one = side(c3_clip, device, frames=args.c3_clip_frames, with_cpu=not args.no_cpu_baseline) if args.c3_clip_frames > 0 else None
        ra_one = side(ra_clip, device, frames=args.ra_clip_frames, with_cpu=not args.no_cpu_baseline) if args.ra_clip_frames > 0 else None
    open_loop = None
    if args.open_loop and world == 1:
        ol_steps = (max(args.group, args.open_loop_steps) + args.group - 1) // args.group * args.group
        r = measure(args, wl_name, L, device, rank, local_rank, world, None, None, ol_steps, min(args.warmup, 4), args.resident or 2, True)
        fr = r["frames"][0]
        per_kernel, tot_ms = kernel_table(fr, r["prof"], r["prof_pics"], r["group"])
        top = sorted(per_kernel.items(), key=lambda kv: -kv[1]["per_step_ms"])[:12]
        open_loop = {"value": round(r["fps"], 2), "unit": "frames/s", "steps": ol_steps, "kernel_sum_ms": round(tot_ms, 4), "kernels_top": dict(top),
                     "workload": workload_text(r["wl"], "frames", 1),
                     "note": "throughput of the batched block kernels with open-loop references and no RD decision: every picture is coded once per "
                             "block size (four times over); NOT an encode rate -- kept for continuity with rounds 1-2"}
    def emit(row_sharded):
        if rank == 0:
            launch_ms = search_ms / max(1, launches)
            byts = ctu_search_bytes(wl["W"], wl["H"], wl["depth"]) * F
            gbs = byts / (launch_ms * 1e-3) / 1e9
            wc, hc = (wl["W"] + 63) // 64, (wl["H"] + 63) // 64
            out = {
                "metric": f"encoded fps ({wl['H']}p all-intra --preset medium closed loop: CTU search with the reference's RD decisions -> deblock -> SAO -> slice data; Mpixels/s in config)",
                "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": steps, "warmup": args.warmup,
                "ms_per_step": round(1e3 * elapsed / steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "u8" if wl["depth"] == 8 else "u16", "data": "synthetic",
                "parity_checked": parity is not None, "parity": parity,
                "config": {"workload": f"{wl['W']}x{wl['H']} {wl['depth']}-bit yuv420p, -p 1 --preset medium at QP {QP} (BASELINE.json configs[1]): per picture "
                                       "uvghip_ctu_plan_run (closed-loop CTU search bit-identical with the reference: partition, modes, levels, "
                                       "reconstruction, CABAC models) -> deblocking on the search's side information -> SAO statistics / decision "
                                       "(edge, band, merge) / apply for Y, U, V -> the arithmetic coder (uvghip_encode_slice_rows: the slice data of the encoder's .266, "
                                       "byte for byte); all of it one uvghip_loop_plan_run per group",
                           "mpixels_per_s": round(fps * wl["W"] * wl["H"] / 1e6, 2), "qp": QP,
                           "step": f"one group of {F} pictures through the closed loop (one uvghip_loop_plan_run: the search launch, the filter chain of its pictures, the slice coder launch)",
                           "pictures_per_step": F, "pictures_timed": steps * F * world, "groups_in_flight": n_groups, "timed_region_s": round(elapsed, 3),
                           "ctus_per_picture": wc * hc, "wavefront_steps_per_picture": wc + hc - 1,
                           "parallelism": f"whole pictures over {world} rank(s) (all-intra pictures are independent), {F} pictures per launch, "
                                          f"{n_groups} launches in flight on their own streams; inside a picture one workgroup per CTU on the WPP wavefront",
                           "note": "the in-loop filters follow the reference's schedule: SAO statistics on every CTU deblocked by its own edges only "
                                   "(uvghip_deblock_frame_sao_snapshot; sao.c:641-668), the whole sao_search_best_mode decision with the coder's SAO "
                                   "models (uvghip_sao_decide_pictures), SAO of the deblocked picture -- the output is the picture the encoder returns, "
                                   "bit for bit (tests/test_gpu_sao_decide.py against reference-run records at 1080p and 2160p)"},
                "roofline": {"bound": "hbm", "kernel": "ctu_search_kernel", "achieved": round(gbs, 3), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(gbs / HBM_PEAK_GBS, 6),
                             "traffic": ctu_search_traffic(F),
                             "avg_launch_ms": round(launch_ms, 3), "alg_bytes_per_launch": byts, "launches_timed": launches, "launches_in_flight": n_groups,
                             "effective_gbs": round(byts * launches / elapsed / 1e9, 3),
                             "note": "the dominant kernel (~ 90 % of the GPU time of the step) is the whole-CTU search: one workgroup walks one CTU's quad tree, "
                                     "CTUs of a picture are a wavefront of dependent workgroups.  It is an instruction chain per CTU, not a streaming kernel "
                                     "(DESIGN.md 4.13: a lone wave pays ~8 cycles per dependent instruction, an LDS round trip 52): achieved = algorithmic bytes "
                                     "(source in, reconstruction / levels / side information / models out) / average launch duration from HIP events on the "
                                     "launch stream.  Round-5 counters (profiles/r05_bench_sq_insts.json, _sq_occupancy.json, one launch in flight): 4.3 M VALU + "
                                     "3.0 M scalar + 0.4 M LDS instructions per CTU (round 4: 10.4 M + 7.1 M), i.e. ~58 % of the wave64 VALU issue peak while it "
                                     "runs, 57 % of the wave cycles waiting.  traffic (PMC FETCH_SIZE x 2 + WRITE_SIZE, fabric side of the L2, "
                                     "profiles/r05_bench_hbm_traffic.json) is ~114 x the algorithmic bytes (round 3: 197 x): the call stack of the out-of-line "
                                     "functions (callee-saved VGPRs written through to the fabric) and the per-workgroup global scratch, not re-reads of the "
                                     "pictures; ~0.34 TB/s while the kernel runs, 4 % of the peak"},
            }
            if extra is not None:
                out["extra_workloads"] = {"2160p10_closed_loop": extra}
            if c3 is not None:
                out.setdefault("extra_workloads", {})["c3_inter_hot_path_open_loop"] = c3
            if c3_loop is not None:
                out.setdefault("extra_workloads", {})["c3_low_delay_closed_loop"] = c3_loop
            if c3_one is not None:
                out.setdefault("extra_workloads", {})["c3_clip"] = c3_one
            if ra_one is not None:
                out.setdefault("extra_workloads", {})["ra_clip"] = ra_one
            if clip is not None:
                out.setdefault("extra_workloads", {})["c2_clip"] = clip
            if tiles_one is not None:
                out.setdefault("extra_workloads", {})["tiles_clip"] = tiles_one
            if c4_one is not None:
                out.setdefault("extra_workloads", {})["c4_clip"] = c4_one
            if open_loop is not None:
                out["open_loop"] = open_loop
            if row_sharded is not None:
                out["row_sharded_rccl"] = row_sharded
            if args.full and world == 1 and not args.no_cpu_baseline and wl_name == "1080p8":
                dropin = {}
                out["cpu_baseline"] = cpu_baseline_reference(wl, dropin=dropin) or cpu_baseline_search(wl)
                if dropin:
                    out.setdefault("extra_workloads", {})["reference_cli_frame_handover"] = dropin
            print(json.dumps(out), flush=True)

    row_sharded = None
    if args.full and world > 1 and args.shard == "rows":
        # The row-sharded RCCL plan is a secondary line and the only part of the run with data-path collectives on a device set this
        # code has never met: if it does not finish in time the judged line is still printed (by a watchdog) and the process ends.
        import threading

        def give_up():
            emit({"error": f"the row-sharded RCCL measurement did not finish within {args.rccl_timeout} s", "rccl_ranks": world})
            os._exit(0)
        dog = threading.Timer(args.rccl_timeout, give_up)
        dog.daemon = True
        dog.start()
        try:
            def bootstrap(raw):                  # the 128-byte RCCL unique id travels over the launcher's process group
                box = [raw]
                dist.broadcast_object_list(box, src=0)
                return box[0]
            transport = bands.RcclTransport(rank, world, bootstrap)
            rs_steps = (max(args.group, 20) + args.group - 1) // args.group * args.group
            r = measure(args, "2160p10alf", L, device, rank, local_rank, world, dist, transport, rs_steps, 2, 2, False)
            cb = r["frames"][0].comm_bytes()
            row_sharded = {"value": round(r["fps"], 2), "unit": "frames/s", "rccl_ranks": world, "scaling": "strong", "steps": rs_steps,
                           "workload": workload_text(r["wl"], "rows", world),
                           "comm_bytes_per_step_rank0": {k: {"sent": v[0], "received": v[1]} for k, v in cb.items()},
                           "note": "open-loop block kernels + in-loop filter chain of 2160p10alf with every picture split over the ranks by CTU rows: "
                                   "halo rows and reconstructed bands over RCCL (grouped ncclSend/ncclRecv, ncclAllReduce of the ALF covariances)"}
            try:
                rs = search_rows(WORKLOADS["1080p8"], device, rank, world, dist, transport)
            except Exception as e:               # noqa: BLE001
                rs = {"error": f"{type(e).__name__}: {e}"}
            row_sharded["closed_loop_search_rows"] = rs
            try:
                ts = tiles_sharded(device, rank, world, dist)
            except Exception as e:               # noqa: BLE001
                ts = {"error": f"{type(e).__name__}: {e}"}
            row_sharded["tiles_sharded"] = ts
        except Exception as e:                   # noqa: BLE001 -- reported, not fatal: the judged line does not depend on it
            row_sharded = {"error": f"{type(e).__name__}: {e}", "rccl_ranks": world}
        dog.cancel()
    emit(row_sharded)
    if transport is not None:
        transport.close()
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
