"""What the tests of ALF in the P / B picture loop share (tests/test_alf_pb_nal.py, tests/test_gpu_alf_pb_loop.py): the ref_inter_*_alf goldens
(tools/refcheck/make_ctu_goldens.py::inter(alf=True): an --alf full run with a GOP structure, one worker thread, no frames in flight -- per
coded picture the rows of the real coding pass, the decisions ALF took, the picture it got and the picture it left, and the APS NAL units in
the order they were written) and the library's host writer over them."""
import ctypes
import os

import numpy as np

import helpers as H

GOLDENS = ["ref_inter_192x128_8_qp22_17frames_ra16_alf", "ref_inter_192x128_10_qp24_9frames_alf", "ref_inter_136x72_8_qp27_17frames_ra16_alf"]
ALF_KEYS = ("alf_meta", "alf_flags", "alf_set_idx", "alf_luma_aps", "alf_chroma_aps", "alf_cc_coeff")
_CACHE = {}


def golden(name):
    """The whole file as a dict, read once (tests leave it unchanged).  `display` etc. as helpers.golden_sources wants them: the .files list too."""
    if name not in _CACHE:
        with np.load(os.path.join(H.GOLDEN, name + ".npz")) as z:
            d = {k: z[k] for k in z.files}
        first = {}
        for k in range(len(d["meta"])):
            first.setdefault(int(d["meta"][k][0]), k)
        d["_first"] = first
        _CACHE[name] = d
    return _CACHE[name]


class Files(dict):
    """A golden dict with the `.files` attribute helpers' functions look for."""
    @property
    def files(self):
        return [k for k in self if not k.startswith("_")]


def frame_state(g, f):
    """(slice_type, frame_qp, poc, reference POCs) of coded picture f."""
    k = g["_first"][f]
    n_refs = int(g["refs"][k][0])
    return int(g["meta"][k][6]), int(g["meta"][k][7]), int(g["refs"][k][51]), [int(p) for p in g["refs"][k][1:1 + n_refs]]


def picture_decisions(g, f):
    """Coded picture f's ALF decisions under the key names api.ClosedLoop.alf_stage's tests use (meta, flags, set_idx, luma_aps, chroma_aps, cc_coeff)."""
    return {k[4:]: g[k][f] for k in ALF_KEYS}


def golden_rows(g, f):
    W, Hh = int(g["dims"][0]), int(g["dims"][1])
    hc = (Hh + 63) // 64
    off = g["row_off"][f * hc:f * hc + hc + 1]
    sizes = np.diff(off).astype(np.int32)
    rows = np.zeros((hc, int(sizes.max())), np.uint8)
    for r in range(hc):
        rows[r, :sizes[r]] = g["row_bytes"][off[r]:off[r + 1]]
    return rows, sizes


def alf_structs(g, f, zero=False):
    """uvghip_alf_slice_t and the uvghip_alf_aps_t array of coded picture f (zero: ALF on in the SPS, everything off in this slice, no APS)."""
    from uvg266_amd import lib
    m = g["alf_meta"][f]
    S = lib.AlfSlice()
    S.alf_type = int(m[3])
    keep = []
    if zero:
        return S, (lib.AlfAps * 1)(), 0, keep
    for c in range(3):
        S.enabled[c] = int(m[4 + c])
    S.n_luma_aps = int(m[7])
    for i in range(8):
        S.luma_aps_id[i] = int(m[9 + i])
    S.chroma_aps_id = int(m[8])
    for c in range(2):
        S.cc_enabled[c] = int(m[17 + c]); S.cc_aps_id[c] = int(m[23 + c])
    sel = np.flatnonzero(g["aps_meta"][:, 0] == f) if len(g["aps_meta"]) else []
    A = (lib.AlfAps * max(len(sel), 1))()
    for i, j in enumerate(sel):
        a = g["aps_meta"][j]
        A[i].aps_id = int(a[2])
        for c in range(2):
            A[i].new_filter[c] = int(a[4 + c]); A[i].non_linear[c] = int(a[6 + c]); A[i].new_cc_filter[c] = int(a[10 + c]); A[i].cc_filter_count[c] = int(a[12 + c])
        A[i].num_luma_filters, A[i].num_alternatives_chroma = int(a[8]), int(a[9])
        arrs = [np.ascontiguousarray(g[k][j], np.int16) for k in ("aps_luma", "aps_chroma", "aps_cc")]
        keep.append(arrs)
        A[i].luma, A[i].chroma, A[i].cc = (x.ctypes.data_as(ctypes.c_void_p) for x in arrs)
    return S, A, len(sel), keep


def nal_type_of(g, slice_type, poc, irap_poc):
    """pictype (src/encoderstate.c:1957-1972) of a picture of these streams: the first picture IDR_N_LP, a later I picture CRA, the pictures before it
    in display order coded after it RASL, the rest TRAIL."""
    if slice_type == 2:
        return 8 if poc == 0 else 9
    return 3 if poc < irap_poc else 0


def write_picture(L, g, f, rows, sizes, sums, irap_poc=0, zero=False):
    """uvghip_write_picture_nals_gop_alf on coded picture f -> bytes."""
    slice_type, frame_qp, poc, ref_pocs = frame_state(g, f)
    qp0 = int(g["dims"][3])
    cfg = g["cfg"]
    ra = H.is_random_access(Files(g))
    neg = np.ascontiguousarray(sorted(poc - p for p in ref_pocs if p < poc), np.int32)
    pos = np.ascontiguousarray(sorted(p - poc for p in ref_pocs if p > poc), np.int32)
    if slice_type == 2 and poc == 0:
        neg, pos = neg[:0], pos[:0]
    S, A, n_aps, keep = alf_structs(g, f, zero)
    sizes = np.ascontiguousarray(sizes, np.int32)
    sums = np.ascontiguousarray(sums, np.uint32)
    cap = int(sizes.sum()) + 8192
    out = np.zeros(cap, np.uint8)
    n = ctypes.c_size_t(0)
    rc = L.uvghip_write_picture_nals_gop_alf(nal_type_of(g, slice_type, poc, irap_poc), poc, H.poc_lsb_bits(Files(g)), slice_type, len(neg), H.ptr(neg) if len(neg) else None,
                                             len(pos), H.ptr(pos) if len(pos) else None, 0 if ra else int(cfg[3]), int(cfg[0]), frame_qp - qp0, 1, ctypes.byref(S), A, n_aps,
                                             H.ptr(rows), rows.shape[1], H.ptr(sizes), len(sizes), H.ptr(sums), H.ptr(out), cap, ctypes.byref(n))
    assert rc == 0, L.uvghip_last_error()
    return out[:n.value].tobytes()


def parameter_sets_end(stream):
    """Where the first picture's own NAL units start in the .266: its first APS (NAL unit type 17), or its slice (IDR_N_LP) when it has none."""
    at = [p for p in (stream.find(b"\x00\x00\x01\x00\x89"), stream.find(b"\x00\x00\x01\x00\x41")) if p > 0]
    assert at
    return min(at)
