"""The NAL units of --alf full streams WITH a GOP structure (BASELINE configs[3]: --gop 16 with ALF on every picture) from the library's host
writer, uvghip_write_picture_nals_gop_alf: the APS NAL units in front of P / B pictures, the slice header's ALF fields between the slice type
and the reference picture lists, the POC in poc_lsb_bits bits -- against the real encoder's .266 (tests/golden/ref_inter_*_alf.npz,
tools/refcheck/make_ctu_goldens.py::inter(alf=True)), byte for byte.  No device needed.

No golden exercises ALF at a partial CTU: every clip with a partial CTU that was tried (136x72, 200x136, 264x136, 328x200 at QP 17 - 27) kept
ALF off in every picture.  The 136x72 golden keeps the case such a size does show: the SPS says ALF, every slice header says no."""
import ctypes

import numpy as np
import pytest

import alf_pb_helpers as A
import helpers as H


def pb_pictures(g):
    frames = int(g["dims"][4])
    return [f for f in range(frames) if A.frame_state(g, f)[0] != 2]


def test_the_goldens_keep_their_coverage():
    """What the three files were chosen for, from their own records: a regenerated golden cannot quietly lose it."""
    enabled = aps_nals = multi_aps = cc_on = off_between = 0
    for name in A.GOLDENS[:2]:
        g = A.golden(name)
        m = g["alf_meta"]
        pb = pb_pictures(g)
        enabled += sum(int(m[f][4]) == 1 for f in pb)
        aps_nals += sum(int(a[0]) in pb for a in g["aps_meta"])
        multi_aps += sum(int(m[f][4]) == 1 and int(m[f][7]) >= 2 for f in pb)
        cc_on += sum(bool(m[f][17] or m[f][18]) for f in pb)
        any_on = [bool(m[f][4:7].any() or m[f][17:19].any()) for f in range(len(m))]
        off_between += sum(not any_on[f] and any_on[f - 1] and f + 1 < len(m) and any_on[f + 1] for f in pb)
        # every item is per coded picture, in coding order
        assert [int(a) for a in m[:, 0]] == list(range(len(m))) and [int(m[f][26]) for f in range(len(m))] == [A.frame_state(g, f)[0] for f in range(len(m))]
        assert g["alf_pre_y"].shape == g["final_y"].shape and g["alf_flags"].shape[1] == 7
    assert enabled >= 12 and aps_nals >= 5 and multi_aps >= 2 and cc_on >= 2 and off_between >= 1, (enabled, aps_nals, multi_aps, cc_on, off_between)
    g = A.golden(A.GOLDENS[2])
    assert not g["alf_meta"][:, 4:7].any() and not g["alf_meta"][:, 17:19].any() and len(g["aps_meta"]) == 0
    assert (g["alf_meta"][:, 3] == 2).all()          # ... in a run with --alf full
    assert int(g["dims"][0]) % 64 and int(g["dims"][1]) % 64          # partial CTUs at both edges


@pytest.mark.parametrize("name", A.GOLDENS)
def test_whole_file_from_rows_decisions_and_final_pictures(name):
    """Picture by picture in coding order: the golden's own rows, its recorded decisions and APSs, the checksum of the picture ALF left (in numpy)
    through uvghip_write_picture_nals_gop_alf; behind the encoder's parameter sets the concatenation is the encoder's .266."""
    from uvg266_amd import lib
    L = lib.load_library()
    g = A.golden(name)
    depth, frames = int(g["dims"][2]), int(g["dims"][4])
    stream = g["bitstream"].tobytes()
    mine, irap_poc = b"", 0
    for f in range(frames):
        rows, sizes = A.golden_rows(g, f)
        sums = [H.picture_checksum(g[k][f], depth) for k in ("final_y", "final_u", "final_v")]
        mine += A.write_picture(L, g, f, rows, sizes, sums, irap_poc)
        slice_type, _, poc, _ = A.frame_state(g, f)
        if slice_type == 2:
            irap_poc = poc
    at = A.parameter_sets_end(stream)
    body = stream[at:]
    if body != mine:
        i = next((j for j in range(min(len(body), len(mine))) if body[j] != mine[j]), min(len(body), len(mine)))
        assert False, (name, "first differing byte", i, body[max(0, i - 8):i + 8].hex(), mine[max(0, i - 8):i + 8].hex(), len(body), len(mine))
    assert stream[:at] + mine == stream


def header_bits(nals, first_row):
    """The slice header of a picture's NAL units as a bit string: behind the start code and the two NAL header bytes, emulation prevention
    removed, up to the rbsp alignment in front of the first row."""
    end = nals.find(first_row)
    assert nals[:4] == b"\x00\x00\x00\x01" and end > 6
    raw, zeros = bytearray(), 0
    for b in nals[6:end]:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        zeros = zeros + 1 if b == 0 else 0
        raw.append(b)
    bits = "".join(f"{b:08b}" for b in raw)
    return bits[:bits.rindex("1")]          # (byte_alignment: a one, then zeros)


def test_a_slice_with_alf_off_differs_from_the_plain_writer_by_one_flag():
    """alf all zero, n_aps = 0: the bytes are the 136x72 golden's stream's (ALF on in the SPS, off in every slice), and against
    uvghip_write_picture_nals_gop's header they hold one more bit -- slice_alf_enabled_flag = 0 behind sh_slice_type."""
    from uvg266_amd import lib
    L = lib.load_library()
    g = A.golden(A.GOLDENS[2])
    depth = int(g["dims"][2])
    stream = g["bitstream"].tobytes()
    checked = set()
    for f in pb_pictures(g)[:4]:
        slice_type, frame_qp, poc, ref_pocs = A.frame_state(g, f)
        rows, sizes = A.golden_rows(g, f)
        sums = np.ascontiguousarray([H.picture_checksum(g[k][f], depth) for k in ("final_y", "final_u", "final_v")], np.uint32)
        new = A.write_picture(L, g, f, rows, sizes, sums, zero=True)
        assert stream.count(new) == 1, ("the golden's stream holds the new writer's bytes", f)
        out, n = np.zeros(len(new) + 64, np.uint8), ctypes.c_size_t(0)
        assert H.write_inter_nals(L, A.Files(g), poc, slice_type, ref_pocs, int(g["cfg"][3]), int(g["cfg"][0]), frame_qp - int(g["dims"][3]), rows, sizes, sums, out, n) == 0
        old = out[:n.value].tobytes()
        assert stream.count(old) == 0
        a, b = header_bits(new, rows[0, :sizes[0]].tobytes()), header_bits(old, rows[0, :sizes[0]].tobytes())
        # picture header in the slice header (1), gdr_or_irap, non_ref, inter allowed, intra allowed (4), ue(pps id) (1), the POC, tmvp, mvd_l1_zero (2), ue(slice type)
        at = 6 + H.poc_lsb_bits(A.Files(g)) + int(g["cfg"][0]) + 1 + (1 if slice_type == 0 else 3)
        assert len(a) == len(b) + 1 and a == b[:at] + "0" + b[at:], (f, at, a, b)
        checked.add(slice_type)
    assert checked == {0, 1}          # a P and a B picture
