"""The slice coder's coefficient path (code_coeffs in uvg266_amd/csrc/slice_coder.hip: the models' sweep on all lanes, the bins' byte
stream, lane 0's range coder) on CRAFTED levels: the hand-over of a 128x128 picture comes from the oracle's search, the levels of every
block whose cbf is set are replaced by seeded levels that hit what real pictures at the goldens' QPs hardly do -- the regular-bin budget
ending inside a group, exactly at a group's end, groups it never reaches, inferred sig flags, DC-only blocks, the last position in the
far corner, remainders on both sides of 5 << rice for every Rice parameter, levels of +-32767, groups of all +-1 -- and the expected bytes
come from the oracle's row coder on that hand-over.  Two rows of CTUs: row 1 starts from the models behind the first CTU of row 0.

The mutant this file is aimed at: the budget test of code_coeffs with `>= 3` in place of `>= 4` (`regular = pos && reg_bins - before >= 3`).
Built and run once: both GPU cases below fail on it; of the QP 22 goldens of test_gpu_slice_coder.py the 832x480 and the 1920x1080 8-bit
pictures pass on it (the 3840x2160 10-bit picture does catch it)."""
import functools

import numpy as np
import pytest

import helpers as H

# (depth, QP, picture): 8 bit at QP 22 -- mostly 4x4 / 8x8 CUs, some of every size; 10 bit at a high QP on smooth content -- 16x16, 32x32, 64x64
CASES = [(8, 22, 3), (10, 42, 5)]
W = HH = 128


def _zxy(z):
    return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4) | ((z >> 3) & 8)


@functools.lru_cache(None)
def scan_of(n):
    """H.266 6.5.2: the up-right diagonal scan of an n x n block in 4x4 groups (raster index per scan position)."""
    def diag(w):
        return [(x, d - x) for d in range(2 * w - 1) for x in range(d + 1) if x < w and d - x < w]
    return np.array([(gy * 4 + y) * n + gx * 4 + x for gx, gy in diag(n // 4) for x, y in diag(4)])


def transform_blocks(cu, W, Hh):
    """The coded transform blocks of a hand-over in the layout of H.oracle_search_picture: (CTU, colour, offset in the CTU's 6144 levels, row
    stride, n) of every block whose cbf is set, as uvg_encode_coding_tree visits them (intra pictures)."""
    out = []
    wc = (W + 63) // 64
    for cy in range((Hh + 63) // 64):
        for cx in range(wc):
            for z in range(256):
                lx, ly = _zxy(z) * 4, _zxy(z >> 1) * 4
                x, y = cx * 64 + lx, cy * 64 + ly
                if x >= W or y >= Hh:
                    continue
                n = 1 << int(cu[y // 4, x // 4, 1])
                if (lx & (n - 1)) or (ly & (n - 1)):
                    continue
                k = cy * wc + cx
                tn = min(n, 32)
                for tu in range(4 if n == 64 else 1):
                    tlx, tly = lx + (tu & 1) * 32, ly + (tu >> 1) * 32
                    cbf = int(cu[(cy * 64 + tly) // 4, (cx * 64 + tlx) // 4, 5])
                    if cbf & 1:
                        out.append((k, 0, tly * 64 + tlx, 64, tn))
                    if n > 4:
                        for c in (1, 2):
                            if cbf >> c & 1:
                                out.append((k, c, 4096 + 1024 * (c - 1) + (tly // 2) * 32 + tlx // 2, 32, tn // 2))
                if n == 4 and (lx & 4) and (ly & 4):          # the 8x8 area's chroma behind its last luma CU: the cbf of the area's first entry
                    cbf = int(cu[(y & ~7) // 4, (x & ~7) // 4, 5])
                    for c in (1, 2):
                        if cbf >> c & 1:
                            out.append((k, c, 4096 + 1024 * (c - 1) + ((ly & ~7) // 2) * 32 + (lx & ~7) // 2, 32, 4))
    return out


def rice_of(s):
    return (s >= 7) + (s >= 14) + (s >= 28)


def walk(lv, n):
    """A plain walk of uvg_encode_coeff_nxn's scan over the n x n levels: -> the set of classes the block shows."""
    scan = scan_of(n)
    flat = lv.reshape(-1)
    a = np.abs(flat[scan].astype(np.int64))
    nz = np.nonzero(a)[0]
    last = int(nz[-1])
    cls = set()
    if last == 0:
        cls.add("dc_only")
    if scan[last] == n * n - 1:
        cls.add("far_corner")
    if (flat == 32767).any():
        cls.add("level+32767")
    if (flat == -32767).any():
        cls.add("level-32767")
    pad = np.zeros((n + 2, n + 2), np.int64)
    pad[:n, :n] = np.abs(lv.astype(np.int64))

    def tsum(sp):          # the sum of the template's five levels: right, right + 1, below right, below, below + 1
        y, x = divmod(int(scan[sp]), n)
        return int(pad[y, x + 1] + pad[y, x + 2] + pad[y + 1, x + 1] + pad[y + 1, x] + pad[y + 2, x])

    rb = (n * n * 28) >> 4
    cg_last = last >> 4
    coded = [g for g in range(cg_last + 1) if g in (0, cg_last) or a[g * 16:g * 16 + 16].any()]
    for g in reversed(coded):
        lo = g * 16
        first = last if g == cg_last else lo + 15
        infer = (lo if g else -1) if first != last else first
        sp, num_nz = first, 0
        while sp >= lo and rb >= 4:
            if num_nz or sp != infer:
                rb -= 1
            elif sp != last:
                cls.add("inferred_sig")
            if a[sp]:
                num_nz += 1
                rb -= 1 if a[sp] == 1 else 3
                if a[sp] >= 4:
                    rice, rem = rice_of(min(max(tsum(sp) - 20, 0), 31)), (int(a[sp]) - 4) >> 1
                    cls.add(("remainder", rice, "below" if rem < 5 << rice else "above"))
            sp -= 1
        regular = first - sp
        if rb < 4:
            if sp >= lo:
                cls.add("budget_ends_inside" if regular else "group_never_reached")
            elif regular and g > 0:          # (group 0 is always coded: something follows in bypass)
                cls.add("budget_ends_at_group_end")
        if regular and (a[lo:lo + 16] == 1).all():          # (reached by the regular bins; sixteen +-1 cost 31 or 32 of them, a 4x4 block has 28)
            cls.add("group_all_ones")
        for q in range(sp, lo - 1, -1):
            rice = rice_of(min(tsum(q), 31))
            pos0 = 1 << rice
            v = pos0 if a[q] == 0 else (int(a[q]) - 1 if a[q] <= pos0 else int(a[q]))
            cls.add(("bypass", rice, "below" if v < 5 << rice else "above"))
    return cls


def craft(rng, n, want, extremes):
    """n x n levels of class `want`, at least one of them nonzero; extremes: a dense block also holds +32767 and -32767."""
    nn = n * n
    scan = scan_of(n)

    def mags(size, top):          # magnitudes 1 .. top, about as many per octave
        return np.minimum(np.exp(rng.random(size) * np.log(top + 1.0)).astype(np.int64), top)

    for attempt in range(2000):
        s = np.zeros(nn, np.int64)          # by scan position
        if want == "dc":
            s[0] = rng.choice([1, 2, 5, 300, 32767])
        elif want in ("inside", "exact"):
            # dense from the far corner down, so that the budget is spent; below its end whatever the dice give
            s[:] = mags(nn, int(rng.choice([2, 6, 40, 2000]))) * (rng.random(nn) < rng.choice([0.5, 0.8, 1.0]))
            head = rng.random(nn) < rng.choice([0.6, 0.9, 1.0])
            s = np.where(head, np.maximum(s, rng.integers(1, 4, nn)), s)
            s[nn - 1] = max(s[nn - 1], 1)
        elif want == "ones":
            s[:] = 1
        else:          # "sparse": groups with only their first position set, groups of all ones, empty groups, lone large levels
            ng = nn // 16
            kinds = rng.integers(0, 5, ng)
            if ng > 2:          # one group of each of the two kinds between the ends, whatever the dice give the others
                kinds[rng.permutation(np.arange(1, ng - 1))[:2]] = [0, 1][:ng - 2]
            for g in range(ng):
                if ng > 1 and kinds[g] == 0:
                    s[g * 16] = mags(1, 300)[0]
                elif ng > 1 and kinds[g] == 1:
                    s[g * 16:g * 16 + 16] = 1
                elif ng == 1 or kinds[g] == 3:
                    s[g * 16:g * 16 + 16] = mags(16, 3000) * (rng.random(16) < 0.2)
            s[nn - 16 + rng.integers(0, 16)] = mags(1, 300)[0]          # (the last group is the block's last)
        s = s * rng.choice([-1, 1], nn)
        if extremes and want in ("inside", "exact"):
            at = rng.choice(nn - 1, 2, replace=False)          # (not the far corner's level: it stays what it is)
            s[at[0]], s[at[1]] = 32767, -32767
        lv = np.zeros(nn, np.int16)
        lv[scan] = np.clip(s, -32767, 32767)
        lv = lv.reshape(n, n)
        if want == "inside" and "budget_ends_inside" not in walk(lv, n):
            continue
        if want == "exact" and "budget_ends_at_group_end" not in walk(lv, n):
            continue
        return lv
    raise AssertionError((n, want))


RICE_CLASSES = [(rice, side) for rice in range(4) for side in ("below", "above")]


def craft_rice(rng, n, kind, targets):
    """n x n levels that show the classes (kind, rice, side) of `targets`: a target is the first position of a 4x4 group with ONE level
    in its template, the one to its right, which alone sets the template's sum and so the Rice parameter (the template of a group's
    first position stays inside the group).  kind "remainder": nothing else in the block, every position is context-coded; the Rice
    parameter is that of sum - 20.  kind "bypass": the upper half of the scan is full of +-2 (four regular bins each, 1.75 a position
    is the budget), so the lower half, where the targets are, is coded in bypass; the Rice parameter is that of the sum."""
    scan = scan_of(n)
    lv = np.zeros(n * n, np.int64)
    ng = n * n // 16
    if kind == "bypass":
        if n == 4:
            lv[[i for i in range(16) if i % 4 + i // 4 >= 3]] = 2          # (outside the template of the DC position)
        else:
            lv[scan[ng // 2 * 16:]] = 2
    assert len(targets) <= (ng if kind == "remainder" else max(1, ng // 2))
    for g, (rice, side) in enumerate(targets):
        at = int(scan[g * 16])
        edge = 5 << rice
        if kind == "remainder":          # (|level| - 4) >> 1 against 5 << rice; sum - 20 in 0..6, 7..13, 14..27, 28..
            lv[at], lv[at + 1] = 4 + 2 * (edge - 1 if side == "below" else edge + 1), (5, 30, 40, 60)[rice]
        else:                            # |level| itself (above 1 << rice) against 5 << rice; the sum in the same bands
            lv[at], lv[at + 1] = (edge - 1 if side == "below" else edge + 3), (3, 10, 20, 40)[rice]
    lv = (lv * rng.choice([-1, 1], n * n)).astype(np.int16).reshape(n, n)
    got = walk(lv, n)
    assert all((kind, rice, side) in got for rice, side in targets), (n, kind, targets)
    return lv


def recipes_of(n):
    """The blocks of a (colour, size) take these recipes in turn.  The sixteen Rice classes: one a block at 4x4, as many as there are
    groups to hold them above that (context-coded: any group; bypass-coded: the lower half of the scan)."""
    base = ["inside", "sparse", "dc", "ones"] if n == 4 else ["inside", "exact", "sparse", "dc", "sparse"]
    ng = n * n // 16
    for kind, per in (("remainder", min(8, ng)), ("bypass", min(8, max(1, ng // 2)))):
        base += [(kind, tuple(RICE_CLASSES[i:i + per])) for i in range(0, 8, per)]
    return base


@functools.lru_cache(None)
def crafted_case(depth, qp, t):
    """-> (search parameters, source planes, the oracle's hand-over with crafted levels, its SAO decisions, expected bytes, row offsets,
    models behind every CTU, {(colour class, n): {class: count}})"""
    orc = H.load_oracle()
    prm = H.search_params(W, HH, qp)
    y, u, v = H.varied_picture(W, HH, t, depth)
    s = H.oracle_search_picture(orc, depth, prm, y, u, v)
    f = H.oracle_sao_picture(orc, depth, W, HH, qp, prm.lam, (y, u, v), (s["rec_y"], s["rec_u"], s["rec_v"]), H.scu_from_cu(s["cu"], qp))
    rng = np.random.default_rng(1000 * depth + qp)
    co = s["coeff"].copy()
    seen, turn = {}, {}
    for k, c, off, stride, n in transform_blocks(s["cu"], W, HH):
        key = ("chroma" if c else "luma", n)
        i = turn.get(key, 0)
        turn[key] = i + 1
        recipes = recipes_of(n)
        r = recipes[i % len(recipes)]
        lv = craft(rng, n, r, (i // len(recipes)) % 2 == 0) if isinstance(r, str) else craft_rice(rng, n, *r)
        idx = off + np.arange(n)[:, None] * stride + np.arange(n)[None, :]
        assert s["coeff"][k][idx].any(), "a block with its cbf set has a level"
        co[k][idx] = lv
        d = seen.setdefault(key, {})
        for cl in walk(lv, n):
            d[cl] = d.get(cl, 0) + 1
    s = dict(s, coeff=co)
    want, off, after = H.oracle_encode_rows(orc, depth, prm, s, f["sao"])
    return prm, (y, u, v), s, f["sao"], want, off, after, seen


def required(n):
    """The classes a block size must show.  A 4x4 block is one group: group 0, whose sig flags are never inferred, with no group behind it
    for the budget's end to fall in front of.  Every Rice parameter with a remainder on either side of 5 << rice, at context-coded and at
    bypass-coded positions, is asked of every size."""
    need = ["budget_ends_inside", "dc_only", "far_corner", "level+32767", "level-32767", "group_all_ones"]
    need += [(kind, rice, side) for kind in ("remainder", "bypass") for rice, side in RICE_CLASSES]
    if n > 4:
        need += ["budget_ends_at_group_end", "group_never_reached", "inferred_sig"]
    return need


@pytest.mark.parametrize("depth,qp,t", CASES)
def test_crafted_handover_shows_every_class(depth, qp, t):
    """The oracle's row coder accepts the crafted hand-over (two rows of bytes), and the walk finds every class of required() in luma and
    in chroma at every block size that occurs.  The CU sizes the cases are there for occur with coded blocks: all five at 8 bit, 16x16,
    32x32 and 64x64 (four 32x32 transform units, a cbf each) at 10 bit."""
    prm, src, s, sao, want, off, after, seen = crafted_case(depth, qp, t)
    assert len(off) == 3 and 0 < off[1] < off[2] == len(want)
    cu = s["cu"]
    coded_cus = {1 << int(l2) for l2 in np.unique(cu[:, :, 1][cu[:, :, 5] != 0])}
    assert coded_cus >= ({4, 8, 16, 32, 64} if depth == 8 else {16, 32, 64}), coded_cus
    assert {n for c, n in seen if c == "luma"} >= ({4, 8, 16, 32} if depth == 8 else {16, 32}), sorted(seen)
    assert {n for c, n in seen if c == "chroma"} >= ({4, 8, 16} if depth == 8 else {16}), sorted(seen)
    for key, d in sorted(seen.items()):
        for cl in required(key[1]):
            assert d.get(cl, 0) > 0, (key, cl, sorted(d, key=str))


@pytest.mark.gpu
@pytest.mark.parametrize("depth,qp,t", CASES)
def test_crafted_levels_code_to_the_oracles_bytes(hip, depth, qp, t):
    import torch
    from uvg266_amd import api
    prm, (y, u, v), s, sao, want, off, after, seen = crafted_case(depth, qp, t)
    cl = api.ClosedLoop(api.ctu_params(W, HH, qp, lam=prm.lam), [tuple(torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (y, u, v))])
    cl.run()
    torch.cuda.synchronize()
    ry, ru, rv = (p.cpu().numpy() for p in cl.rec[0])
    got = H.search_result_from_device_layout(W, HH, ry, ru, rv, cl.cu[0].cpu().numpy().reshape(-1).view(H.SCU_NP), cl.coeff[0].cpu().numpy(),
                                             cl.models[0].cpu().numpy().view(np.uint32))
    assert np.array_equal(got["cu"], s["cu"]), "the device's partition is the oracle's: the crafted levels go where its blocks are"
    info, _ = cl.results()
    assert np.array_equal(H.sao_info_comparable(info[0]), H.sao_info_comparable(sao))
    # the crafted levels, and behind the first CTU of row 0 the models the coder leaves there on these levels (what row 1 starts from)
    cl.coeff[0].copy_(torch.from_numpy(np.ascontiguousarray(s["coeff"])).cuda())
    wc = (W + 63) // 64
    m = cl.models[0].cpu().numpy().view(np.uint32).copy()
    for cy in range((HH + 63) // 64):
        a = after[cy * wc]
        s0, s1 = a[:514].copy().view(np.uint16).astype(np.uint32), a[514:1028].copy().view(np.uint16).astype(np.uint32)
        m[cy * wc, 2] = s0 | s1 << 16
    cl.models[0].copy_(torch.from_numpy(m.view(np.int32)).cuda())
    out, nbytes = cl.encode_rows()
    torch.cuda.synchronize()
    nb = nbytes.cpu().numpy()[0]
    assert np.array_equal(np.concatenate([[0], np.cumsum(nb)]), off)
    assert np.array_equal(np.concatenate([out[0, r, :nb[r]].cpu().numpy() for r in range(len(nb))]), want)
