"""Expected results of the merge stages with the temporal candidate (x265hip_col_field_build, x265hip_merge_decide_col,
x265hip_b_merge_decide_col), on the CPU.

tests/merge_expect.py and tests/bmerge_expect.py hold the lists and walks without the temporal candidate; their walk() calls their own
candidate_list().  This module restates both lists and both walks WITH the candidate, from the reference's statements (line numbers
beside each), and reuses those modules' Pricer, clip_mv, tu_bits, has_equal_motion and chains: swapped(ME, walk) puts a restated walk in
the place of ME.walk / BM.walk for the time of a `with` block, so ME.stage_expectation / ME.p_chain / BM.stage_expectation /
BM.merge_b_chain run unchanged around it.

What is restated: the temporal candidate of CUData::getInterMergeCandidates (common/cudata.cpp:1594-1650: the bottom-right position
with its picture and CTU conditions, the centre fallback, the insertion between B2 and the combined / zero candidates, the return at
count == maxNumMergeCand), getColMVP (:1968-2000) on a field of one entry per 16x16 unit (TMVP_UNIT_MASK), scaleMvByPOCDist (:2030-2045)
and scaleMv (:104-110).  As for the lists without the candidate, getInterMergeCandidates / getColMVP are methods of CUData that need the
encoder's CU tree: with what oracle/ offers they cannot be pinned against compiled reference code.  They are pinned by hand-worked
cases written out from the statements (tests/test_tmvp_cpu.py) and by the mutations below.

A collocated field is a ColSource: one (packed vector, POC distance) per 8x8 cell of the collocated picture; distance 0 = intra.  The
device sees its unit field (the upper-left cell of every 16x16 unit); the cells in between are read by the `no_unit_mask` mutation only."""
import contextlib

import numpy as np

import bmerge_expect as BM
import intra_expect as IE
import merge_expect as ME

unpack, pack, clip_mv, tu_bits = ME.unpack, ME.pack, ME.clip_mv, ME.tu_bits
NEIGHBOURS = ME.NEIGHBOURS

P_MASKS = ("temporal_present", "won_temporal", "temporal_scaled", "rb_in_ctu", "rb_in_right_ctu", "rb_absent_last_ctu_row", "rb_outside_picture",
           "centre_after_rb_failed", "temporal_absent", "temporal_equals_spatial_kept", "temporal_cut_at_max", "temporal_fills_last_slot",
           "inherits_temporal")
B_MASKS = P_MASKS + ("won_temporal_bi", "combined_from_temporal", "won_combined_from_temporal")
P_MUTATIONS = ("temporal_before_b2", "temporal_pruned_against_a1", "centre_first", "rb_below_ctu_allowed", "rb_from_this_ctu", "no_unit_mask",
               "no_scaling", "floor_division", "no_negative_rounding", "zero_fill_after_full")
# (`floor_division` needs a negative col_delta, which the B cases - a col_delta of 4 - do not have)
B_MUTATIONS = tuple(m for m in P_MUTATIONS if m != "floor_division") + ("one_scale_both_lists", "temporal_not_in_cutoff")


def cdiv(a, b):
    """C's integer division: truncation toward zero."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip3(lo, hi, v):
    return min(hi, max(lo, v))


def scale_factor(cur_delta, col_delta, mutation=None):
    """The scale of scaleMvByPOCDist (cudata.cpp:2030-2045); None where the distances are equal and the vector is returned as it is."""
    if cur_delta == col_delta:                                                                # :2035-2036
        return None
    tdb, tdd = clip3(-128, 127, cur_delta), clip3(-128, 127, col_delta)                       # :2039-2040
    if mutation == "floor_division":
        x = (0x4000 + abs(tdd // 2)) // tdd
    else:
        x = cdiv(0x4000 + abs(cdiv(tdd, 2)), tdd)                                             # :2041
    return clip3(-4096, 4095, (tdb * x + 32) >> 6)                                            # :2042


def scale_component(v, scale, mutation=None):
    """scaleMv (cudata.cpp:104-110) of one component."""
    p = scale * v
    return clip3(-32768, 32767, (p + 127 + (1 if p < 0 and mutation != "no_negative_rounding" else 0)) >> 8)


def scale_mv(v, cur_delta, col_delta, mutation=None):
    """scaleMvByPOCDist of the packed vector v."""
    if mutation == "no_scaling":
        return int(v)
    s = scale_factor(cur_delta, col_delta, mutation)
    if s is None:
        return int(v)
    qx, qy = unpack(v)
    return pack(scale_component(qx, s, mutation), scale_component(qy, s, mutation))


class ColSource:
    """A collocated picture's motion per 8x8 cell: mv int32 [h/8, w/8] (packed) and delta int16 [h/8, w/8] (colPOC - colRefPOC; 0 = intra)."""

    def __init__(self, w64, h64, mv=None, delta=None):
        self.w64, self.h64 = w64, h64
        self.mv = np.zeros((h64 // 8, w64 // 8), np.int32) if mv is None else np.asarray(mv, np.int32)
        self.delta = np.zeros((h64 // 8, w64 // 8), np.int16) if delta is None else np.asarray(delta, np.int16)
        assert self.mv.shape == self.delta.shape == (h64 // 8, w64 // 8)

    def unit_field(self):
        """(col_mv int32 [ctu * 16], col_delta int16 [ctu * 16]): what the device is handed - units in raster order inside the CTU, the
        vector 0 where the distance is 0."""
        cw, ch = self.w64 // 64, self.h64 // 64
        mv, dl = np.zeros(cw * ch * 16, np.int32), np.zeros(cw * ch * 16, np.int16)
        for ctu in range(cw * ch):
            for u in range(16):
                gy, gx = (ctu // cw) * 8 + (u // 4) * 2, (ctu % cw) * 8 + (u % 4) * 2
                dl[ctu * 16 + u] = self.delta[gy, gx]
                mv[ctu * 16 + u] = self.mv[gy, gx] if self.delta[gy, gx] else 0
        return mv, dl

    def read(self, x, y, masked=True):
        """getColMVP's view of sample (x, y): (packed vector, distance) of its 16x16 unit (partUnitIdx & TMVP_UNIT_MASK, :1973), or None
        where that is intra (:1974-1975)."""
        gx, gy = (x >> 4 << 1, y >> 4 << 1) if masked else (x >> 3, y >> 3)
        d = int(self.delta[gy, gx])
        return (int(self.mv[gy, gx]), d) if d else None


def positions(level, w64, h64, x0, y0, mutation=None):
    """Where the temporal candidate of the N x N block at (x0, y0) looks (cudata.cpp:1596-1634): (kind, bottom-right sample or None,
    centre sample).  kind names why there is or is not a bottom-right try."""
    n = 8 << level
    lx, ly = x0 % 64, y0 % 64
    centre = (x0 + n // 2, y0 + n // 2)                                                       # deriveCenterIdx, :1632
    if not (x0 + n < w64 and y0 + n < h64):                                                   # :1601-1602
        return "rb_outside_picture", None, centre
    if ly + n >= 64 and mutation != "rb_below_ctu_allowed":                                   # bNotLastRow false: ctuIdx stays -1 (:1614-1615, :1621-1622)
        return "rb_absent_last_ctu_row", None, centre
    if lx + n >= 64:                                                                          # :1616-1620: CTU + 1, unit column 0
        if mutation == "rb_from_this_ctu":
            return "rb_in_right_ctu", (x0 - lx, y0 + n), centre
        return "rb_in_right_ctu", (x0 + n, y0 + n), centre
    return "rb_in_ctu", (x0 + n, y0 + n), centre                                              # :1609-1613


def collocated(col, level, x0, y0, mutation=None):
    """(unscaled packed vector, distance, kind, took the centre after a failed try) or (None, 0, kind, False): the bottom-right try, then
    the centre (:1629-1634)."""
    kind, rb, centre = positions(level, col.w64, col.h64, x0, y0, mutation)
    masked = mutation != "no_unit_mask"
    order = [p for p in ((centre, rb) if mutation == "centre_first" else (rb, centre)) if p is not None]
    for k, (x, y) in enumerate(order):
        if y >= col.h64:                                        # only `rb_below_ctu_allowed` gets here, in the last CTU row: nothing to read
            continue
        got = col.read(x, y, masked)
        if got is not None:
            return got[0], got[1], kind, (x, y) == centre and rb is not None and mutation != "centre_first"
    return None, 0, kind, False


def _spatial(nb, max_merge, equal, temporal, mutation, fl):
    """The spatial candidates (cudata.cpp:1495-1593) with the early returns; returns (list, returned)."""
    a1, b1, b0, a0, b2 = (nb.get(k) for k in ("A1", "B1", "B0", "A0", "B2"))
    out = []
    if a1 is not None:                                                                        # :1495-1510
        out.append((a1, "A1"))
        if len(out) == max_merge:
            return out, True
    if b1 is not None and not (a1 is not None and equal(a1, b1)):                             # :1517-1532
        out.append((b1, "B1"))
        if len(out) == max_merge:
            return out, True
    if b0 is not None and not (b1 is not None and equal(b1, b0)):                             # :1537-1551
        out.append((b0, "B0"))
        if len(out) == max_merge:
            return out, True
    if a0 is not None and not (a1 is not None and equal(a1, a0)):                             # :1556-1570
        out.append((a0, "A0"))
        if len(out) == max_merge:
            return out, True
    if mutation == "temporal_before_b2" and temporal is not None:
        out.append((temporal, "temporal"))
        fl["temporal_present"] = True
        if len(out) == max_merge:
            return out, True
    if len(out) < 4 and b2 is not None and not (a1 is not None and equal(a1, b2)) and not (b1 is not None and equal(b1, b2)):   # :1573-1593
        out.append((b2, "B2"))
        if len(out) == max_merge:
            return out, True
    return out, False


def _temporal(out, nb, max_merge, equal, temporal, mutation, fl):
    """:1594-1650 behind the spatial candidates; returns True where the list was returned."""
    if temporal is None or mutation == "temporal_before_b2":
        return False
    a1 = nb.get("A1")
    if mutation == "temporal_pruned_against_a1" and a1 is not None and equal(a1, temporal):
        return False
    fl["temporal_present"] = True
    fl["temporal_equals_spatial_kept"] = any(equal(m, temporal) and equal(temporal, m) for m, _ in out)
    out.append((temporal, "temporal"))                                                        # :1643-1645: no pruning
    if len(out) == max_merge:                                                                 # :1647-1648
        fl["temporal_fills_last_slot"] = True
        if mutation == "zero_fill_after_full":
            out[-1] = (None, "zero")                            # a fill that runs once more writes over the last slot
        return True
    return False


P_FLAGS = ("temporal_present", "temporal_equals_spatial_kept", "temporal_cut_at_max", "temporal_fills_last_slot")


def candidate_list_p(nb, max_merge, temporal=None, mutation=None):
    """getInterMergeCandidates for a P slice with one reference and temporal MVP.  nb: {"A1" | ...: packed motion or None}; temporal: the
    scaled packed vector getColMVP gives, or None.  Returns ([(motion, origin)], flags); origin "temporal" for the candidate."""
    fl = {k: False for k in P_FLAGS}
    equal = lambda p, q: p == q
    out, done = _spatial(nb, max_merge, equal, temporal, mutation, fl)
    if done:
        fl["temporal_cut_at_max"] = temporal is not None and not fl["temporal_present"]
        return out, fl
    if _temporal(out, nb, max_merge, equal, temporal, mutation, fl):
        return [(0 if m is None else m, o) for m, o in out], fl
    while len(out) < max_merge:                                                               # :1687-1709
        out.append((0, "zero"))
    return out, fl


B_FLAGS = P_FLAGS + ("combined_from_temporal",)


def candidate_list_b(nb, max_merge, temporal=None, same_picture=False, mutation=None):
    """getInterMergeCandidates for a B slice with one reference per list and temporal MVP.  nb: {"A1" | ...: BM.motion() or None};
    temporal: BM.motion(3, scaled for list 0, scaled for list 1) or None.  Origins: "temporal", "combined", "combined_temporal" (a combined
    candidate with the temporal one as a source), "zero"."""
    fl = {k: False for k in B_FLAGS}
    equal = BM.has_equal_motion
    zero = BM.motion(3, 0, 0)
    out, done = _spatial(nb, max_merge, equal, temporal, mutation, fl)
    if done:
        fl["temporal_cut_at_max"] = temporal is not None and not fl["temporal_present"]
        return out, fl
    if _temporal(out, nb, max_merge, equal, temporal, mutation, fl):
        return [(zero if m is None else m, o) for m, o in out], fl
    count = len(out)
    if mutation == "temporal_not_in_cutoff" and fl["temporal_present"]:
        count -= 1
    cutoff = count * (count - 1)                                                              # :1654: once, the temporal candidate included
    pairs = BM.combined_pairs()
    for k in range(min(cutoff, 12)):                                                          # :1658
        i, j = pairs[k]
        (ci, oi), (cj, oj) = out[i], out[j]
        if (ci[0] & 1) and (cj[0] & 2):                                                       # :1663
            if same_picture and ci[1] == cj[2]:                                               # :1670
                continue
            from_t = "temporal" in (oi, oj)
            fl["combined_from_temporal"] |= from_t
            out.append((BM.motion(3, ci[1], cj[2]), "combined_temporal" if from_t else "combined"))   # :1672-1676
            if len(out) == max_merge:                                                         # :1678-1679
                return out, fl
    while len(out) < max_merge:                                                               # :1687-1709
        out.append((zero, "zero"))
    return out, fl


def _grid(w64, h64, level):
    n = 8 << level
    bpc = 64 // n
    cw, chh = w64 // 64, h64 // 64
    return n, bpc, bpc * bpc, cw, chh


def _position_masks(masks, b, kind, took_centre, found):
    masks[kind][b] = True
    masks["centre_after_rb_failed"][b] = took_centre
    masks["temporal_absent"][b] = not found


def walk_p(w64, h64, level, searched, max_merge, price, lam, inter_cost=None, cost_fn=None, mutation=None, col=None, cur_delta=None, tmvp_mutation=None):
    """ME.walk with the temporal candidate.  col: a ColSource (None = no collocated field: ME.walk's result); cur_delta: curPOC - refPOC;
    tmvp_mutation: one of P_MUTATIONS.  Returns ME.walk's dictionary with this module's masks."""
    assert mutation is None and (tmvp_mutation is None or tmvp_mutation in P_MUTATIONS)
    mut = tmvp_mutation
    n, bpc, nblk, cw, chh = _grid(w64, h64, level)
    tot = cw * chh * nblk
    bw, bh = cw * bpc, chh * bpc
    final = np.zeros(tot, np.int64)
    from_temporal = np.zeros(tot, bool)                       # the block's motion came from a temporal candidate, directly or inherited
    merge, idx = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    mv_out, mv_pred = np.zeros(tot, np.int32), np.zeros(tot, np.int32)
    cost, best, ic_used = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32), np.zeros(tot, np.int64)
    masks = {k: np.zeros(tot, bool) for k in P_MASKS}

    def index(gbx, gby):
        return ((gby // bpc) * cw + gbx // bpc) * nblk + IE.zindex(gbx % bpc, gby % bpc)
    for b in range(tot):
        ctu, z = divmod(b, nblk)
        bx, by = IE.zorder(z)
        gbx, gby = (ctu % cw) * bpc + bx, (ctu // cw) * bpc + by
        x0, y0 = gbx * n, gby * n
        nb, where = {}, {}
        for name, dx, dy in NEIGHBOURS:
            nx, ny = gbx + dx, gby + dy
            nb[name] = None
            if 0 <= nx < bw and 0 <= ny < bh and index(nx, ny) < b:                            # inside the picture and already coded
                where[name] = index(nx, ny)
                nb[name] = int(final[where[name]])
        temporal = None
        if col is not None:
            cmv, cd, kind, took_centre = collocated(col, level, x0, y0, mut)
            _position_masks(masks, b, kind, took_centre, cmv is not None)
            if cmv is not None:
                temporal = scale_mv(cmv, cur_delta, cd, mut)                                  # :1998
                masks["temporal_scaled"][b] = cur_delta != cd
        cands, fl = candidate_list_p(nb, max_merge, temporal, mut)
        for k, v in fl.items():
            masks[k][b] = v
        lam8 = lam(b)
        top = None
        for i, (v, origin) in enumerate(cands):
            cl = clip_mv(v, x0, y0, w64, h64)
            sad = price(b, cl)
            c = sad + ((tu_bits(i, len(cands)) * lam8 + 128) >> 8)                            # calcRdSADCost, rdcost.h:148-153
            if top is None or c < top[0]:                                                     # analysis.cpp:2833
                top = (c, sad, i, v, cl, origin)
        c, sad, i, v, cl, origin = top
        cost[b] = (sad, c)
        ic = int(cost_fn(b, c)) if cost_fn is not None else int(inter_cost[b])
        ic_used[b] = ic
        if ic < c:                                                                            # analysis.cpp:1650
            final[b] = int(searched[b])
            mv_out[b] = mv_pred[b] = int(searched[b])
            best[b] = (-1, ic)
            continue
        merge[b], idx[b] = 1, i
        final[b] = v
        mv_out[b], mv_pred[b] = v, cl
        best[b] = (sad, c)
        masks["won_temporal"][b] = origin == "temporal"
        masks["inherits_temporal"][b] = origin in where and bool(from_temporal[where[origin]])
        from_temporal[b] = origin == "temporal" or masks["inherits_temporal"][b]
    return dict(merge=merge, merge_idx=idx, mv_out=mv_out, mv_pred=mv_pred, cost=cost, best=best, inter_cost=ic_used, masks=masks)


def walk_b(w64, h64, level, winners, max_merge, price, lam, inter_cost=None, cost_fn=None, same_picture=False, mutation=None, col=None, cur_deltas=None,
           tmvp_mutation=None):
    """BM.walk with the temporal candidate.  col: the ColSource of L1[0]; cur_deltas = (curPOC - POC(L0[0]), curPOC - POC(L1[0])).  For a B
    slice here m_bCheckLDC and m_colFromL0Flag are false (dpb.cpp:193-195): both lists read list 0 of the collocated picture, so the
    availability falls out equal for both and the candidate is dir 3 with the one vector scaled per list."""
    assert mutation is None and (tmvp_mutation is None or tmvp_mutation in P_MUTATIONS + B_MUTATIONS)
    mut = tmvp_mutation
    n, bpc, nblk, cw, chh = _grid(w64, h64, level)
    tot = cw * chh * nblk
    bw, bh = cw * bpc, chh * bpc
    final = [None] * tot
    from_temporal = np.zeros(tot, bool)
    merge, idx, dirs = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    vec_out, vec_pred = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32)
    cost, best, ic_used = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32), np.zeros(tot, np.int64)
    masks = {k: np.zeros(tot, bool) for k in B_MASKS}
    wrap = lambda v: int(np.int32(np.uint32(v & 0xffffffff)))

    def index(gbx, gby):
        return ((gby // bpc) * cw + gbx // bpc) * nblk + IE.zindex(gbx % bpc, gby % bpc)
    for b in range(tot):
        ctu, z = divmod(b, nblk)
        bx, by = IE.zorder(z)
        gbx, gby = (ctu % cw) * bpc + bx, (ctu // cw) * bpc + by
        x0, y0 = gbx * n, gby * n
        win = BM.motion(*winners[b])
        nb, where = {}, {}
        for name, dx, dy in NEIGHBOURS:
            nx, ny = gbx + dx, gby + dy
            nb[name] = None
            if 0 <= nx < bw and 0 <= ny < bh and index(nx, ny) < b:
                where[name] = index(nx, ny)
                nb[name] = final[where[name]]
        temporal = None
        if col is not None:
            cmv, cd, kind, took_centre = collocated(col, level, x0, y0, mut)                   # :1627-1641: per list, equal for both
            _position_masks(masks, b, kind, took_centre, cmv is not None)
            if cmv is not None:
                d1 = cur_deltas[0] if mut == "one_scale_both_lists" else cur_deltas[1]
                temporal = BM.motion(3, scale_mv(cmv, cur_deltas[0], cd, mut), scale_mv(cmv, d1, cd, mut))
                masks["temporal_scaled"][b] = cur_deltas[0] != cd or cur_deltas[1] != cd
        cands, fl = candidate_list_b(nb, max_merge, temporal, same_picture, mut)
        for k, v in fl.items():
            masks[k][b] = v
        lam8 = lam(b)
        clip = lambda v: clip_mv(v, x0, y0, w64, h64)
        top = None
        for i, (m, origin) in enumerate(cands):
            c0 = clip(m[1]) if m[0] & 1 else 0
            c1 = clip(m[2]) if m[0] & 2 else 0
            sad = price(b, m[0], c0, c1)
            c = sad + ((tu_bits(i, len(cands)) * lam8 + 128) >> 8)
            if top is None or c < top[0]:                                                     # analysis.cpp:2833
                top = (c, sad, i, m, (c0, c1), origin)
        c, sad, i, m, cl, origin = top
        cost[b] = (sad, c)
        ic = int(cost_fn(b, c)) if cost_fn is not None else int(inter_cost[b])
        ic_used[b] = ic
        if ic < c:                                                                            # analysis.cpp:1650-1655
            final[b] = win
            dirs[b] = win[0]
            vec_out[b] = (wrap(win[1]), wrap(win[2]))
            vec_pred[b] = (wrap(winners[b][1]), wrap(winners[b][2]))                           # the input records, untouched
            best[b] = (-1, ic)
            continue
        merge[b], idx[b], dirs[b] = 1, i, m[0]
        final[b] = BM.motion(m[0], m[1], m[2])
        vec_out[b] = (wrap(final[b][1]), wrap(final[b][2]))
        vec_pred[b] = (wrap(cl[0]), wrap(cl[1]))
        best[b] = (sad, c)
        masks["won_temporal"][b] = masks["won_temporal_bi"][b] = origin == "temporal"
        masks["won_combined_from_temporal"][b] = origin == "combined_temporal"
        masks["inherits_temporal"][b] = origin in where and bool(from_temporal[where[origin]])
        from_temporal[b] = origin in ("temporal", "combined_temporal") or masks["inherits_temporal"][b]
    used = np.stack([(dirs & 1) != 0, (dirs & 2) != 0], axis=1)
    return dict(merge=merge, merge_idx=idx, dir=dirs, ref_used=used, vec_out=vec_out, vec_pred=vec_pred, cost=cost, best=best, inter_cost=ic_used, masks=masks)


@contextlib.contextmanager
def swapped(module, walk):
    """module.walk = walk inside the block: module.stage_expectation and the chains that call it then run the restated walk."""
    old = module.walk
    module.walk = walk
    try:
        yield
    finally:
        module.walk = old


def compress(level, w64, h64, mv, poc_delta, intra=None, ref_idx=None):
    """x265hip_col_field_build restated: mv int32 [ctu * 85, 2] records, poc_delta one int or a sequence per reference index, intra uint8 /
    ref_idx int8 [ctu * blocks] or None.  Unit (ux, uy) takes the motion of the block that covers sample (16 ux, 16 uy).  Returns
    (col_mv int32 [ctu * 16], col_delta int16 [ctu * 16])."""
    n, bpc, nblk, cw, chh = _grid(w64, h64, level)
    mv = np.asarray(mv, np.int32).reshape(-1, 2)
    deltas = [int(poc_delta)] * 8 if isinstance(poc_delta, (int, np.integer)) else [int(d) for d in poc_delta]
    lbase = (0, 64, 80)[level]
    col_mv, col_delta = np.zeros(cw * chh * 16, np.int32), np.zeros(cw * chh * 16, np.int16)
    for ctu in range(cw * chh):
        for u in range(16):
            ux, uy = u % 4, u // 4
            z = IE.zindex(16 * ux // n, 16 * uy // n)
            blk = ctu * nblk + z
            if intra is not None and intra[blk]:
                continue
            r = int(ref_idx[blk]) if ref_idx is not None else 0
            if r < 0:
                continue
            col_mv[ctu * 16 + u], col_delta[ctu * 16 + u] = mv[ctu * 85 + lbase + z, 1], deltas[r]
    return col_mv, col_delta


def source_of_units(w64, h64, col_mv, col_delta):
    """The ColSource of a unit field (every cell of a unit holds the unit's entry): what a later picture reads of a field the device built."""
    cw = w64 // 64
    s = ColSource(w64, h64)
    for i in range(len(col_mv)):
        ctu, u = divmod(i, 16)
        gy, gx = (ctu // cw) * 8 + (u // 4) * 2, (ctu % cw) * 8 + (u % 4) * 2
        s.mv[gy:gy + 2, gx:gx + 2], s.delta[gy:gy + 2, gx:gx + 2] = col_mv[i], col_delta[i]
    return s
