"""The collocated field of the temporal merge candidate (x265hip_col_field_build and what x265hip_merge_decide_col /
x265hip_b_merge_decide_col read of it), on the CPU.

The candidate lists and the walks in coding order are those of tests/merge_expect.py and tests/bmerge_expect.py, which take the
candidate from here: walk(..., col=a ColSource, cur_delta / cur_deltas, tmvp_mutation) calls temporal_vectors() per block.  This module
restates, from the reference's statements (line numbers beside each), where the candidate comes from: the bottom-right position with its
picture and CTU conditions and the centre fallback (common/cudata.cpp:1594-1650), getColMVP (:1968-2000) on a field of one entry per
16x16 unit (TMVP_UNIT_MASK), scaleMvByPOCDist (:2030-2045) and scaleMv (:104-110).  getInterMergeCandidates / getColMVP are methods of
CUData that need the encoder's CU tree: with what oracle/ offers they cannot be pinned against compiled reference code.  They are pinned
by hand-worked cases written out from the statements (tests/test_tmvp_cpu.py) and by the mutations below.

A collocated field is a ColSource: one (packed vector, POC distance) per 8x8 cell of the collocated picture; distance 0 = intra.  The
device sees its unit field (the upper-left cell of every 16x16 unit); the cells in between are read by the `no_unit_mask` mutation only."""
import numpy as np

import intra_expect as IE
import intra_inter_expect as IX

pack = IX.pack_mv

P_MASKS = ("temporal_present", "won_temporal", "temporal_scaled", "rb_in_ctu", "rb_in_right_ctu", "rb_absent_last_ctu_row", "rb_outside_picture",
           "centre_after_rb_failed", "temporal_absent", "temporal_equals_spatial_kept", "temporal_cut_at_max", "temporal_fills_last_slot",
           "inherits_temporal")
B_MASKS = P_MASKS + ("won_temporal_bi", "combined_from_temporal", "won_combined_from_temporal")
P_MUTATIONS = ("temporal_before_b2", "temporal_pruned_against_a1", "centre_first", "rb_below_ctu_allowed", "rb_from_this_ctu", "no_unit_mask",
               "no_scaling", "floor_division", "no_negative_rounding", "zero_fill_after_full")
# (`floor_division` needs a negative col_delta, which the B cases - a col_delta of 4 - do not have)
B_MUTATIONS = tuple(m for m in P_MUTATIONS if m != "floor_division") + ("one_scale_both_lists", "temporal_not_in_cutoff")


def unpack(v):
    s16 = lambda x: (x & 0xffff) - ((x & 0x8000) << 1)
    return s16(int(v)), s16(int(v) >> 16)


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


def temporal_vectors(col, level, x0, y0, deltas, masks, b, mutation=None):
    """The temporal candidate of block b, whose first sample is (x0, y0): the collocated vector scaled for each POC distance of `deltas`
    (:1998; one per list - for a B slice here m_bCheckLDC and m_colFromL0Flag are false, dpb.cpp:193-195: both lists read list 0 of the
    collocated picture, so the availability falls out equal for both), or None where col is None or has no motion there.  Records the
    position masks of the block."""
    if col is None:
        return None
    cmv, cd, kind, took_centre = collocated(col, level, x0, y0, mutation)                     # :1627-1641
    masks[kind][b] = True
    masks["centre_after_rb_failed"][b] = took_centre
    masks["temporal_absent"][b] = cmv is None
    if cmv is None:
        return None
    masks["temporal_scaled"][b] = any(d != cd for d in deltas)
    return [scale_mv(cmv, deltas[0] if mutation == "one_scale_both_lists" else d, cd, mutation) for d in deltas]


def _grid(w64, h64, level):
    n = 8 << level
    bpc = 64 // n
    cw, chh = w64 // 64, h64 // 64
    return n, bpc, bpc * bpc, cw, chh


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
