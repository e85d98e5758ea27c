"""Expected results of the merge stage of a P picture (x265hip_merge_decide) and of stages.MergePFramePipeline, on the CPU.

From the oracle's pieces, as intra_inter_expect.inter_side obtains them: the luma prediction through oracle_api.pred_capture of the bi
stage with every block on list 0, run on the CLIPPED vectors, its sa8d through the table's cu[].sa8d slot, the coding through
O.inter_recon / O.inter_recon_chroma on mv_pred, the boundary strengths through O.deblock_bs_inter on mv_out.

Restated here in Python, with the reference's line numbers beside each statement: the candidate list
(CUData::getInterMergeCandidates, common/cudata.cpp:1458-1712, P slice, one reference; its spatial and temporal part,
spatial_candidates(), serves tests/bmerge_expect.py as well, the temporal candidate itself comes from tests/tmvp_expect.py), CUData::clipMv
(cudata.cpp:1915-1928), getTUBits (search.h:246-249), the two strict comparisons (analysis.cpp:2833 among the candidates, :1650 against
the inter candidate) and the walk in coding order.  The candidate list cannot be pinned against compiled reference code with what
oracle/ offers: getInterMergeCandidates is a method of CUData that reads the encoder's CU tree, and the reference build exports
primitives and a few free functions, not that.  Its restatement is therefore checked by hand-worked lists written out from the
statements of cudata.cpp (tests/test_merge_cpu.py) and by the mutations below, each of which must change the expectation of some case.
clipMv is also pinned against the compiled reference where oracle/_ref is built: reference_prediction() hands the UNCLIPPED mv_out
records to x265ref_motion_compensation (oracle/ref_predict.cpp: the real Predict::motionCompensation per 2Nx2N CU, which calls
CUData::clipMv, predict.cpp:92), and its picture must equal the oracle's prediction of the clipped mv_pred records.

A block's motion is one packed word qx | qy << 16, as in the records."""
import numpy as np

import intra_expect as IE
import intra_inter_expect as IX
import tmvp_expect as TX

O, F, H, harness, SC = IE.O, IE.F, IE.H, IE.harness, IE.SC

MASKS = ("merge_won", "inter_won", "tie_stays_merge", "tie_lowest_index", "won_A1", "won_B1", "won_B0", "won_A0", "won_B2", "won_zero",
         "pruned_B1", "pruned_B0", "pruned_A0", "pruned_B2", "B0_equals_A1_kept", "B2_dropped_at_four", "cut_at_max", "inherits_inherited",
         "A0_from_left_ctu", "B0_from_above_right_ctu", "B0_not_yet_coded", "A0_not_yet_coded", "A0_below_ctu", "clip_changed_prediction")
MUTATIONS = ("le_against_inter", "le_among_candidates", "prune_every_pair", "b2_regardless_of_count", "searched_not_final", "no_clip",
             "clip_stored", "available_by_position", "tu_bits_without_saving")
NEIGHBOURS = (("A1", -1, 0), ("B1", 0, -1), ("B0", 1, -1), ("A0", -1, 1), ("B2", -1, -1))


unpack, pack = TX.unpack, TX.pack


def clip_mv(v, x0, y0, width, height, ctu=64):
    """CUData::clipMv (cudata.cpp:1915-1928) for a CU whose first sample is (x0, y0)."""
    qx, qy = unpack(v)
    xmax, xmin = (width + 8 - x0 - 1) << 2, -((ctu + 8 + x0 - 1) << 2)                        # :1920-1921
    ymax, ymin = (height + 8 - y0 - 1) << 2, -((ctu + 8 + y0 - 1) << 2)                       # :1923-1924
    return pack(min(xmax, max(xmin, qx)), min(ymax, max(ymin, qy)))                           # :1926-1927


def tu_bits(i, num, mutation=None):
    """getTUBits (search.h:246-249): a truncated unary index, the last one saves its terminating bit."""
    return i + (1 if (i < num - 1 or mutation == "tu_bits_without_saving") else 0)


SPATIAL_FLAGS = ("pruned_B1", "pruned_B0", "pruned_A0", "pruned_B2", "B0_equals_A1_kept", "B2_dropped_at_four", "cut_at_max")
TEMPORAL_FLAGS = ("temporal_present", "temporal_equals_spatial_kept", "temporal_cut_at_max", "temporal_fills_last_slot")


def spatial_candidates(nb, max_merge, equal, zero, temporal=None, mutation=None):
    """The spatial and the temporal candidates of getInterMergeCandidates (cudata.cpp:1495-1650) with every return at count ==
    maxNumMergeCand, for a P and a B slice alike.  nb: {"A1" | "B1" | "B0" | "A0" | "B2": a motion, or None where the neighbour is not
    available}; equal(p, q, record=True): p.hasEqualMotion(q) - with record it is a pruning decision (the caller may note why and may
    mutate it), without it the reference's plain comparison; zero: the slice's zero candidate; temporal: the scaled collocated motion or
    None.  Returns ([(motion, origin)], flags, whether the list was returned full) - origin is the neighbour's name or "temporal"."""
    a1, b1, b0, a0, b2 = (nb.get(k) for k in ("A1", "B1", "B0", "A0", "B2"))
    out, fl = [], {k: False for k in SPATIAL_FLAGS + TEMPORAL_FLAGS}

    def pruned(v, name, *against):
        hit = any(p is not None and equal(p, v) for p in against) or (mutation == "prune_every_pair" and any(v == m for m, _ in out))
        fl["pruned_" + name] |= hit
        return hit

    def full(later=()):
        if len(out) < max_merge:
            return False
        fl["cut_at_max"] = any(v is not None for v in later)
        fl["temporal_cut_at_max"] = temporal is not None and not fl["temporal_present"]
        return True
    if a1 is not None:                                                                        # :1495-1510
        out.append((a1, "A1"))
        if full((b1, b0, a0, b2)):
            return out, fl, True
    if b1 is not None and not pruned(b1, "B1", a1):                                           # :1517-1532
        out.append((b1, "B1"))
        if full((b0, a0, b2)):
            return out, fl, True
    if b0 is not None and not pruned(b0, "B0", b1):                                           # :1537-1551: against B1 only
        fl["B0_equals_A1_kept"] = a1 is not None and equal(a1, b0, False)
        out.append((b0, "B0"))
        if full((a0, b2)):
            return out, fl, True
    if a0 is not None and not pruned(a0, "A0", a1):                                           # :1556-1570: against A1 only
        out.append((a0, "A0"))
        if full((b2,)):
            return out, fl, True
    if mutation == "temporal_before_b2" and temporal is not None:
        fl["temporal_present"] = True
        out.append((temporal, "temporal"))
        if full():
            return out, fl, True
    if len(out) < 4 or mutation == "b2_regardless_of_count":                                  # :1573
        if b2 is not None and not pruned(b2, "B2", a1, b1):                                   # :1577-1592: against A1 and B1
            out.append((b2, "B2"))
            if full():
                return out, fl, True
    elif b2 is not None:
        fl["B2_dropped_at_four"] = True
    if temporal is not None and mutation != "temporal_before_b2" and not (mutation == "temporal_pruned_against_a1" and a1 is not None and
                                                                          equal(a1, temporal, False)):   # :1594-1650
        fl["temporal_present"] = True
        fl["temporal_equals_spatial_kept"] = any(equal(m, temporal, False) and equal(temporal, m, False) for m, _ in out)
        out.append((temporal, "temporal"))                                                    # :1643-1645: no pruning
        if len(out) == max_merge:                                                             # :1647-1648
            fl["temporal_fills_last_slot"] = True
            if mutation == "zero_fill_after_full":
                out[-1] = (zero, "zero")                        # a fill that runs once more writes over the last slot
            return out, fl, True
    return out, fl, False


def candidate_list(nb, max_merge, mutation=None, temporal=None):
    """getInterMergeCandidates for a P slice with one reference.  nb: {"A1" | "B1" | "B0" | "A0" | "B2": packed motion, or None where the
    neighbour is not available}; temporal: the scaled packed vector getColMVP gives, or None.  Returns ([(motion, origin)], flags) -
    origin is the neighbour's name, "temporal" or "zero"; with one reference hasEqualMotion is equality of the vectors."""
    out, fl, _ = spatial_candidates(nb, max_merge, lambda p, q, record=True: p == q, 0, temporal, mutation)
    while len(out) < max_merge:                                                               # :1676-1710: zero vectors, refIdx 0 (one reference)
        out.append((0, "zero"))
    return out, fl


class Grid:
    """The blocks of a picture in coding order (CTUs in raster order, z-order inside) and a block's five neighbours: what the walks of a P
    and of a B slice share."""

    def __init__(self, w64, h64, level):
        self.n, self.bpc, self.nblk, self.cw, self.chh = TX._grid(w64, h64, level)
        self.tot = self.cw * self.chh * self.nblk

    def index(self, gbx, gby):
        return ((gby // self.bpc) * self.cw + gbx // self.bpc) * self.nblk + IE.zindex(gbx % self.bpc, gby % self.bpc)

    def block(self, b):
        """(bx, by) inside the CTU and (x0, y0), the first sample."""
        ctu, z = divmod(b, self.nblk)
        bx, by = IE.zorder(z)
        return bx, by, ((ctu % self.cw) * self.bpc + bx) * self.n, ((ctu // self.cw) * self.bpc + by) * self.n

    def neighbours(self, b, coded, masks, uncoded=None, border_masks=True):
        """(nb, where) of block b: nb[name] = coded(q) for a neighbour q inside the picture and coded before b, else None (or uncoded(q),
        what the `available_by_position` mutation reads); where[name] = q for every neighbour inside the picture."""
        bx, by, x0, y0 = self.block(b)
        nb, where = {}, {}
        for name, dx, dy in NEIGHBOURS:
            nx, ny = x0 // self.n + dx, y0 // self.n + dy
            nb[name] = None
            if not (0 <= nx < self.cw * self.bpc and 0 <= ny < self.chh * self.bpc):          # getPU*: outside the picture
                continue
            q = where[name] = self.index(nx, ny)
            if q < b:                                                                         # already coded
                nb[name] = coded(q)
            elif uncoded is not None:
                nb[name] = uncoded(q)
            elif name in ("B0", "A0"):
                below = name == "A0" and by + 1 == self.bpc
                masks["A0_below_ctu" if below else name + "_not_yet_coded"][b] = True
        masks["A0_from_left_ctu"][b] = nb["A0"] is not None and bx == 0 and border_masks
        masks["B0_from_above_right_ctu"][b] = nb["B0"] is not None and bx + 1 == self.bpc and by == 0 and border_masks
        return nb, where


class Pricer:
    """cu[].sa8d(fenc, predInterLumaPixel(fref, mv)) of (block, vector) pairs through the oracle: the prediction of one vector per block
    per O.inter_recon_bi call (pred_capture), the sa8d through the table's slot.  price() answers from the cache; a miss is recorded and
    answered with 0 - fixpoint() evaluates the misses and repeats the walk until it met none."""

    def __init__(self, depth, cur_y, ref_y, w64, h64, level):
        self.depth, self.w64, self.h64, self.level = depth, w64, h64, level
        self.n = 8 << level
        self.nblk = (64 // self.n) ** 2
        self.cw = w64 // 64
        self.nctu = self.cw * (h64 // 64)
        _, _, self.stride, self.rows, self.org = F.padded_dims(w64, h64)
        self.y, self.r = np.ascontiguousarray(cur_y).reshape(-1), np.ascontiguousarray(ref_y).reshape(-1)
        self.slots = IE.Slots(depth, self.n, with_reference=False)
        self.cache, self.missing = {}, set()

    def position(self, b):
        ctu, z = divmod(b, self.nblk)
        bx, by = IE.zorder(z)
        return (ctu % self.cw) * 64 + bx * self.n, (ctu // self.cw) * 64 + by * self.n

    def price(self, b, v):
        if (b, v) in self.cache:
            return self.cache[(b, v)]
        self.missing.add((b, v))
        return 0

    def evaluate(self):
        lbase = (0, 64, 80)[self.level]
        todo = {}
        for b, v in sorted(self.missing):
            todo.setdefault(b, []).append(v)
        self.missing = set()
        layer = 0
        while any(len(vs) > layer for vs in todo.values()):
            mv = np.zeros((self.nctu * 85, 2), np.int32)
            for b, vs in todo.items():
                if len(vs) > layer:
                    mv[(b // self.nblk) * 85 + lbase + b % self.nblk, 1] = vs[layer]
            cap = np.zeros((self.h64, self.w64), self.y.dtype)
            with O.pred_capture(self.depth, cap):
                O.inter_recon_bi(self.depth, self.y, self.stride, self.org, self.r, self.r, self.w64, self.h64, self.level, mv, mv, 30,
                                 dir_flags=np.ones(self.nctu * self.nblk, np.uint8))
            for b, vs in todo.items():
                if len(vs) > layer:
                    gx, gy = self.position(b)
                    p = np.ascontiguousarray(cap[gy:gy + self.n, gx:gx + self.n])
                    self.cache[(b, vs[layer])] = self.slots.cost(self.y.ctypes.data + (self.org + gy * self.stride + gx) * self.y.itemsize, self.stride, p)
            layer += 1

    def fixpoint(self, fn, limit=400):
        for _ in range(limit):
            out = fn(self.price)
            if not self.missing:
                return out
            self.evaluate()
        raise AssertionError("the walk did not settle")


def walk(w64, h64, level, searched, max_merge, price, lam, inter_cost=None, cost_fn=None, mutation=None, col=None, cur_delta=None, tmvp_mutation=None):
    """The walk in coding order.  searched: packed vector per block (index = ctu * blocks + z); price(block, packed clipped vector) ->
    sa8d; lam(block) -> lambda8; inter_cost: int per block, or cost_fn(block, merge cost) -> the inter cost to decide against; col: a
    TX.ColSource - the list then has the temporal candidate - with cur_delta = curPOC - refPOC; tmvp_mutation: one of TX.P_MUTATIONS.
    Returns merge, merge_idx (uint8), mv_out, mv_pred (packed int32 per block), cost / best int32 [blocks, 2], inter_cost (what was
    decided against) and the masks: MASKS, and TX.P_MASKS as well where the walk is told of a collocated picture (col or cur_delta)."""
    assert mutation is None or (mutation in MUTATIONS and tmvp_mutation is None)
    assert tmvp_mutation is None or tmvp_mutation in TX.P_MUTATIONS
    g = Grid(w64, h64, level)
    tot = g.tot
    final = np.zeros(tot, np.int64)
    from_temporal = np.zeros(tot, bool)                       # the block's motion came from a temporal candidate, directly or inherited
    merge, idx = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    mv_out, mv_pred = np.zeros(tot, np.int32), np.zeros(tot, np.int32)
    cost, best, ic_used = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32), np.zeros(tot, np.int64)
    masks = {k: np.zeros(tot, bool) for k in MASKS + TX.P_MASKS}
    coded = lambda q: int(searched[q]) if mutation == "searched_not_final" else int(final[q])
    uncoded = (lambda q: int(searched[q])) if mutation == "available_by_position" else None     # what a block that is not yet decided holds
    for b in range(tot):
        _, _, x0, y0 = g.block(b)
        nb, where = g.neighbours(b, coded, masks, uncoded, mutation is None)
        temporal = TX.temporal_vectors(col, level, x0, y0, (cur_delta,), masks, b, tmvp_mutation)
        cands, fl = candidate_list(nb, max_merge, mutation or tmvp_mutation, temporal and temporal[0])
        for k, v in fl.items():
            masks[k][b] = v
        lam8 = lam(b)
        top, priced = None, []
        for i, (v, origin) in enumerate(cands):
            cl = v if mutation == "no_clip" else clip_mv(v, x0, y0, w64, h64)
            sad = price(b, cl)
            c = sad + ((tu_bits(i, len(cands), mutation) * lam8 + 128) >> 8)                   # calcRdSADCost, rdcost.h:148-153
            priced.append(c)
            if top is None or (c <= top[0] if mutation == "le_among_candidates" else c < top[0]):   # analysis.cpp:2833
                top = (c, sad, i, v, cl, origin)
        c, sad, i, v, cl, origin = top
        ties = priced.count(c) - 1
        cost[b] = (sad, c)
        ic = int(cost_fn(b, c)) if cost_fn is not None else int(inter_cost[b])
        ic_used[b] = ic
        inter = ic <= c if mutation == "le_against_inter" else ic < c                          # analysis.cpp:1650
        masks["tie_stays_merge"][b] = ic == c
        if inter:
            final[b] = int(searched[b])
            mv_out[b] = mv_pred[b] = int(searched[b])
            best[b] = (-1, ic)
            masks["inter_won"][b] = True
            continue
        merge[b], idx[b] = 1, i
        final[b] = cl if mutation == "clip_stored" else v
        mv_out[b], mv_pred[b] = final[b], cl
        best[b] = (sad, c)
        masks["merge_won"][b] = True
        masks["tie_lowest_index"][b] = ties > 0
        masks["won_" + origin][b] = True
        spatial = origin in where and where[origin] < b
        masks["inherits_inherited"][b] = spatial and bool(merge[where[origin]])
        masks["inherits_temporal"][b] = spatial and bool(from_temporal[where[origin]])
        from_temporal[b] = origin == "temporal" or masks["inherits_temporal"][b]
        masks["clip_changed_prediction"][b] = clip_mv(v, x0, y0, w64, h64) != v
    if col is None and cur_delta is None:
        masks = {k: masks[k] for k in MASKS}
    return dict(merge=merge, merge_idx=idx, mv_out=mv_out, mv_pred=mv_pred, cost=cost, best=best, inter_cost=ic_used, masks=masks)


def records(packed, cost_words, level, nctu, base=None):
    """int32 [nctu * 85, 2] records with {cost word, packed vector} at the level's slots; the other slots from `base` (or zero)."""
    nblk = 64 >> (2 * level)
    lbase = (0, 64, 80)[level]
    mv = np.zeros((nctu * 85, 2), np.int32) if base is None else np.array(base, np.int32).reshape(-1, 2).copy()
    sl = (np.arange(len(packed)) // nblk) * 85 + lbase + np.arange(len(packed)) % nblk
    mv[sl, 0], mv[sl, 1] = cost_words, packed
    return mv


def level_slots(level, nctu):
    nblk = 64 >> (2 * level)
    b = np.arange(nctu * nblk)
    return (b // nblk) * 85 + (0, 64, 80)[level] + b % nblk


def stage_expectation(depth, cur_y, ref_y, w64, h64, level, mv, max_merge, lambda8, inter_cost=None, cost_fn=None, tu_qp=None, lambda8_by_qp=None, qp=0,
                      mutation=None, pricer=None, col=None, cur_delta=None, tmvp_mutation=None):
    """What x265hip_merge_decide (with col: x265hip_merge_decide_col) leaves for the searched records mv (int32 [ctu*85, 2]).  Returns
    walk()'s dictionary with mv_out / mv_pred as RECORDS of the level's slots (the cost word the input's for an inter block, the merge cost
    for a merged one)."""
    pr = pricer or Pricer(depth, cur_y, ref_y, w64, h64, level)
    nctu = (w64 // 64) * (h64 // 64)
    sl = level_slots(level, nctu)
    searched = np.asarray(mv).reshape(-1, 2)[sl, 1]

    def lam(b):
        gx, gy = pr.position(b)
        return IX.block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
    e = pr.fixpoint(lambda price: walk(w64, h64, level, searched, max_merge, price, lam, inter_cost=inter_cost, cost_fn=cost_fn, mutation=mutation,
                                       col=col, cur_delta=cur_delta, tmvp_mutation=tmvp_mutation))
    words = np.where(e["merge"] != 0, e["cost"][:, 1], np.asarray(mv).reshape(-1, 2)[sl, 0])
    e["vec_out"], e["vec_pred"] = e["mv_out"], e["mv_pred"]
    e["mv_out"], e["mv_pred"] = records(e["vec_out"], words, level, nctu)[sl], records(e["vec_pred"], words, level, nctu)[sl]
    return e


def tie_pattern(b, merge_cost):
    """The supplied inter cost of the pattern cases: merge cost - 1 (inter wins), the merge cost itself (a tie: merge), + 1 (merge wins),
    by block index modulo 3."""
    return merge_cost + (b % 3) - 1


def skip_flags(merge, *num_sigs):
    """encodeResidue: a merged 2Nx2N CU without a coded coefficient becomes MODE_SKIP (analysis.cpp:3358-3359)."""
    s = np.asarray(merge) != 0
    for ns in num_sigs:
        s &= np.asarray(ns) == 0
    return s.astype(np.uint8)


def oracle_prediction(depth, cur_y, ref_y, w64, h64, level, mv):
    """The oracle's luma prediction of the picture for the records mv (pred_capture of the bi stage with every block on list 0)."""
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    y, r = np.ascontiguousarray(cur_y).reshape(-1), np.ascontiguousarray(ref_y).reshape(-1)
    nctu = (w64 // 64) * (h64 // 64)
    cap = np.zeros((h64, w64), y.dtype)
    with O.pred_capture(depth, cap):
        O.inter_recon_bi(depth, y, stride, org, r, r, w64, h64, level, mv, mv, 30, dir_flags=np.ones(nctu * (64 >> (2 * level)), np.uint8))
    return cap


def reference_prediction(lib, ref_y, w64, h64, level, mv):
    """Predict::motionCompensation of the compiled reference (lib.x265ref_motion_compensation, oracle/ref_predict.cpp) for a P picture of
    2Nx2N CUs with the records mv: the luma prediction, every vector clipped by the reference's own CUData::clipMv.  ref_y: the padded
    plane (PicYuv geometry)."""
    import ctypes
    ref_y = np.ascontiguousarray(ref_y)
    dt = ref_y.dtype
    mv = np.ascontiguousarray(mv, dtype=np.int32)
    chroma = np.zeros((h64 // 2, w64 // 2), dt)                 # the chroma planes are predicted too; nothing here reads them
    out = [np.zeros((h64, w64), dt), np.zeros((h64 // 2, w64 // 2), dt), np.zeros((h64 // 2, w64 // 2), dt)]
    weights = np.tile(np.array([0, 1, 0, 0], np.int32), (2, 3, 1))
    f = lib.x265ref_motion_compensation
    f.argtypes = [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    rc = f(ref_y.ctypes.data, chroma.ctypes.data, chroma.ctypes.data, ref_y.ctypes.data, chroma.ctypes.data, chroma.ctypes.data, w64, h64, level,
           mv.ctypes.data, None, None, 0, 0, 0, weights.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data)
    assert rc == 0, rc
    return out[0]


def p_chain(depth, cur, ref, w64, h64, rng_r, subme, level, qp, max_merge=3, sao_rdo=None, tu_flags=H.TU_SIGN_HIDE, base_bits=IX.BASE_BITS, lambda8=IE.LAMBDA8,
            cores=0, tu_qp=None, cu_qp=None, lambda8_by_qp=None, col=None, cur_delta=None):
    """One P picture with merge blocks through the oracle, stage by stage (the CPU twin of stages.MergePFramePipeline.run with chroma,
    deblocking and SAO applied; tu_qp / cu_qp / lambda8_by_qp: what set_qp_maps hands on; col / cur_delta: the handed collocated field of
    a step with temporal_mvp).  Every stage output by name."""
    S = IE.importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    nctu = (w64 // 64) * (h64 // 64)
    qpc = S.chroma_quant_qp(qp, depth)
    y, r = cur[0], ref[0]
    if tu_qp is not None:                       # the stages clamp a map's entries to the quantiser's range; the oracle runs take them as they are
        tu_qp = np.clip(tu_qp, 0, 51 + 6 * (depth - 8)).astype(np.int8)
    _, mv = SC.search_head(depth, y, r, stride, org, w64, h64, rng_r, subme, cores=cores)
    it = IX.inter_side(depth, cur, ref, w64, h64, level, mv, qp, (qpc, qpc), tu_flags, base_bits=base_bits, lambda8=lambda8, table=IX.s_bitsizes(4 * rng_r + 4),
                       tu_qp=tu_qp, lambda8_by_qp=lambda8_by_qp)
    e = stage_expectation(depth, y, r, w64, h64, level, mv, max_merge, lambda8, inter_cost=it["inter_cost"][:, 1], tu_qp=tu_qp, lambda8_by_qp=lambda8_by_qp, qp=qp,
                          col=col, cur_delta=cur_delta)
    full = lambda recs: records(recs[:, 1], recs[:, 0], level, nctu)
    mvp, mvo = full(e["mv_pred"]), full(e["mv_out"])
    cd = IX.inter_side(depth, cur, ref, w64, h64, level, mvp, qp, (qpc, qpc), tu_flags, tu_qp=tu_qp)          # the coding from mv_pred
    out = {"subpel_mv": mv, "inter_cost": it["inter_cost"], "merge": e["merge"], "merge_idx": e["merge_idx"], "merge_cost": e["cost"], "best": e["best"],
           "mv_out": e["mv_out"], "mv_pred": e["mv_pred"]}
    out.update({k: cd[k] for k in ("levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")})
    out["skip"] = skip_flags(e["merge"], cd["num_sig"], cd["num_sig_c0"], cd["num_sig_c1"])
    bv, bh = O.deblock_bs_inter(depth, w64, h64, level, mvo, cd["num_sig"])
    return SC.filter_tail(out, depth, cur, cd["recon"], [cd["recon_c0"], cd["recon_c1"]], bv, bh, qp, w64, h64, cu_qp=cu_qp, sao_rdo=sao_rdo, cores=cores)


def p_device_outputs(pipe, dt):
    """The same names from a stages.MergePFramePipeline after run() (chroma, deblocking, SAO applied)."""
    g = lambda t: t.cpu().numpy()
    sl = level_slots(pipe.md.level, pipe.nctu)
    out = SC.step_outputs(pipe, dt)
    out.update({"subpel_mv": g(pipe.sp.out).reshape(-1, 2), "inter_cost": g(pipe.ic.cost).reshape(-1, 2), "merge": g(pipe.md.merge), "merge_idx": g(pipe.md.merge_idx),
                "merge_cost": g(pipe.md.cost).reshape(-1, 2), "best": g(pipe.md.best).reshape(-1, 2), "mv_out": g(pipe.md.mv_out).reshape(-1, 2)[sl],
                "mv_pred": g(pipe.md.mv_pred).reshape(-1, 2)[sl], "skip": g(pipe.skip)})
    return out
