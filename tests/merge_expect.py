"""Expected results of the merge stage of a P picture (x265hip_merge_decide) and of stages.MergePFramePipeline, on the CPU.

From the oracle's pieces, as intra_inter_expect.inter_side obtains them: the luma prediction through oracle_api.pred_capture of the bi
stage with every block on list 0, run on the CLIPPED vectors, its sa8d through the table's cu[].sa8d slot, the coding through
O.inter_recon / O.inter_recon_chroma on mv_pred, the boundary strengths through O.deblock_bs_inter on mv_out.

Restated here in Python, with the reference's line numbers beside each statement: the candidate list
(CUData::getInterMergeCandidates, common/cudata.cpp:1458-1712, P slice, one reference, no temporal candidate), CUData::clipMv
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

O, F, H, harness, SC = IE.O, IE.F, IE.H, IE.harness, IE.SC

MASKS = ("merge_won", "inter_won", "tie_stays_merge", "tie_lowest_index", "won_A1", "won_B1", "won_B0", "won_A0", "won_B2", "won_zero",
         "pruned_B1", "pruned_B0", "pruned_A0", "pruned_B2", "B0_equals_A1_kept", "B2_dropped_at_four", "cut_at_max", "inherits_inherited",
         "A0_from_left_ctu", "B0_from_above_right_ctu", "B0_not_yet_coded", "A0_not_yet_coded", "A0_below_ctu", "clip_changed_prediction")
MUTATIONS = ("le_against_inter", "le_among_candidates", "prune_every_pair", "b2_regardless_of_count", "searched_not_final", "no_clip",
             "clip_stored", "available_by_position", "tu_bits_without_saving")
NEIGHBOURS = (("A1", -1, 0), ("B1", 0, -1), ("B0", 1, -1), ("A0", -1, 1), ("B2", -1, -1))


def unpack(v):
    s16 = lambda x: (x & 0xffff) - ((x & 0x8000) << 1)
    return s16(int(v)), s16(int(v) >> 16)


pack = IX.pack_mv


def clip_mv(v, x0, y0, width, height, ctu=64):
    """CUData::clipMv (cudata.cpp:1915-1928) for a CU whose first sample is (x0, y0)."""
    qx, qy = unpack(v)
    xmax, xmin = (width + 8 - x0 - 1) << 2, -((ctu + 8 + x0 - 1) << 2)                        # :1920-1921
    ymax, ymin = (height + 8 - y0 - 1) << 2, -((ctu + 8 + y0 - 1) << 2)                       # :1923-1924
    return pack(min(xmax, max(xmin, qx)), min(ymax, max(ymin, qy)))                           # :1926-1927


def tu_bits(i, num, mutation=None):
    """getTUBits (search.h:246-249): a truncated unary index, the last one saves its terminating bit."""
    return i + (1 if (i < num - 1 or mutation == "tu_bits_without_saving") else 0)


def candidate_list(nb, max_merge, mutation=None):
    """getInterMergeCandidates for a P slice with one reference and no temporal candidate.  nb: {"A1" | "B1" | "B0" | "A0" | "B2": packed
    motion, or None where the neighbour is not available}.  Returns (list of (motion, origin)), flags) - origin is the neighbour's name
    or "zero"; with one reference hasEqualMotion is equality of the vectors."""
    a1, b1, b0, a0, b2 = (nb.get(k) for k in ("A1", "B1", "B0", "A0", "B2"))
    every = mutation == "prune_every_pair"
    out, fl = [], {k: False for k in ("pruned_B1", "pruned_B0", "pruned_A0", "pruned_B2", "B0_equals_A1_kept", "B2_dropped_at_four", "cut_at_max")}

    def seen(v):
        return every and any(v == m for m, _ in out)

    def cut(later):
        fl["cut_at_max"] = any(v is not None for v in later)
        return out, fl
    if a1 is not None:                                                                        # :1495-1510
        out.append((a1, "A1"))
        if len(out) == max_merge:
            return cut((b1, b0, a0, b2))
    if b1 is not None:                                                                        # :1517-1532
        if (a1 is not None and a1 == b1) or seen(b1):
            fl["pruned_B1"] = True
        else:
            out.append((b1, "B1"))
            if len(out) == max_merge:
                return cut((b0, a0, b2))
    if b0 is not None:                                                                        # :1537-1551: against B1 only
        if (b1 is not None and b1 == b0) or seen(b0):
            fl["pruned_B0"] = True
        else:
            fl["B0_equals_A1_kept"] = a1 is not None and a1 == b0
            out.append((b0, "B0"))
            if len(out) == max_merge:
                return cut((a0, b2))
    if a0 is not None:                                                                        # :1556-1570: against A1 only
        if (a1 is not None and a1 == a0) or seen(a0):
            fl["pruned_A0"] = True
        else:
            out.append((a0, "A0"))
            if len(out) == max_merge:
                return cut((b2,))
    if len(out) < 4 or mutation == "b2_regardless_of_count":                                  # :1573
        if b2 is not None:                                                                    # :1577-1592: against A1 and B1
            if (a1 is not None and a1 == b2) or (b1 is not None and b1 == b2) or seen(b2):
                fl["pruned_B2"] = True
            else:
                out.append((b2, "B2"))
                if len(out) == max_merge:
                    return out, fl
    elif b2 is not None:
        fl["B2_dropped_at_four"] = True
    while len(out) < max_merge:                                                               # :1676-1710: zero vectors, refIdx 0 (one reference)
        out.append((0, "zero"))
    return out, fl


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


def walk(w64, h64, level, searched, max_merge, price, lam, inter_cost=None, cost_fn=None, mutation=None):
    """The walk in coding order.  searched: packed vector per block (index = ctu * blocks + z); price(block, packed clipped vector) ->
    sa8d; lam(block) -> lambda8; inter_cost: int per block, or cost_fn(block, merge cost) -> the inter cost to decide against.  Returns
    merge, merge_idx (uint8), mv_out, mv_pred (packed int32 per block), cost / best int32 [blocks, 2], inter_cost (what was decided
    against) and the masks."""
    assert mutation is None or mutation in MUTATIONS
    n = 8 << level
    bpc = 64 // n
    nblk = bpc * bpc
    cw, chh = w64 // 64, h64 // 64
    tot = cw * chh * nblk
    bw, bh = cw * bpc, chh * bpc
    final = np.zeros(tot, np.int64)
    merge, idx = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    mv_out, mv_pred = np.zeros(tot, np.int32), np.zeros(tot, np.int32)
    cost, best, ic_used = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32), np.zeros(tot, np.int64)
    masks = {k: np.zeros(tot, bool) for k in MASKS}

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
            if not (0 <= nx < bw and 0 <= ny < bh):                                           # getPU*: outside the picture
                continue
            q = index(nx, ny)
            where[name] = q
            if q < b:                                                                         # already coded (CTUs in raster order, z-order inside)
                nb[name] = int(searched[q]) if mutation == "searched_not_final" else int(final[q])
            elif mutation == "available_by_position":
                nb[name] = int(searched[q])                                                   # what a block that is not yet decided holds
            elif name in ("B0", "A0"):
                below = name == "A0" and by + 1 == bpc
                masks["A0_below_ctu" if below else name + "_not_yet_coded"][b] = True
        masks["A0_from_left_ctu"][b] = nb["A0"] is not None and bx == 0 and mutation is None
        masks["B0_from_above_right_ctu"][b] = nb["B0"] is not None and bx + 1 == bpc and by == 0 and mutation is None
        cands, fl = candidate_list(nb, max_merge, mutation)
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
        masks["inherits_inherited"][b] = origin != "zero" and where[origin] < b and bool(merge[where[origin]])
        masks["clip_changed_prediction"][b] = clip_mv(v, x0, y0, w64, h64) != v
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
                      mutation=None, pricer=None):
    """What x265hip_merge_decide leaves for the searched records mv (int32 [ctu*85, 2]).  Returns walk()'s dictionary with mv_out / mv_pred
    as RECORDS of the level's slots (the cost word the input's for an inter block, the merge cost for a merged one)."""
    pr = pricer or Pricer(depth, cur_y, ref_y, w64, h64, level)
    nctu = (w64 // 64) * (h64 // 64)
    sl = level_slots(level, nctu)
    searched = np.asarray(mv).reshape(-1, 2)[sl, 1]

    def lam(b):
        gx, gy = pr.position(b)
        return IX.block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
    e = pr.fixpoint(lambda price: walk(w64, h64, level, searched, max_merge, price, lam, inter_cost=inter_cost, cost_fn=cost_fn, mutation=mutation))
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
            cores=0, tu_qp=None, cu_qp=None, lambda8_by_qp=None):
    """One P picture with merge blocks through the oracle, stage by stage (the CPU twin of stages.MergePFramePipeline.run with chroma,
    deblocking and SAO applied; tu_qp / cu_qp / lambda8_by_qp: what set_qp_maps hands on).  Every stage output by name."""
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
    e = stage_expectation(depth, y, r, w64, h64, level, mv, max_merge, lambda8, inter_cost=it["inter_cost"][:, 1], tu_qp=tu_qp, lambda8_by_qp=lambda8_by_qp, qp=qp)
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
