"""Expected results of the merge walk of a P picture with the AMVP arm (x265hip_merge_decide_amvp) and of
stages.MergePFramePipeline(amvp=True), on the CPU.

The merge side - list, clip, prices, the walk in coding order - is tests/merge_expect.py's, imported and not changed.  Restated here in
Python, with the reference's line numbers beside each statement: the predictor list (CUData::getPMV, common/cudata.cpp:1715-1807, over
the neighbours of CUData::getNeighbourMV, :1810-1865), the first choice (Search::selectMVP, encoder/search.cpp:1992-2023), the final
choice and the rate (Search::checkBestMVP, :2702-2713, called at :2455 after bits += bitcost(outmv); BitCost::bitcost(mv, mvp),
bitcost.h:54-58).  getPMV, selectMVP and checkBestMVP are methods of CUData / Search that need the encoder's CU tree: with what oracle/
offers they cannot be pinned against compiled reference code.  They are pinned by hand-worked cases written out from the statements
(tests/test_amvp_cpu.py) and by the mutations below, each of which must change the expectation of some case.

Scope: one P slice with one reference, every block a 2Nx2N inter CU with refIdx 0.  getDirectPMV (cudata.cpp:1931-1944) is then true
exactly where the neighbour is available and getIndirectPMV never decides anything; with several references the POC comparison of
getDirectPMV and the scaled indirect candidates would have to be modelled.  m_bFrameParallel is false (selectMVP :2005-2016 is skipped).

The boundary: in the reference the search itself runs around amvp[selectMVP] and charges mv - mvp while it searches; here the searched
vector is an input.  What is modelled is everything after motionEstimate returns."""
import numpy as np

import intra_expect as IE
import intra_inter_expect as IX
import merge_expect as ME
import tmvp_expect as TX

pack, unpack = ME.pack, ME.unpack

LIST_MUTATIONS = ("a1_before_a0", "b1_before_b0", "b2_never", "pair_not_reduced", "temporal_although_two", "temporal_unscaled", "no_zero_fill")
MUTATIONS = LIST_MUTATIONS + ("select_lt", "select_no_clip", "select_on_sa8d", "check_le", "price_against_zero", "searched_not_final")
MASKS = ("left_A0", "left_A1", "left_absent", "above_B0", "above_B1", "above_B2", "above_absent", "pair_reduced", "amvp_temporal_taken",
         "amvp_temporal_not_needed", "amvp_temporal_wanted_absent", "zero_one", "zero_two", "idx1_on_bits", "idx0_on_bits", "tie_sad_picks_1",
         "tie_sad_picks_0", "tie_bits_and_sad", "mvd_zero", "inter_won_zero_pricing_merged", "merged_zero_pricing_inter", "amvp_tie_stays_merge")
TABLE_LEN = 65537                   # 2 * BC_MAX_MV + 1 (bitcost.h): every difference of two int16 components has its own entry


def amvp_candidates(nb, temporal, mutation=None, temporal_unscaled=None):
    """CUData::getPMV for one reference.  nb: {"A0" | "A1" | "B0" | "B1" | "B2": packed motion, or None where the neighbour is not
    available}; temporal: the scaled collocated vector, or None (no temporal MVP, or the lookup failed).  Returns ([c0, c1], flags)."""
    assert mutation is None or mutation in LIST_MUTATIONS
    fl = {}
    cands = []
    left = ("A1", "A0") if mutation == "a1_before_a0" else ("A0", "A1")                        # :1740-1743
    above = ("B1", "B0", "B2") if mutation == "b1_before_b0" else ("B0", "B1", "B2")           # :1752-1757
    if mutation == "b2_never":
        above = above[:2]
    src_left = next((k for k in left if nb.get(k) is not None), None)
    src_above = next((k for k in above if nb.get(k) is not None), None)
    for k in ("A0", "A1"):
        fl["left_" + k] = src_left == k
    for k in ("B0", "B1", "B2"):
        fl["above_" + k] = src_above == k
    fl["left_absent"], fl["above_absent"] = src_left is None, src_above is None
    if src_left is not None:
        cands.append(nb[src_left])
    if src_above is not None:                                                                 # (bAddedSmvp gates the indirect ones only)
        cands.append(nb[src_above])
    fl["pair_reduced"] = len(cands) == 2 and cands[0] == cands[1]
    if fl["pair_reduced"] and mutation != "pair_not_reduced":                                 # :1779-1780
        cands.pop()
    spatial = len(cands)
    if mutation == "temporal_unscaled" and temporal is not None:
        temporal = temporal_unscaled
    fl["amvp_temporal_taken"] = temporal is not None and (spatial < 2 or mutation == "temporal_although_two")
    if fl["amvp_temporal_taken"]:                                                             # :1784-1801
        if spatial < 2:
            cands.append(temporal)
        else:
            cands[1] = temporal
    fl["zero_one"], fl["zero_two"] = len(cands) == 1, len(cands) == 0
    while len(cands) < 2:                                                                     # :1803-1804
        cands.append(cands[0] if (mutation == "no_zero_fill" and cands) else 0)
    return cands, fl


def bitcost(mv, mvp, table):
    """BitCost::bitcost(mv, mvp) (bitcost.h:54-58): (uint32_t)(s_bitsizes[|qx - px|] + s_bitsizes[|qy - py|] + 0.5f) in float32; a
    difference beyond the table takes its last entry (the entry's rule; the reference's table is never short)."""
    (qx, qy), (px, py) = unpack(mv), unpack(mvp)
    ix, iy = min(abs(qx - px), len(table) - 1), min(abs(qy - py), len(table) - 1)
    return int(np.uint32(np.float32(np.float32(table[ix] + table[iy]) + np.float32(0.5))))


def select_mvp(cands, dist, clip, mutation=None):
    """Search::selectMVP: dist(clipped packed vector) -> bufSAD of the luma prediction; clip: CUData::clipMv of the block."""
    if cands[0] == cands[1]:                                                                  # :1994-1995
        return 0
    c = [dist(clip(v)) for v in cands]                                                        # :2017-2019
    if mutation == "select_no_clip":
        # an unclipped vector may point outside the padded plane, where nothing can be predicted: the mutation stands in for it by
        # charging the distance between the vector and its clipped form, so of two candidates that clip to one vector the nearer one wins
        c = [d + sum(abs(p - q) for p, q in zip(unpack(v), unpack(clip(v)))) for d, v in zip(c, cands)]
    if mutation == "select_lt":
        return 0 if c[0] < c[1] else 1
    return 0 if c[0] <= c[1] else 1                                                           # :2022


def check_best_mvp(cands, mv, idx, table, mutation=None):
    """Search::checkBestMVP: the final index and bitcost(mv, amvp[index])."""
    b = [bitcost(mv, c, table) for c in cands]
    diff = b[1 - idx] - b[idx]                                                                # :2704
    if diff <= 0 if mutation == "check_le" else diff < 0:                                     # :2705
        idx = 1 - idx
    return idx, b[idx]


class SadSlots:
    """pu[].sad of the n x n luma block from the oracle's table, with Slots' cost() signature."""

    def __init__(self, depth, n):
        self.keep = IE.harness.load_oracle(depth, IE.ROOT)
        self.sad = self.keep.fn("pu[%d].sad" % {8: 1, 16: 2, 32: 3}[n])
        self.n = n

    def cost(self, fenc_ptr, fenc_stride, pred):
        return int(self.sad(fenc_ptr, fenc_stride, pred.ctypes.data, self.n))


class SadPricer(ME.Pricer):
    """merge_expect.Pricer with the plain SAD (bufSAD) in place of sa8d: the prediction of the clipped vector through the oracle, the
    distortion through the table's sad slot."""

    def __init__(self, depth, cur_y, ref_y, w64, h64, level):
        ME.Pricer.__init__(self, depth, cur_y, ref_y, w64, h64, level)
        self.slots = SadSlots(depth, self.n)


def fixpoint(pricer, sad_pricer, fn, limit=400):
    for _ in range(limit):
        out = fn(pricer.price, sad_pricer.price)
        if not pricer.missing and not sad_pricer.missing:
            return out
        pricer.evaluate()
        sad_pricer.evaluate()
    raise AssertionError("the walk did not settle")


def walk(w64, h64, level, searched, max_merge, price, sad, lam, table, base_bits, inter_sa8d=None, cost_fn=None, mutation=None, col=None, cur_delta=None):
    """merge_expect.walk plus the AMVP arm.  sad(block, packed clipped vector) -> bufSAD; table: the bit sizes; inter_sa8d: int per
    block, or cost_fn(block, merge cost) -> the inter COST the block shall have, from which the walk derives the sa8d to hand to the
    device (cost - rate).  mutation: one of MUTATIONS.  Returns ME.walk's dictionary (best / inter_cost with the AMVP inter cost) plus
    mvp_idx uint8, mvd / amvp / inter int32 [blocks, 2], inter_sa8d (what was or is to be handed in) and MASKS."""
    assert mutation is None or mutation in MUTATIONS
    g = ME.Grid(w64, h64, level)
    tot = g.tot
    final = np.zeros(tot, np.int64)
    merge, idx_out = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    mv_out, mv_pred = np.zeros(tot, np.int32), np.zeros(tot, np.int32)
    cost, best = np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32)
    mvp_idx, mvd, amvp, inter_out = np.zeros(tot, np.uint8), np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32)
    sa8d_used, ic_used = np.zeros(tot, np.int64), np.zeros(tot, np.int64)
    masks = {k: np.zeros(tot, bool) for k in ME.MASKS + TX.P_MASKS + MASKS}
    scratch = {k: np.zeros(tot, bool) for k in ME.MASKS + TX.P_MASKS}
    for b in range(tot):
        bx, by, x0, y0 = g.block(b)
        clip = lambda v: ME.clip_mv(v, x0, y0, w64, h64)
        nb, where = g.neighbours(b, lambda q: int(final[q]), masks)
        temporal = TX.temporal_vectors(col, level, x0, y0, (cur_delta,), masks, b)
        temporal = temporal and temporal[0]
        cands, fl = ME.candidate_list(nb, max_merge, None, temporal)
        for k, v in fl.items():
            masks[k][b] = v
        lam8 = lam(b)
        top, priced = None, []
        for i, (v, origin) in enumerate(cands):
            cl = clip(v)
            s = price(b, cl)
            c = s + ((ME.tu_bits(i, len(cands)) * lam8 + 128) >> 8)
            priced.append(c)
            if top is None or c < top[0]:                                                     # analysis.cpp:2833
                top = (c, s, i, v, cl, origin)
        c, s, i, v, cl, origin = top
        cost[b] = (s, c)
        # ---- the inter candidate: getNeighbourMV's five (A0 = below left, A1 = left, B0 = above right, B1 = above, B2 = above left) are
        # the merge list's neighbours under their AMVP names; their motion is what they ended up with
        pnb = dict(nb)
        if mutation == "searched_not_final":
            pnb = {k: (None if pnb[k] is None else int(searched[where[k]])) for k in pnb}
        unscaled = None
        if mutation == "temporal_unscaled" and temporal is not None:
            unscaled = TX.temporal_vectors(col, level, x0, y0, (cur_delta,), scratch, b, "no_scaling")[0]
        pm, pfl = amvp_candidates(pnb, temporal, mutation if mutation in LIST_MUTATIONS else None, unscaled)
        for k, f in pfl.items():
            masks[k][b] = f
        masks["amvp_temporal_not_needed"][b] = col is not None and not (pfl["zero_one"] or pfl["zero_two"] or pfl["amvp_temporal_taken"])
        masks["amvp_temporal_wanted_absent"][b] = col is not None and temporal is None and (pfl["zero_one"] or pfl["zero_two"])
        mv = int(searched[b])
        dist = (lambda q: price(b, q)) if mutation == "select_on_sa8d" else (lambda q: sad(b, q))
        first = select_mvp(pm, dist, clip, mutation)
        pidx, pbits = check_best_mvp(pm, mv, first, table, mutation)
        b0, b1 = bitcost(mv, pm[0], table), bitcost(mv, pm[1], table)
        if pm[0] != pm[1]:
            masks["idx1_on_bits"][b], masks["idx0_on_bits"][b] = b1 < b0, b0 < b1
            if b0 == b1:
                d0, d1 = dist(clip(pm[0])), dist(clip(pm[1]))
                masks["tie_sad_picks_1"][b], masks["tie_sad_picks_0"][b], masks["tie_bits_and_sad"][b] = d1 < d0, d0 < d1, d0 == d1
        if mutation == "price_against_zero":
            pbits = bitcost(mv, 0, table)
        bits = base_bits + pbits                                                              # search.cpp:2455
        rate = (bits * lam8 + 128) >> 8
        sa = int(cost_fn(b, c)) - rate if cost_fn is not None else int(inter_sa8d[b])
        ic = sa + rate                                                                        # calcRdSADCost, rdcost.h:148-153
        sa8d_used[b], ic_used[b] = sa, ic
        (qx, qy), (px, py) = unpack(mv), unpack(pm[pidx])
        mvp_idx[b], mvd[b], amvp[b], inter_out[b] = pidx, (qx - px, qy - py), pm, (bits, ic)
        masks["mvd_zero"][b] = (qx, qy) == (px, py)
        old = sa + (((base_bits + bitcost(mv, 0, table)) * lam8 + 128) >> 8)                   # the pricing against (0, 0)
        inter = ic < c                                                                        # analysis.cpp:1650
        masks["inter_won_zero_pricing_merged"][b], masks["merged_zero_pricing_inter"][b] = inter and not old < c, old < c and not inter
        masks["tie_stays_merge"][b] = masks["amvp_tie_stays_merge"][b] = ic == c
        if inter:
            final[b] = mv
            mv_out[b] = mv_pred[b] = mv
            best[b] = (-1, ic)
            masks["inter_won"][b] = True
            continue
        merge[b], idx_out[b] = 1, i
        final[b] = v
        mv_out[b], mv_pred[b] = v, cl
        best[b] = (s, c)
        masks["merge_won"][b] = True
    return dict(merge=merge, merge_idx=idx_out, mv_out=mv_out, mv_pred=mv_pred, cost=cost, best=best, inter_cost=ic_used, inter_sa8d=sa8d_used,
                mvp_idx=mvp_idx, mvd=mvd, amvp=amvp, inter=inter_out, masks=masks)


OUTPUTS = ("merge", "merge_idx", "mv_out", "mv_pred", "cost", "best", "mvp_idx", "mvd", "amvp", "inter")


def stage_expectation(depth, cur_y, ref_y, w64, h64, level, mv, max_merge, lambda8, table, base_bits, inter_sa8d=None, cost_fn=None, tu_qp=None,
                      lambda8_by_qp=None, qp=0, mutation=None, pricer=None, sad_pricer=None, col=None, cur_delta=None):
    """What x265hip_merge_decide_amvp leaves for the searched records mv (int32 [ctu*85, 2]): walk()'s dictionary with mv_out / mv_pred as
    RECORDS of the level's slots, as merge_expect.stage_expectation gives them."""
    pr = pricer or ME.Pricer(depth, cur_y, ref_y, w64, h64, level)
    sp = sad_pricer or SadPricer(depth, cur_y, ref_y, w64, h64, level)
    nctu = (w64 // 64) * (h64 // 64)
    sl = ME.level_slots(level, nctu)
    searched = np.asarray(mv).reshape(-1, 2)[sl, 1]

    def lam(b):
        gx, gy = pr.position(b)
        return IX.block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
    e = fixpoint(pr, sp, lambda price, sad: walk(w64, h64, level, searched, max_merge, price, sad, lam, table, base_bits, inter_sa8d=inter_sa8d,
                                                 cost_fn=cost_fn, mutation=mutation, col=col, cur_delta=cur_delta))
    words = np.where(e["merge"] != 0, e["cost"][:, 1], np.asarray(mv).reshape(-1, 2)[sl, 0])
    e["vec_out"], e["vec_pred"] = e["mv_out"], e["mv_pred"]
    e["mv_out"], e["mv_pred"] = ME.records(e["vec_out"], words, level, nctu)[sl], ME.records(e["vec_pred"], words, level, nctu)[sl]
    return e


def p_chain(depth, cur, ref, w64, h64, rng_r, subme, level, qp, max_merge=3, sao_rdo=None, tu_flags=ME.H.TU_SIGN_HIDE, base_bits=IX.BASE_BITS,
            lambda8=IE.LAMBDA8, cores=0, col=None, cur_delta=None):
    """merge_expect.p_chain with the AMVP arm: the CPU twin of stages.MergePFramePipeline(amvp=True).run.  Every stage output by name."""
    S = IE.importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = ME.F.padded_dims(w64, h64)
    nctu = (w64 // 64) * (h64 // 64)
    qpc = S.chroma_quant_qp(qp, depth)
    y, r = cur[0], ref[0]
    _, mv = ME.SC.search_head(depth, y, r, stride, org, w64, h64, rng_r, subme, cores=cores)
    it = IX.inter_side(depth, cur, ref, w64, h64, level, mv, qp, (qpc, qpc), tu_flags, base_bits=base_bits, lambda8=lambda8, table=IX.s_bitsizes(4 * rng_r + 4))
    e = stage_expectation(depth, y, r, w64, h64, level, mv, max_merge, lambda8, IX.s_bitsizes(TABLE_LEN), base_bits, inter_sa8d=it["inter_cost"][:, 0],
                          qp=qp, col=col, cur_delta=cur_delta)
    full = lambda recs: ME.records(recs[:, 1], recs[:, 0], level, nctu)
    mvp, mvo = full(e["mv_pred"]), full(e["mv_out"])
    cd = IX.inter_side(depth, cur, ref, w64, h64, level, mvp, qp, (qpc, qpc), tu_flags)
    out = {"subpel_mv": mv, "inter_cost": it["inter_cost"], "merge": e["merge"], "merge_idx": e["merge_idx"], "merge_cost": e["cost"], "best": e["best"],
           "mv_out": e["mv_out"], "mv_pred": e["mv_pred"], "mvp_idx": e["mvp_idx"], "mvd": e["mvd"], "amvp": e["amvp"], "inter": e["inter"]}
    out.update({k: cd[k] for k in ("levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")})
    out["skip"] = ME.skip_flags(e["merge"], cd["num_sig"], cd["num_sig_c0"], cd["num_sig_c1"])
    bv, bh = ME.O.deblock_bs_inter(depth, w64, h64, level, mvo, cd["num_sig"])
    return ME.SC.filter_tail(out, depth, cur, cd["recon"], [cd["recon_c0"], cd["recon_c1"]], bv, bh, qp, w64, h64, sao_rdo=sao_rdo, cores=cores)


def p_device_outputs(pipe, dt):
    """The same names from a stages.MergePFramePipeline(amvp=True) after run()."""
    g = lambda t: t.cpu().numpy()
    out = ME.p_device_outputs(pipe, dt)
    out.update({"mvp_idx": g(pipe.md.mvp_idx), "mvd": g(pipe.md.mvd).reshape(-1, 2), "amvp": g(pipe.md.amvp).reshape(-1, 2), "inter": g(pipe.md.inter).reshape(-1, 2)})
    return out
