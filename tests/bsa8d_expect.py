"""Expected results of the sa8d choice of a B picture's blocks (x265hip_b_sa8d_decide) and of stages.Sa8dBFramePipeline, assembled from the
oracle's pieces and the expectations that exist.

Nothing here computes a prediction or a transform of its own: the two lists' records are bidir_expect.oracle_records, the bidirectional
prediction P (addAvg of the 14-bit intermediates) and the single-list predictions (rounded pixels) are captured from the oracle's bi stage
through oracle_api.pred_capture - every block on both lists, or every block on one -, sa8d and pixelavg_pp are the oracle table's
cu[].sa8d and pu[].pixelavg_pp slots (the real reference's beside them where oracle/_ref is built: both are called and must agree), the
vector bits are intra_inter_expect.mv_bits, the intra part is intra_inter_expect.walk fed with this decision's outputs and costs, and the
coding chain is O.inter_recon_bi / O.inter_recon_chroma_bi, O.deblock_bs_b(intra=) and the SAO / border chain of bidir_expect.b_chain.
What is restated here is the integer arithmetic of Analysis::checkInter_rd0_4 (analysis.cpp:3059-3071), Analysis::checkBidir2Nx2N
(:3145-3270) and the choice of Analysis::compressInterCU_rd0_4 (:1649-1655)."""
import importlib

import numpy as np

import bidir_expect as BE
import intra_expect as IE
import intra_inter_expect as IX

O, F, H, harness, SC = IE.O, IE.F, IE.H, IE.harness, IE.SC
spec = BE.spec

DIR_COST = BE.DIR_COST
BASE_BITS, BI_BITS_DELTA = (4, 4), -1          # H.b_sa8d_bits(): (3 + 1 + 0) per list, 5 - 3 - 3
OUTCOMES = ("list0_kept", "list1_kept", "bi_searched", "bi_zero")
MUTATIONS = ("le_in_choice", "avg_of_rounded", "no_bits_delta", "no_zero_twin", "list_by_sa8d")
FLAG_LIST1, FLAG_ZERO_WON, FLAG_ZERO_TRIED = 1, 2, 4


class Slots:
    """cu[].sa8d and pu[].pixelavg_pp of the N x N luma block from the oracle's table - and the real reference's where it is built."""

    def __init__(self, depth, n, with_reference=True):
        self.cu = IE.Slots(depth, n, with_reference)
        self.pu = BE.Slots(depth, n, with_reference)
        self.n, self.dt, self.tables = n, self.cu.dt, self.cu.tables

    def sa8d(self, fenc_ptr, fenc_stride, pred):
        return self.cu.cost(fenc_ptr, fenc_stride, np.ascontiguousarray(pred))

    def average(self, a_ptr, a_stride, b_ptr, b_stride):
        outs = []
        for avg in self.pu.avg:
            tmp = np.zeros((self.n, self.n), self.dt)
            avg(tmp.ctypes.data, self.n, a_ptr, a_stride, b_ptr, b_stride, 32)
            outs.append(tmp)
        assert all(np.array_equal(outs[0], o) for o in outs[1:]), "oracle and reference pixelavg_pp disagree"
        return outs[0]


def captured_prediction(depth, cur, fref0, fref1, w64, h64, level, mv0, mv1, direction, avx2=False):
    """The luma prediction the oracle's bi stage forms with every block on `direction` (1: fref0 / mv0 alone, rounded pixels; 3: addAvg of
    both lists' 14-bit intermediates), [h64, w64]."""
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    n = 8 << level
    nblk = (64 // n) ** 2
    nctu = (w64 // 64) * (h64 // 64)
    flat = lambda p: np.ascontiguousarray(p).reshape(-1)
    cap = np.zeros((h64, w64), cur.dtype)
    with O.pred_capture(depth, cap, avx2=avx2):
        O.inter_recon_bi(depth, flat(cur), stride, org, flat(fref0), flat(fref1), w64, h64, level, mv0, mv1, 30 + 6 * (depth - 8),
                         dir_flags=np.full(nctu * nblk, direction, np.uint8), avx2=avx2)
    return cap


def decide(depth, cur, refs, w64, h64, level, recs, dir_cost=DIR_COST, base_bits=BASE_BITS, bi_bits_delta=BI_BITS_DELTA, lambda8=IE.LAMBDA8, table=None,
           qp=0, tu_qp=None, lambda8_by_qp=None, ref_ids=(0, 1), mutation=None, with_reference=True):
    """The decision for every block of `level`.  cur / refs = (list 0, list 1): padded luma planes [rows, stride]; recs = the two lists'
    records [nctu * 85, 2].  Returns dict: dir uint8 [blocks], ref0 / ref1 int8, mv0 / mv1 int32 [blocks, 2] (the level's entries of
    mv*_out in block order), cost int32 [blocks, 4] = {winner, uni, bi after the zero pair, flags}, sa8d int32 [blocks, 4] = the plain sa8d
    of {list 0, list 1, both, zero pair} and the masks of OUTCOMES."""
    assert mutation is None or mutation in MUTATIONS
    n, nb, base = 8 << level, (64 >> (3 + level)) ** 2, BE.LEVEL_BASE[level]
    cw = w64 // 64
    nctu = cw * (h64 // 64)
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    table = IX.s_bitsizes(4 * 57 + 4) if table is None else table
    slots = Slots(depth, n, with_reference)
    es = cur.itemsize
    recs = [np.ascontiguousarray(r, dtype=np.int32).reshape(-1, 2) for r in recs]
    pred_bi = captured_prediction(depth, cur, refs[0], refs[1], w64, h64, level, recs[0], recs[1], 3)
    pred_l = [captured_prediction(depth, cur, refs[l], refs[l], w64, h64, level, recs[l], recs[l], 1) for l in (0, 1)]
    tot = nctu * nb
    d = np.zeros(tot, np.uint8)
    ref0, ref1 = np.zeros(tot, np.int8), np.zeros(tot, np.int8)
    mvo = [np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32)]
    cost, sa = np.zeros((tot, 4), np.int32), np.zeros((tot, 4), np.int32)
    masks = {k: np.zeros(tot, bool) for k in OUTCOMES}
    delta = 0 if mutation == "no_bits_delta" else bi_bits_delta
    zero_bits = IX.mv_bits(0, table)
    for ctu in range(nctu):
        cx, cy = (ctu % cw) * 64, (ctu // cw) * 64
        for z in range(nb):
            bx, by = BE.zorder(z)
            gx, gy = cx + bx * n, cy + by * n
            off = org + gy * stride + gx
            b = ctu * nb + z
            fp = cur.ctypes.data + off * es
            lam = IX.block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
            rate = lambda bits: (bits * lam + 128) >> 8                                             # RDCost::getCost
            words = [int(recs[l][ctu * 85 + base + z, 1]) for l in (0, 1)]
            cl = [int(recs[l][ctu * 85 + base + z, 0]) + dir_cost[l] for l in (0, 1)]
            bits = [base_bits[l] + IX.mv_bits(words[l], table) for l in (0, 1)]
            blk = lambda p: p[gy:gy + n, gx:gx + n]
            s_l = [slots.sa8d(fp, stride, blk(pred_l[l])) for l in (0, 1)]
            uni_l = [s_l[l] + rate(bits[l]) for l in (0, 1)]
            if mutation == "list_by_sa8d":
                l = 0 if uni_l[0] <= uni_l[1] else 1
            else:
                l = 0 if cl[0] <= cl[1] else 1                                                      # search.cpp:2611: list 0 on a tie
            uni = uni_l[l]
            if mutation == "avg_of_rounded":
                p0, p1 = np.ascontiguousarray(blk(pred_l[0])), np.ascontiguousarray(blk(pred_l[1]))
                pbi = slots.average(p0.ctypes.data, n, p1.ctypes.data, n)
            else:
                pbi = blk(pred_bi)
            s_bi = slots.sa8d(fp, stride, pbi)
            bi = s_bi + rate(bits[0] + bits[1] + delta)                                             # analysis.cpp:3197-3198
            m, flags, s_z = list(words), l, -1
            if (words[0] != 0 or words[1] != 0) and mutation != "no_zero_twin":                     # bTryZero
                zp = slots.average(refs[0].ctypes.data + off * es, stride, refs[1].ctypes.data + off * es, stride)
                s_z = slots.sa8d(fp, stride, zp)
                zc = s_z + rate(base_bits[0] + base_bits[1] + 2 * zero_bits + delta)                # :3241-3250
                flags |= FLAG_ZERO_TRIED
                if zc < bi:
                    bi, m, flags = zc, [0, 0], flags | FLAG_ZERO_WON
            three = bi <= uni if mutation == "le_in_choice" else bi < uni                          # :1653: strictly cheaper
            dd = 3 if three else 1 + l
            d[b] = dd
            ref0[b] = ref_ids[0] if dd & 1 else -1
            ref1[b] = ref_ids[1] if dd & 2 else -1
            win = bi if dd == 3 else uni
            mvo[0][b] = (win, m[0] if dd == 3 else words[0]) if dd & 1 else (cl[0], 0)
            mvo[1][b] = (win, m[1] if dd == 3 else words[1]) if dd & 2 else (cl[1], 0)
            cost[b] = (win, uni, bi, flags)
            sa[b] = (s_l[0], s_l[1], s_bi, s_z)
            masks["list0_kept"][b], masks["list1_kept"][b] = dd == 1, dd == 2
            masks["bi_searched"][b] = dd == 3 and not flags & FLAG_ZERO_WON
            masks["bi_zero"][b] = dd == 3 and bool(flags & FLAG_ZERO_WON)
    return dict(dir=d, ref0=ref0, ref1=ref1, mv0=mvo[0], mv1=mvo[1], cost=cost, sa8d=sa, masks=masks, tables=slots.tables)


INTRA_MASKS = ("intra_beats_single", "intra_beats_bi", "inter_kept", "intra_beside_bi")


def inter_coding(depth, cur, refs, w64, h64, level, e, qp, qp_c, flags, chroma=True, avx2=False, cores=0):
    """The bi-predictive coding of the decision e (decide()'s dict) in the names intra_inter_expect.walk takes: recon / levels / num_sig / dist
    (+ _c0 / _c1) and inter_cost [blocks, 2] whose second word is the winning inter sa8d cost.  cur / refs: padded (Y, Cb, Cr) planes."""
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    nctu = (w64 // 64) * (h64 // 64)
    flat = lambda p: np.ascontiguousarray(p).reshape(-1)
    mv0, mv1 = BE.full_mv_out(level, nctu, e["mv0"], 0), BE.full_mv_out(level, nctu, e["mv1"], 0)
    res = [O.inter_recon_bi(depth, flat(cur[0]), stride, org, flat(refs[0][0]), flat(refs[1][0]), w64, h64, level, mv0, mv1, qp, dir_flags=e["dir"],
                            intra_slice=flags, nthreads=cores, avx2=avx2)]
    if chroma:
        res += [O.inter_recon_chroma_bi(depth, flat(cur[c]), flat(refs[0][c]), flat(refs[1][c]), sc, oc, w64, h64, level, mv0, mv1, qp_c[c - 1],
                                        dir_flags=e["dir"], intra_slice=flags, nthreads=cores, avx2=avx2) for c in (1, 2)]
    out = {"inter_cost": np.stack([e["cost"][:, 1], e["cost"][:, 0]], axis=1).astype(np.int32), "mv0_out": mv0, "mv1_out": mv1}
    for i, (rec, lev, ns, dist) in enumerate(res):
        sfx = "" if i == 0 else "_c%d" % (i - 1)
        out.update({"recon" + sfx: np.ascontiguousarray(rec).reshape(-1), "levels" + sfx: lev, "num_sig" + sfx: ns, "dist" + sfx: dist})
    return out


def intra_masks(e, w, w64, level):
    """What the intra walk w reached on the decision e: the masks of INTRA_MASKS."""
    n = 8 << level
    nblk = (64 // n) ** 2
    intra = w["intra"].astype(bool)
    beside = np.zeros(len(intra), bool)
    for b in np.flatnonzero(intra):
        ctu, z = divmod(int(b), nblk)
        bx, by = IE.zorder(z)
        gx, gy = (ctu % (w64 // 64)) * 64 + bx * n, (ctu // (w64 // 64)) * 64 + by * n
        for (x, y) in ((gx - 1, gy), (gx, gy - 1)):
            if x >= 0 and y >= 0:
                q = IE.coding_index(x, y, n, w64, nblk)
                beside[b] |= bool(e["dir"][q] == 3 and not intra[q])
    return {"intra_beats_single": intra & (e["dir"] != 3), "intra_beats_bi": intra & (e["dir"] == 3), "inter_kept": ~intra, "intra_beside_bi": beside}


def sa8d_b_chain(depth, cur_planes, ref0_planes, ref1_planes, w64, h64, rng_r, subme, level, qp, b_intra, sao_rdo=None, dir_cost=DIR_COST,
                 tu_flags=H.TU_SIGN_HIDE, lambda8=IE.LAMBDA8, mode_bits=IE.MODE_BITS, cores=0, avx2=False, with_reference=False):
    """One B picture through the oracle, stage by stage (the CPU twin of stages.Sa8dBFramePipeline.run with chroma, deblocking and SAO
    applied).  *_planes = padded (Y, Cb, Cr) host planes.  Every stage output by name."""
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    cur, r0, r1 = cur_planes[0], ref0_planes[0], ref1_planes[0]
    out, recs = {}, []
    for l, ref in enumerate((r0, r1)):
        recs.append(SC.search_head(depth, cur, ref, stride, org, w64, h64, rng_r, subme, cores=cores, avx2=avx2)[1])
        out["subpel_mv%d" % l] = recs[l]
    e = decide(depth, cur, (r0, r1), w64, h64, level, recs, dir_cost=dir_cost, lambda8=lambda8, table=IX.s_bitsizes(4 * rng_r + 4), qp=qp,
               with_reference=with_reference)
    qpc = S.chroma_quant_qp(qp, depth)
    it = inter_coding(depth, cur_planes, (ref0_planes, ref1_planes), w64, h64, level, e, qp, (qpc, qpc), tu_flags, avx2=avx2, cores=cores)
    mv0, mv1 = it["mv0_out"], it["mv1_out"]
    out.update({"dir": e["dir"], "ref0": e["ref0"], "ref1": e["ref1"], "mv0_out": mv0, "mv1_out": mv1, "b_cost": e["cost"]})
    intra = None
    if b_intra:
        w = IX.walk(depth, cur_planes, w64, h64, level, qp, it, qp_c=(qpc, qpc), flags=tu_flags, lambda8=lambda8, mode_bits=mode_bits)
        intra = w["intra"]
        out.update({"mode": w["mode"], "intra": intra})
        it = w
    out.update({k: it[k] for k in ("levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")})
    bv, bh = O.deblock_bs_b(depth, w64, h64, level, mv0, mv1, e["ref0"], e["ref1"], it["num_sig"], slice_b=True, intra=intra, avx2=avx2)
    return SC.filter_tail(out, depth, cur_planes, it["recon"], [it["recon_c0"], it["recon_c1"]], bv, bh, qp, w64, h64, sao_rdo=sao_rdo, cores=cores, avx2=avx2)


def device_outputs(pipe, dt):
    """The same names from a stages.Sa8dBFramePipeline after run() (chroma, deblocking, SAO applied)."""
    g = lambda t: t.cpu().numpy()
    out, bd = SC.step_outputs(pipe, dt), pipe.bd
    out.update({"subpel_mv0": g(pipe.spl[0].out).reshape(-1, 2), "subpel_mv1": g(pipe.spl[1].out).reshape(-1, 2), "dir": g(bd.dir), "ref0": g(bd.ref0), "ref1": g(bd.ref1),
                "mv0_out": g(bd.mv0_out).reshape(-1, 2), "mv1_out": g(bd.mv1_out).reshape(-1, 2), "b_cost": g(bd.cost).reshape(-1, 4)})
    if pipe.ii is not None:
        out.update({"mode": g(pipe.ii.mode), "intra": g(pipe.ii.intra)})
    return out
