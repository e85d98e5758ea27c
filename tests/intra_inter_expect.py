"""Expected results of the intra-in-inter stages of a P picture (x265hip_inter_sa8d_cost, x265hip_intra_in_inter), assembled from the
oracle's pieces and tests/intra_expect.py's.

The inter side is the oracle's: the luma prediction through oracle_api.pred_capture of the bi stage with every block on list 0, its
sa8d through the table's cu[].sa8d slot, the inter coding through O.inter_recon / O.inter_recon_chroma.  What is restated here is the
integer arithmetic of Analysis::checkInter_rd0_4 (analysis.cpp:3023-3071: bits = base + BitCost::bitcost, cost = calcRdSADCost) and the
coding-order walk of Analysis::compressInterCU_rd0_4's choice (analysis.cpp:1649-1671): the recon planes start as the inter
reconstruction, every block runs the 35-mode scan of Search::checkIntraInInter from the reconstruction around it, and a block whose
intra cost is strictly below its inter cost is recoded through O.intra_recon with the P slice's flags.  The most probable modes read DC
for a neighbour that is not intra (CUData::getIntraDirLumaPredictor, cudata.cpp:910-953)."""
import numpy as np

import intra_expect as IE

O, F, H, harness, SC = IE.O, IE.F, IE.H, IE.harness, IE.SC

BASE_BITS = 2                     # m_listSelBits[0] (1) + MVP_IDX_BITS (1) + getTUBits(0, 1) (0): H.ref_cost_bits(1, lam=1)[0]
MASKS = ("intra_won", "inter_won", "tie_stays_inter", "intra_left_is_inter", "intra_left_is_intra_angular", "intra_reads_inter_recon_across_ctu",
         "intra_reads_intra_recon", "inter_after_intra_in_ctu")
MUTATIONS = ("le_in_choice", "stale_mode_in_mpm", "tiles_not_primed", "intra_slice_rounding")


def s_bitsizes(length):
    """BitCost::s_bitsizes[0 .. length - 1], the statements of bitcost.cpp:105-108 in float32."""
    out = np.zeros(length, np.float32)
    out[0] = np.float32(0.718)
    log2_2 = np.float32(2.0) / np.log(np.float32(2.0))
    for i in range(1, length):
        out[i] = np.log(np.float32(i + 1)) * log2_2 + np.float32(1.718)
    return out


def mv_bits(packed, table):
    """BitCost::bitcost(mv) against the predictor (0, 0) (bitcost.h:48-52); a component beyond the table takes its last entry."""
    s16 = lambda v: (v & 0xffff) - ((v & 0x8000) << 1)
    qx, qy = s16(packed), s16(packed >> 16)
    ix, iy = min(abs(qx), len(table) - 1), min(abs(qy), len(table) - 1)
    return int(np.uint32(np.float32(np.float32(table[ix] + table[iy]) + np.float32(0.5))))


def pack_mv(qx, qy):
    v = (int(qx) & 0xffff) | ((int(qy) & 0xffff) << 16)
    return v - (1 << 32) if v & (1 << 31) else v


def mv_records(vectors, level, nctu):
    """int32 [nctu * 85, 2] records {cost, qx | qy << 16} with vectors[ctu * blocks + z] = (qx, qy) at the level's slots."""
    nblk = 64 >> (2 * level)
    lbase = (0, 64, 80)[level]
    mv = np.zeros((nctu * 85, 2), np.int32)
    for b, (qx, qy) in enumerate(vectors):
        mv[(b // nblk) * 85 + lbase + b % nblk, 1] = pack_mv(qx, qy)
    return mv


def block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy):
    if lambda8_by_qp is None:
        return lambda8
    q = qp if tu_qp is None else min(max(int(tu_qp[0, gy // 8, gx // 8]), 0), 51 + 6 * (depth - 8))
    return min(int(lambda8_by_qp[q]), 1 << 24)


def inter_side(depth, cur, ref, w64, h64, level, mv, qp, qp_c, flags, chroma=True, tu_qp=None, base_bits=BASE_BITS, lambda8=IE.LAMBDA8, lambda8_by_qp=None,
               table=None, avx2=False):
    """The inter candidate of every block.  cur / ref: padded (Y [rows, stride], Cb, Cr) host planes, mv: the records.  Returns dict:
    inter_cost int32 [blocks, 2] = {sa8d, cost}, pred (the luma prediction), recon / levels / num_sig / dist (+ _c0 / _c1) of the inter coding."""
    import qp_map_expect as QE
    n = 8 << level
    nblk = (64 // n) ** 2
    cw = w64 // 64
    nctu = cw * (h64 // 64)
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    table = s_bitsizes(4 * 64 + 4) if table is None else table
    y, r = np.ascontiguousarray(cur[0]).reshape(-1), np.ascontiguousarray(ref[0]).reshape(-1)
    cap = np.zeros((h64, w64), y.dtype)
    with O.pred_capture(depth, cap, avx2=avx2):
        O.inter_recon_bi(depth, y, stride, org, r, r, w64, h64, level, mv, mv, qp, dir_flags=np.ones(nctu * nblk, np.uint8), avx2=avx2)
    slots = IE.Slots(depth, n, with_reference=False)
    lbase = (0, 64, 80)[level]
    ic = np.zeros((nctu * nblk, 2), np.int32)
    for b in range(nctu * nblk):
        ctu, z = divmod(b, nblk)
        bx, by = IE.zorder(z)
        gx, gy = (ctu % cw) * 64 + bx * n, (ctu // cw) * 64 + by * n
        p = np.ascontiguousarray(cap[gy:gy + n, gx:gx + n])
        sad = slots.cost(y.ctypes.data + (org + gy * stride + gx) * y.itemsize, stride, p)
        bits = base_bits + mv_bits(int(mv[ctu * 85 + lbase + z, 1]), table)
        lam = block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
        ic[b] = (sad, sad + ((bits * lam + 128) >> 8))                                              # calcRdSADCost, rdcost.h:148-153
    out = {"inter_cost": ic, "pred": cap}

    def luma(q):
        return O.inter_recon(depth, y, stride, org, r, stride, org, w64, h64, level, mv, q, intra_slice=flags, avx2=avx2)

    def chroma_run(c):
        return lambda q: O.inter_recon_chroma(depth, np.ascontiguousarray(cur[c]).reshape(-1), np.ascontiguousarray(ref[c]).reshape(-1), sc, oc, w64, h64, level, mv,
                                              q, intra_slice=flags, avx2=avx2)
    if tu_qp is None:
        res = [luma(qp)] + ([chroma_run(c)(qp_c[c - 1]) for c in (1, 2)] if chroma else [])
    else:
        res = [QE._composed(luma, tu_qp[0], w64, h64, level, False, stride, org)] + \
              ([QE._composed(chroma_run(c), tu_qp[c], w64, h64, level, True, sc, oc) for c in (1, 2)] if chroma else [])
    for i, (rec, lev, ns, dist) in enumerate(res):
        sfx = "" if i == 0 else "_c%d" % (i - 1)
        out.update({"recon" + sfx: np.ascontiguousarray(rec).reshape(-1), "levels" + sfx: lev, "num_sig" + sfx: ns, "dist" + sfx: dist})
    return out


def walk(depth, cur, w64, h64, level, qp, inter, qp_c=None, flags=0, lambda8=IE.LAMBDA8, mode_bits=IE.MODE_BITS, strong=True, chroma=True, tu_qp=None,
         lambda8_by_qp=None, inter_cost=None, cost_fn=None, mutation=None, with_reference=False):
    """The coding-order walk.  cur: padded (Y, Cb, Cr) source planes; inter: inter_side()'s dict (the recon planes' initial state and the
    coding an inter block keeps); inter_cost: int32 per block (default inter["inter_cost"][:, 1]), or cost_fn(block, intra cost) -> the
    inter cost to decide that block against (ties and near-ties on a fixed pattern).  mutation: one of MUTATIONS (what a wrong kernel
    would compute) or None.  Returns intra_expect.expect's dictionary plus intra uint8, inter_cost int32 (the numbers decided against) and
    the masks of MASKS; `mode` holds DC for an inter block, `cost` the INTRA candidate's {sad, cost} of every block."""
    assert mutation is None or mutation in MUTATIONS
    n = 8 << level
    bpc = 64 // n
    nblk = bpc * bpc
    cw, chh = w64 // 64, h64 // 64
    nctu = cw * chh
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    nplanes = 3 if chroma else 1
    src = [np.ascontiguousarray(cur[c]).reshape(-1) for c in range(nplanes)]
    sfx = ["", "_c0", "_c1"][:nplanes]
    rec = [np.array(inter["recon" + s], copy=True).reshape(-1) for s in sfx]
    lev = [np.array(inter["levels" + s], copy=True) for s in sfx]
    ns = [np.array(inter["num_sig" + s], copy=True) for s in sfx]
    dist = [np.array(inter["dist" + s], copy=True) for s in sfx]
    # what neighbours are read from: the recon planes - except under tiles_not_primed, where a CTU's own area reads as zero until a block
    # of the CTU is coded as intra (a kernel whose working tiles do not start as the inter reconstruction)
    view = rec if mutation != "tiles_not_primed" else [p.copy() for p in rec]
    slots = IE.Slots(depth, n, with_reference)
    log2n = int(np.log2(n))
    es = src[0].itemsize
    nc = n // 2
    qp_c = qp_c if qp_c is not None else (qp, qp)
    qmax = 51 + 6 * (depth - 8)
    tot = nctu * nblk
    ic_in = None if inter_cost is None and cost_fn is not None else np.asarray(inter["inter_cost"][:, 1] if inter_cost is None else inter_cost, np.int64)
    ic_used = np.zeros(tot, np.int32)
    mode_out, mpm_mode, intra = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    cost_out = np.zeros((tot, 2), np.int32)
    masks = {k: np.zeros(tot, bool) for k in MASKS}
    job = np.zeros(1, dtype=H.job_dtype())
    code_flags = flags | (H.TU_INTRA_SLICE if mutation == "intra_slice_rounding" else 0)

    def area(plane, c, x0, y0, w, h):
        """view of the w x h samples at (x0, y0) of plane c"""
        if c == 0:
            return plane.reshape(rows, stride)[F.MARGIN_Y + y0:F.MARGIN_Y + y0 + h, F.MARGIN_X + x0:F.MARGIN_X + x0 + w]
        return plane.reshape(-1, sc)[F.CHROMA_MARGIN_Y + y0:F.CHROMA_MARGIN_Y + y0 + h, F.CHROMA_MARGIN_X + x0:F.CHROMA_MARGIN_X + x0 + w]

    for ctu in range(nctu):
        cx, cy = (ctu % cw) * 64, (ctu // cw) * 64
        if view is not rec:
            for c in range(nplanes):
                area(view[c], c, cx >> (c > 0), cy >> (c > 0), 64 >> (c > 0), 64 >> (c > 0))[:] = 0
        for z in range(nblk):
            bx, by = IE.zorder(z)
            gx, gy = cx + bx * n, cy + by * n
            b = ctu * nblk + z
            qps = [qp, qp_c[0], qp_c[1]] if tu_qp is None else [min(max(int(tu_qp[c, gy // 8, gx // 8]), 0), qmax) for c in range(3)]
            lam = block_lambda(tu_qp, lambda8_by_qp, lambda8, qp, depth, gx, gy)
            flg = IE.neighbour_flags(gx, gy, n, w64, h64)
            off = org + gy * stride + gx
            ref_buf = IE.fill_reference_samples(view[0], off, stride, flg, n, 4, depth)
            flt_buf, _ = IE.init_adi_pattern(ref_buf, n, depth, strong, slots)
            # getIntraDirLumaPredictor: the left block if it is inside the picture, the above block only inside the CTU - and DC where that
            # block is not intra (mpm_mode holds DC for inter blocks)
            li = IE.coding_index(gx - 1, gy, n, w64, nblk) if gx > 0 else -1
            ai = IE.coding_index(gx, gy - 1, n, w64, nblk) if by > 0 else -1
            left = int(mpm_mode[li]) if li >= 0 else 1
            above = int(mpm_mode[ai]) if ai >= 0 else 1
            preds = IE.most_probable_modes(left, above)
            fp = src[0].ctypes.data + off * es
            best = None
            for mode in IE.SCAN_ORDER:
                buf = ref_buf if mode == 1 else (flt_buf if IE.FILTER_FLAGS[mode] & n else ref_buf)
                p = slots.predict(mode, buf, 1 if (n <= 16 and mode != 0) else 0)
                sad = slots.cost(fp, stride, p)
                bits = mode_bits[0] if mode == preds[0] else (mode_bits[1] if mode in preds[1:] else mode_bits[2])
                cost = sad + ((bits * lam + 128) >> 8)
                if best is None or cost < best[0]:
                    best = (cost, sad, mode, p)
            cost, sad, mode, pwin = best
            cost_out[b] = (sad, cost)
            ic = int(cost_fn(b, cost)) if cost_fn is not None else int(ic_in[b])
            ic_used[b] = ic
            wins = cost <= ic if mutation == "le_in_choice" else cost < ic                         # analysis.cpp:1664: strictly lower
            masks["tie_stays_inter"][b] = cost == ic
            reads = [c_ * nblk + z_ for (c_, z_) in IE.reads_of_block(gx, gy, n, w64, h64)]
            if not wins:
                mode_out[b] = 1
                mpm_mode[b] = mode if mutation == "stale_mode_in_mpm" else 1
                masks["inter_won"][b] = True
                masks["inter_after_intra_in_ctu"][b] = intra[ctu * nblk:b].any()
                continue
            intra[b], mode_out[b], mpm_mode[b] = 1, mode, mode
            masks["intra_won"][b] = True
            masks["intra_left_is_inter"][b] = li >= 0 and not intra[li]
            masks["intra_left_is_intra_angular"][b] = li >= 0 and bool(intra[li]) and mode_out[li] >= 2
            masks["intra_reads_inter_recon_across_ctu"][b] = any(not intra[q] and q // nblk != ctu for q in reads)
            masks["intra_reads_intra_recon"][b] = any(intra[q] for q in reads)
            if slots.ref_pred_intra is not None:
                want = np.zeros((n, n), slots.dt)
                assert slots.ref_pred_intra(mode, log2n, ref_buf.ctypes.data, flt_buf.ctypes.data, 0, want.ctypes.data) == 0
                assert np.array_equal(want, pwin), f"block {b}: x265ref_pred_intra disagrees with the winning prediction of mode {mode}"
            nbs = np.concatenate([ref_buf, flt_buf])
            job["off"][0] = (off, 0, 4 * n + 1, 0)
            job["arg"][0, 0] = mode
            r, l, s_, d = O.intra_recon(depth, n, src[0], stride, nbs, n * n, n, qps[0], code_flags, job)
            for pl in ([rec[0]] if view is rec else [rec[0], view[0]]):
                area(pl, 0, gx, gy, n, n)[:] = r.reshape(n, n)
            lev[0][b * n * n:(b + 1) * n * n], ns[0][b], dist[0][b] = l, s_[0], d[0]
            for c in range(nplanes - 1):
                offc = oc + (gy // 2) * sc + gx // 2
                cb = IE.fill_reference_samples(view[1 + c], offc, sc, flg, nc, 2, depth)
                job["off"][0] = (offc, 0, 0, 0)
                r, l, s_, d = O.intra_recon(depth, nc, src[1 + c], sc, cb, nc * nc, nc, qps[1 + c], code_flags, job, chroma=True)
                for pl in ([rec[1 + c]] if view is rec else [rec[1 + c], view[1 + c]]):
                    area(pl, 1 + c, gx // 2, gy // 2, nc, nc)[:] = r.reshape(nc, nc)
                lev[1 + c][b * nc * nc:(b + 1) * nc * nc], ns[1 + c][b], dist[1 + c][b] = l, s_[0], d[0]
        if view is not rec:                                     # the CTU is done: other CTUs read what the planes hold
            for c in range(nplanes):
                s = 64 >> (c > 0)
                area(view[c], c, cx >> (c > 0), cy >> (c > 0), s, s)[:] = area(rec[c], c, cx >> (c > 0), cy >> (c > 0), s, s)
    out = dict(mode=mode_out, cost=cost_out, intra=intra, inter_cost=ic_used, levels=lev[0], num_sig=ns[0], dist=dist[0], recon=rec[0], masks=masks,
               tables=slots.tables)
    for c in range(nplanes - 1):
        out.update({"levels_c%d" % c: lev[1 + c], "num_sig_c%d" % c: ns[1 + c], "dist_c%d" % c: dist[1 + c], "recon_c%d" % c: rec[1 + c]})
    return out


def tie_pattern(b, intra_cost):
    """The supplied inter cost of the tie cases: intra cost - 1 (inter wins), the intra cost itself (a tie: inter), + 1 (intra wins), by block
    index modulo 3."""
    return intra_cost + (b % 3) - 1


def p_chain(depth, cur, ref, w64, h64, rng_r, subme, level, qp, sao_rdo=None, tu_flags=H.TU_SIGN_HIDE, base_bits=BASE_BITS, cores=0, avx2=False):
    """One P picture with intra blocks through the oracle, stage by stage (the CPU twin of stages.IntraPFramePipeline.run with chroma,
    deblocking and SAO applied): search, refinement, inter coding, the walk, boundary strengths with the intra flags, deblocking, SAO,
    borders.  Every stage output by name."""
    S = IE.importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    qpc = S.chroma_quant_qp(qp, depth)
    _, mv = SC.search_head(depth, cur[0], ref[0], stride, org, w64, h64, rng_r, subme, cores=cores, avx2=avx2)
    it = inter_side(depth, cur, ref, w64, h64, level, mv, qp, (qpc, qpc), tu_flags, base_bits=base_bits, table=s_bitsizes(4 * rng_r + 4), avx2=avx2)
    e = walk(depth, cur, w64, h64, level, qp, it, qp_c=(qpc, qpc), flags=tu_flags)
    out = {"subpel_mv": mv, "inter_cost": it["inter_cost"]}
    out.update({k: e[k] for k in ("mode", "intra", "levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")})
    bv, bh = O.deblock_bs_inter(depth, w64, h64, level, mv, e["num_sig"], avx2=avx2, intra=e["intra"])
    return SC.filter_tail(out, depth, cur, e["recon"], [e["recon_c0"], e["recon_c1"]], bv, bh, qp, w64, h64, sao_rdo=sao_rdo, cores=cores, avx2=avx2)


def p_device_outputs(pipe, dt):
    """The same names from a stages.IntraPFramePipeline after run() (chroma, deblocking, SAO applied)."""
    g = lambda t: t.cpu().numpy()
    out = SC.step_outputs(pipe, dt)
    out.update({"subpel_mv": g(pipe.sp.out).reshape(-1, 2), "inter_cost": g(pipe.ic.cost).reshape(-1, 2), "mode": g(pipe.ii.mode), "intra": g(pipe.ii.intra)})
    return out
