"""Expected results of the coding stages under a per-block QP map, without touching the oracle.

  * cu_qp_maps_restated: a literal Python restatement of the non-hevcAq arm of Analysis::calculateQpforCuSize (analysis.cpp:3679-3713) and
    of Quant::setQPforQuant / setChromaQP (quant.cpp:221-244) - Python floats are the reference's doubles, the summation order is the
    reference's - for x265hip_cu_qp_maps.
  * the synthetic map of the GPU tests (map_values / block_qps / cells_of_blocks) and the coverage it has to have (coverage).
  * compose: inter blocks do not depend on each other, so the expectation for a map with the values q1..qk is the oracle stage run once
    per q with a uniform QP, every block's levels, numSig, SSE and samples taken from the run of its own q.
  * walk: I pictures - blocks read their neighbours' reconstruction - as the coding-order walk of tests/intra_expect.py (its pieces are
    imported, the file is not changed) with the block's own three QPs and its own lambda."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import step_chain as SC         # noqa: E402

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

# g_chromaScale (constants.cpp:346-350), indices 0..69
CHROMA_SCALE = list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + list(range(38, 52)) + [51] * 18


def cu_qp_maps_restated(depth, width, height, level, qg_size, base_qp, qp_offsets, qp_min=0, qp_max=51, cb_qp_offset=0, cr_qp_offset=0):
    """(cu_qp int8 [h/8, w/8], tu_qp int8 [3, h/8, w/8]) the way the reference forms them, CU by CU."""
    bd = 6 * (depth - 8)
    loop_incr = 8 if qg_size == 8 else 16                                       # analysis.cpp:3679
    max_cols = (width + (loop_incr - 1)) // loop_incr                           # :3688
    block_size = 8 << level                                                     # :3689 (maxCUSize >> depth)
    cu = np.zeros((height // 8, width // 8), np.int8)
    tu = np.zeros((3, height // 8, width // 8), np.int8)

    def chroma(qpin):                                                           # quant.cpp:233-244, 4:2:0
        qp = min(max(qpin, -bd), 57)
        if qp >= 30:
            qp = CHROMA_SCALE[qp]
        return qp + bd
    for block_y in range(0, height, block_size):
        for block_x in range(0, width, block_size):
            qp = float(base_qp)
            if qp_offsets is not None:                                          # :3682
                d_qp_offset, cnt = 0.0, 0
                block_yy = block_y
                while block_yy < block_y + block_size and block_yy < height:    # :3692
                    block_xx = block_x
                    while block_xx < block_x + block_size and block_xx < width:  # :3694
                        idx = (block_yy // loop_incr) * max_cols + block_xx // loop_incr
                        d_qp_offset += float(qp_offsets[idx])                   # :3697
                        cnt += 1
                        block_xx += loop_incr
                    block_yy += loop_incr
                d_qp_offset /= cnt                                              # :3701
                qp += d_qp_offset
            m_qp = min(max(int(qp + 0.5), qp_min), qp_max)                      # :3713 ((int) truncates towards zero, like int())
            ys, xs = slice(block_y // 8, (block_y + block_size) // 8), slice(block_x // 8, (block_x + block_size) // 8)
            cu[ys, xs] = m_qp
            tu[0, ys, xs] = m_qp + bd                                           # quant.cpp:224
            tu[1, ys, xs] = chroma(m_qp + cb_qp_offset)                         # :228
            tu[2, ys, xs] = chroma(m_qp + cr_qp_offset)                         # :229
    return cu, tu


# ------------------------------------------------------------------------------------------------ the synthetic map of the GPU tests
def map_values(depth):
    """Eight quantiser QPs: 0, the depth's maximum, every residue of 6 and eight different qp / 6."""
    bd = 6 * (depth - 8)
    return [0, 51 + bd, 7, 14 + bd // 2, 22 + bd // 2, 29 + bd, 35 + bd, 40 + bd]


def xcd_order(v, nblocks):
    """virtual index -> block of the uni-predictive 16 / 32 point kernels (xcd_swizzle of csrc/common.h)"""
    per = nblocks >> 3
    v = np.asarray(v)
    return np.where(v < (per << 3), (v & 7) * per + (v >> 3), v)


def block_qps(nblocks, grid, values, rng, swizzled):
    """One QP per block (index = ctu * blocks per CTU + z): `values` dealt evenly in random order, redrawn where block v + grid of a wavefront's walk
    would repeat the QP of block v.  swizzled: the walk visits xcd_order(v) at step v (the uni-predictive kernels), else block v."""
    k = len(values)
    pick = rng.permutation(np.arange(nblocks) % k)          # every value on the same share of the blocks, also where they are few
    for v in range(grid, nblocks):
        if pick[v] == pick[v - grid]:
            pick[v] = (pick[v] + 1 + int(rng.integers(0, k - 1))) % k
    qv = np.asarray(values, np.int64)[pick]
    out = np.zeros(nblocks, np.int64)
    out[xcd_order(np.arange(nblocks), nblocks) if swizzled else np.arange(nblocks)] = qv
    walk = out[xcd_order(np.arange(nblocks), nblocks)] if swizzled else out
    assert grid >= nblocks or (walk[grid:] != walk[:-grid]).all(), "a wavefront would meet the same QP in consecutive blocks"
    return out


def block_positions(width, height, level):
    """(px, py) luma sample of every block, index = ctu * blocks per CTU + z"""
    n = 8 << level
    npu = (64 // n) ** 2
    nb = (width // 64) * (height // 64) * npu
    b = np.arange(nb)
    ctu, z = b // npu, b % npu
    bx = (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4)
    by = ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)
    return (ctu % (width // 64)) * 64 + bx * n, (ctu // (width // 64)) * 64 + by * n


def cells_of_blocks(qpb, width, height, level):
    """The map the stages take - int8 [h/8, w/8], every 8x8 cell of a block holding its value - from one value per block."""
    px, py = block_positions(width, height, level)
    c = (8 << level) // 8
    m = np.zeros((height // 8, width // 8), np.int8)
    for dy in range(c):
        for dx in range(c):
            m[py // 8 + dy, px // 8 + dx] = qpb
    return m


def blocks_of_cells(cells, width, height, level):
    px, py = block_positions(width, height, level)
    return np.asarray(cells)[py // 8, px // 8].astype(np.int64)


def coverage(qpb, width, height, level, depth):
    """The conditions a map of the GPU tests has to meet; returns the smallest share of blocks any residue of 6 has."""
    q = np.asarray(qpb)
    shares = [float(np.mean(q % 6 == r)) for r in range(6)]
    assert min(shares) >= 0.03, f"residues of 6 on {shares} of the blocks"
    assert len(np.unique(q // 6)) >= 4, "fewer than four values of qp / 6"
    assert (q == 0).any() and (q == 51 + 6 * (depth - 8)).any(), "0 or the depth's maximum is missing"
    assert len(np.unique(q)) <= 8
    cells = cells_of_blocks(q, width, height, level)
    c = (8 << level) // 8
    blocks = cells[::c, ::c]
    assert (blocks[:, 1:] != blocks[:, :-1]).any() and (blocks[1:, :] != blocks[:-1, :]).any(), "no raster neighbours that differ"
    assert (q[1:] != q[:-1]).mean() > 0.5, "z-order neighbours mostly agree"
    return min(shares)


# ------------------------------------------------------------------------------------------------ inter stages: one oracle run per value
def compose(run, qpb, n, plane_cells, stride, org, pw, ph):
    """run(q) -> (recon plane, levels, num_sig, dist) of the oracle stage at uniform QP q; qpb: the QP of every block; n: the transform size
    (levels hold n * n entries per block); plane_cells: the block QP of every SAMPLE of the pw x ph plane the stage writes ([ph, pw]).
    Returns the same four arrays with every block taken from the run of its own QP (recon: the picture area; the rest from the first run,
    which no stage writes)."""
    rec = lev = ns = dist = None
    qpb = np.asarray(qpb)
    r0, c0 = divmod(org, stride)
    for q in np.unique(qpb):
        r, l, s, d = run(int(q))
        if rec is None:
            rec, lev, ns, dist = r.copy().reshape(-1), l.copy(), s.copy(), d.copy()
        sel = qpb == q
        lev.reshape(-1, n * n)[sel] = l.reshape(-1, n * n)[sel]
        ns[sel], dist[sel] = s[sel], d[sel]
        area = rec.reshape(-1, stride)[r0:r0 + ph, c0:c0 + pw]
        src = r.reshape(-1, stride)[r0:r0 + ph, c0:c0 + pw]
        m = plane_cells == q
        area[m] = src[m]
    return rec, lev, ns, dist


def sample_qps(cells, sub):
    """the block QP of every sample of a plane from the cell map: sub = 8 samples per cell for luma, 4 for a 4:2:0 chroma plane"""
    return np.kron(np.asarray(cells), np.ones((sub, sub), np.int8)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ I pictures: the walk with the block's own QPs
def walk(depth, planes, w64, h64, level, tu_qp, lambda8_by_qp=None, lambda8=1024, flags=H.TU_INTRA_SLICE, mode_bits=(2, 3, 6), strong=True,
         with_reference=False, recon_init=None):
    """intra_expect.expect with tu_qp int8 [3, h/8, w/8] (the quantiser QPs of Y, Cb, Cr per 8x8 cell of the luma grid) in place of one QP per
    plane, and the mode decision of a block priced with lambda8_by_qp[its luma quantiser QP] (None: lambda8).  4:2:0 chroma always."""
    import intra_expect as IE
    O = IE.O
    n = 8 << level
    bpc = 64 // n
    nblk = bpc * bpc
    cw, chh = w64 // 64, h64 // 64
    nctu = cw * chh
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    src = [np.ascontiguousarray(p).reshape(-1) for p in planes[:3]]
    init = recon_init if recon_init is not None else IE.garbage_planes(depth, [s.shape for s in src])
    rec = [np.array(p, copy=True).reshape(-1) for p in init]
    slots = IE.Slots(depth, n, with_reference)
    es = src[0].itemsize
    nc = n // 2
    tot = nctu * nblk
    mode_out = np.zeros(tot, np.uint8)
    cost_out = np.zeros((tot, 2), np.int32)
    lev = [np.zeros(tot * n * n, np.int16)] + [np.zeros(tot * nc * nc, np.int16) for _ in range(2)]
    ns = [np.zeros(tot, np.uint32) for _ in range(3)]
    dist = [np.zeros(tot, np.uint64) for _ in range(3)]
    lam_used = np.zeros(tot, np.int64)
    job = np.zeros(1, dtype=H.job_dtype())
    qmax = 51 + 6 * (depth - 8)
    for ctu in range(nctu):
        cx, cy = (ctu % cw) * 64, (ctu // cw) * 64
        for z in range(nblk):
            bx, by = IE.zorder(z)
            gx, gy = cx + bx * n, cy + by * n
            b = ctu * nblk + z
            qps = [min(max(int(tu_qp[c, gy // 8, gx // 8]), 0), qmax) for c in range(3)]
            lam = lambda8 if lambda8_by_qp is None else min(int(lambda8_by_qp[qps[0]]), 1 << 24)       # the stage prices an entry above 2^24 like 2^24
            lam_used[b] = lam
            flg = IE.neighbour_flags(gx, gy, n, w64, h64)
            off = org + gy * stride + gx
            ref_buf = IE.fill_reference_samples(rec[0], off, stride, flg, n, 4, depth)
            flt_buf, _ = IE.init_adi_pattern(ref_buf, n, depth, strong, slots)
            left = int(mode_out[IE.coding_index(gx - 1, gy, n, w64, nblk)]) if gx > 0 else 1
            above = int(mode_out[IE.coding_index(gx, gy - 1, n, w64, nblk)]) if by > 0 else 1
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
                    best = (cost, sad, mode)
            cost, sad, mode = best
            mode_out[b] = mode
            cost_out[b] = (sad, cost)
            nbs = np.concatenate([ref_buf, flt_buf])
            job["off"][0] = (off, 0, 4 * n + 1, 0)
            job["arg"][0, 0] = mode
            r, l, s_, d = O.intra_recon(depth, n, src[0], stride, nbs, n * n, n, qps[0], flags, job)
            rec[0].reshape(rows, stride)[F.MARGIN_Y + gy:F.MARGIN_Y + gy + n, F.MARGIN_X + gx:F.MARGIN_X + gx + n] = r.reshape(n, n)
            lev[0][b * n * n:(b + 1) * n * n], ns[0][b], dist[0][b] = l, s_[0], d[0]
            offc = oc + (gy // 2) * sc + gx // 2
            for c in range(2):
                cb = IE.fill_reference_samples(rec[1 + c], offc, sc, flg, nc, 2, depth)
                job["off"][0] = (offc, 0, 0, 0)
                r, l, s_, d = O.intra_recon(depth, nc, src[1 + c], sc, cb, nc * nc, nc, qps[1 + c], flags, job, chroma=True)
                y0, x0 = F.CHROMA_MARGIN_Y + gy // 2, F.CHROMA_MARGIN_X + gx // 2
                rec[1 + c].reshape(-1, sc)[y0:y0 + nc, x0:x0 + nc] = r.reshape(nc, nc)
                lev[1 + c][b * nc * nc:(b + 1) * nc * nc], ns[1 + c][b], dist[1 + c][b] = l, s_[0], d[0]
    out = dict(mode=mode_out, cost=cost_out, levels=lev[0], num_sig=ns[0], dist=dist[0], recon=rec[0], lambda8=lam_used)
    for c in range(2):
        out.update({"levels_c%d" % c: lev[1 + c], "num_sig_c%d" % c: ns[1 + c], "dist_c%d" % c: dist[1 + c], "recon_c%d" % c: rec[1 + c]})
    return out


def lambda8_table(depth):
    """A lambda8_by_qp table for the tests: floor(256 x 2^((qp - 12) / 6)) at the CU QP = quantiser QP - QP_BD_OFFSET, clipped at 0 - the closed
    form x265_lambda_tab (constants.cpp) is rounded from, as RDCost::setLambda floors it (rdcost.h:93-97).  A host passes its own table; the
    tests need distinct entries over the map's values."""
    import math
    bd = 6 * (depth - 8)
    return np.array([int(math.floor(256.0 * 2.0 ** ((max(q - bd, 0) - 12) / 6.0))) for q in range(52 + bd)], np.uint32)


# ------------------------------------------------------------------------------------------------ the steps' oracle chains under maps
def _composed(run, cells, w64, h64, level, chroma, stride, org):
    qpb = blocks_of_cells(cells, w64, h64, level)
    sub = 4 if chroma else 8
    return compose(run, qpb, sub << level, sample_qps(cells, sub), stride, org, w64 * sub // 8, h64 * sub // 8)


def p_chain(depth, cur_planes, ref_planes, w64, h64, rng_r, subme, level, qp, cu_qp, tu_qp, tu_flags=2, cores=0, avx2=False):
    """One P picture through the oracle under maps (the CPU twin of FramePipeline.run with chroma, deblocking, sign hiding, no SAO):
    *_planes = padded (Y [rows, stride], Cb, Cr) host planes; cu_qp [h/8, w/8], tu_qp [3, h/8, w/8].  Every stage output by name."""
    import oracle_api as O
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    cur, ref = cur_planes[0], ref_planes[0]
    _, mv = SC.search_head(depth, cur, ref, stride, org, w64, h64, rng_r, subme, cores=cores, avx2=avx2)
    out = {"subpel_mv": mv}
    rec, lev, ns, dist = _composed(lambda q: O.inter_recon(depth, cur, stride, org, ref, stride, org, w64, h64, level, mv, q, intra_slice=tu_flags,
                                                           nthreads=cores, avx2=avx2), tu_qp[0], w64, h64, level, False, stride, org)
    out.update({"levels": lev, "num_sig": ns, "dist": dist})
    crec = []
    for c in (1, 2):
        r, l, s, _ = _composed(lambda q: O.inter_recon_chroma(depth, cur_planes[c].reshape(-1), ref_planes[c].reshape(-1), sc, oc, w64, h64, level, mv, q,
                                                              intra_slice=tu_flags, nthreads=cores, avx2=avx2), tu_qp[c], w64, h64, level, True, sc, oc)
        crec.append(r)
        out["levels_c%d" % (c - 1)], out["num_sig_c%d" % (c - 1)] = l, s
    bv, bh = O.deblock_bs_inter(depth, w64, h64, level, mv, ns, avx2=avx2)
    return SC.filter_tail(out, depth, cur_planes, rec, crec, bv, bh, qp, w64, h64, cu_qp=cu_qp, sao=False, avx2=avx2)


def b_chain(depth, cur_planes, ref0_planes, ref1_planes, w64, h64, rng_r, subme, level, qp, cu_qp, tu_qp, tu_flags=2, cores=0, avx2=False):
    """One B picture under maps (the CPU twin of BFramePipeline.run with chroma, deblocking, sign hiding, no SAO); the decision is
    tests/bidir_expect.py's."""
    import bidir_expect as BE
    O = BE.O
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = SC.chroma_geometry(w64)
    cur, r0, r1 = cur_planes[0], ref0_planes[0], ref1_planes[0]
    nctu = (w64 // 64) * (h64 // 64)
    cq, qoff = F.qpel_cost_table(rng_r)
    recs = [SC.search_head(depth, cur, ref, stride, org, w64, h64, rng_r, subme, cores=cores, avx2=avx2)[1] for ref in (r0, r1)]
    phases = [BE.phases_of(depth, ref, stride) for ref in (r0, r1)]
    e = BE.expect(depth, cur, stride, org, w64, h64, level, recs, phases, cq, qoff, BE.DIR_COST, with_reference=False)
    mv0, mv1 = BE.full_mv_out(level, nctu, e["mv0"], 0), BE.full_mv_out(level, nctu, e["mv1"], 0)
    out = {"dir": e["dir"], "mv0_out": mv0, "mv1_out": mv1}
    rec, lev, ns, dist = _composed(lambda q: O.inter_recon_bi(depth, cur.reshape(-1), stride, org, r0.reshape(-1), r1.reshape(-1), w64, h64, level, mv0, mv1, q,
                                                              dir_flags=e["dir"], intra_slice=tu_flags, nthreads=cores, avx2=avx2),
                                   tu_qp[0], w64, h64, level, False, stride, org)
    out.update({"levels": lev, "num_sig": ns, "dist": dist})
    crec = []
    for c in (1, 2):
        r, l, s, _ = _composed(lambda q: O.inter_recon_chroma_bi(depth, cur_planes[c].reshape(-1), ref0_planes[c].reshape(-1), ref1_planes[c].reshape(-1), sc, oc,
                                                                 w64, h64, level, mv0, mv1, q, dir_flags=e["dir"], intra_slice=tu_flags, nthreads=cores, avx2=avx2),
                               tu_qp[c], w64, h64, level, True, sc, oc)
        crec.append(r)
        out["levels_c%d" % (c - 1)], out["num_sig_c%d" % (c - 1)] = l, s
    bv, bh = O.deblock_bs_b(depth, w64, h64, level, mv0, mv1, e["ref0"], e["ref1"], ns, slice_b=True, avx2=avx2)
    return SC.filter_tail(out, depth, cur_planes, rec, crec, bv, bh, qp, w64, h64, cu_qp=cu_qp, sao=False, avx2=avx2)


def i_chain(depth, planes, w64, h64, level, qp, cu_qp, tu_qp, lambda8_by_qp=None, tu_flags=H.TU_INTRA_SLICE | H.TU_SIGN_HIDE, avx2=False):
    """One I picture under maps (the CPU twin of IFramePipeline.run with chroma, deblocking, sign hiding, no SAO)."""
    import oracle_api as O
    nctu = (w64 // 64) * (h64 // 64)
    e = walk(depth, planes, w64, h64, level, tu_qp, lambda8_by_qp=lambda8_by_qp, flags=tu_flags)
    out = {k: e[k] for k in ("mode", "levels", "num_sig", "dist", "levels_c0", "levels_c1", "num_sig_c0", "num_sig_c1")}
    bv, bh = O.deblock_bs_inter(depth, w64, h64, level, np.zeros((nctu * 85, 2), np.int32), e["num_sig"], avx2=avx2, intra=np.ones(nctu * (64 >> (2 * level)), np.uint8))
    return SC.filter_tail(out, depth, planes, e["recon"], [e["recon_c0"], e["recon_c1"]], bv, bh, qp, w64, h64, cu_qp=cu_qp, sao=False, avx2=avx2)


def varied_clip(clip, depth):
    """The clip with the contrast of its 32x32 blocks (all three planes, every picture alike) scaled by 0.08 / 0.35 / 1 / 1.9 in turn: block
    energies that differ, so that adaptive quantisation at its default strength spreads the blocks over four or more QPs."""
    gains = np.array([0.08, 0.35, 1.0, 1.9])
    out = []
    for planes in clip:
        q = []
        for c, p in enumerate(planes):
            b = 32 if c == 0 else 16
            yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
            g = gains[((xx // b) + 2 * (yy // b)) % 4]
            m = float(1 << (depth - 1))
            q.append(np.clip(np.rint(m + (p.astype(np.float64) - m) * g), 0, (1 << depth) - 1).astype(p.dtype))
        out.append(tuple(q))
    return out


def step_outputs(pipe, dt, kind):
    """The chains' names from a FramePipeline ("p"), BFramePipeline ("b") or IFramePipeline ("i") after run() (chroma, deblocking, no SAO)."""
    g = lambda t: t.cpu().numpy()
    out = SC.step_outputs(pipe, dt)
    if kind == "i":
        out["mode"] = g(pipe.ip.mode)
    elif kind == "p":
        out["subpel_mv"] = g(pipe.sp.out).reshape(-1, 2)
    else:
        out.update({"dir": g(pipe.bd.dir), "mv0_out": g(pipe.bd.mv0_out).reshape(-1, 2), "mv1_out": g(pipe.bd.mv1_out).reshape(-1, 2)})
    return out
