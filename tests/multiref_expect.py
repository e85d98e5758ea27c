"""Expected results of the P step with several references (x265hip_ref_select, x265hip_inter_recon_refs and the chroma entries,
stages.MultiRefFramePipeline), assembled from the oracle's pieces.

The selection is not a function of the oracle library: the records per reference come from O.me_fullsearch + O.subpel_refine, and what
remains is the addition and the strict comparison of Search::predInterSearch's uni-directional loop (search.cpp:2403-2404, 2457).  The
reconstruction of block b is block b of O.inter_recon / O.inter_recon_chroma run over the whole picture against reference ref_idx[b]:
blocks of the inter TU stage are independent of each other."""
import functools
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_api as O          # noqa: E402
import bidir_expect as BE       # noqa: E402
import qp_map_expect as QE      # noqa: E402
import step_chain as SC         # noqa: E402

F = importlib.import_module("x265-yuuki-asuna_amd.frames")

LEVEL_BASE = (0, 64, 80)
MASKS = ("ref0", "ref1", "ref2", "ref3", "tie", "tie_not_ref0", "bias_decides")
COST_DEFAULT, COST_FLAT, COST_REVERSED = (12, 16, 20, 20), (8, 8, 8, 8), (192, 128, 64, 0)


def ref_cost_bits(nrefs, lam=4):
    """lambda x (m_listSelBits[0] + MVP_IDX_BITS + getTUBits(r, nrefs)) (search.cpp:2403-2404, search.h:246-249)"""
    return tuple(lam * (1 + 1 + r + (1 if r < nrefs - 1 else 0)) for r in range(nrefs))


def five_ref_lumas(depth, w=768, h=192, seed=31):
    """(cur, [refs 0 .. 3]) luma pictures, nearest reference first, in six vertical stripes: (0) plain motion, (1 - 3) only reference
    1 / 2 / 3 shows the clip's content, (4) all four references equal the current picture (equal costs: ties), (5) reference 3 is a copy
    of reference 1 and references 0 / 2 show other content (a tie the first reference takes no part in)."""
    clip = F.synth_clip(w, h, 5, depth=depth, seed=seed)
    other = F.synth_clip(w, h, 5, depth=depth, seed=seed + 1000)
    cur = clip[4][0].copy()
    refs = [clip[3 - k][0].copy() for k in range(4)]
    q = w // 6
    for s in (1, 2, 3):
        for k in range(4):
            if k != s:
                refs[k][:, s * q:(s + 1) * q] = other[k][0][:, s * q:(s + 1) * q]
    for k in range(4):
        refs[k][:, 4 * q:5 * q] = cur[:, 4 * q:5 * q]
    refs[3][:, 5 * q:] = refs[1][:, 5 * q:]
    refs[0][:, 5 * q:] = other[0][0][:, 5 * q:]
    refs[2][:, 5 * q:] = other[2][0][:, 5 * q:]
    return cur, refs


def select(level, nctu, recs, ref_cost, ref_ids=None):
    """The selection for every block of `level`: recs = the records [nctu * 85, 2] per reference, list order.  Returns dict: ref_idx /
    ref_id int8 [nctu * nb], mv_out int32 [nctu * nb, 2] (the level's entries, block order), cost int32 [nctu * nb, nrefs] and the masks."""
    nb, base = (64 >> (3 + level)) ** 2, LEVEL_BASE[level]
    n = len(recs)
    ids = np.arange(n) if ref_ids is None else np.asarray(ref_ids)
    lvl = [np.asarray(r, np.int32).reshape(nctu, 85, 2)[:, base:base + nb].reshape(-1, 2) for r in recs]
    raw = np.stack([r[:, 0] for r in lvl], axis=1).astype(np.int64)
    cost = raw + np.asarray(ref_cost, np.int64)[None, :n]
    idx = np.zeros(len(cost), np.int64)
    best = cost[:, 0].copy()
    for r in range(1, n):                                   # strict '<' in list order (search.cpp:2457)
        better = cost[:, r] < best
        idx[better], best[better] = r, cost[better, r]
    words = np.stack([r[:, 1] for r in lvl], axis=1)
    rows = np.arange(len(cost))
    mv_out = np.stack([best.astype(np.int32), words[rows, idx]], axis=1)
    at_min = (cost == best[:, None]).sum(axis=1)
    masks = {"ref%d" % r: idx == r for r in range(4)}
    masks["tie"] = at_min >= 2
    masks["tie_not_ref0"] = masks["tie"] & (idx != 0)
    masks["bias_decides"] = np.argmin(raw, axis=1) != idx
    return dict(ref_idx=idx.astype(np.int8), ref_id=ids[idx].astype(np.int8), mv_out=mv_out, cost=cost.astype(np.int32), masks=masks)


def full_mv_out(level, nctu, level_entries, prefill):
    return BE.full_mv_out(level, nctu, level_entries, prefill)


def _per_block(run, ref_idx, w64, h64, level, chroma, stride, org, qp_cells=None):
    """Every block taken from run(r, q): the oracle stage over the whole picture against reference r at QP q (q = None without a map)."""
    sub = 4 if chroma else 8
    key = np.asarray(ref_idx, np.int64)
    cells = QE.cells_of_blocks(key, w64, h64, level).astype(np.int64)
    if qp_cells is not None:
        key = key * 256 + QE.blocks_of_cells(qp_cells, w64, h64, level)
        cells = cells * 256 + np.asarray(qp_cells, np.int64)
    samples = np.kron(cells, np.ones((sub, sub), np.int64))
    call = lambda k: run(int(k) // 256, int(k) % 256) if qp_cells is not None else run(int(k), None)
    return QE.compose(call, key, sub << level, samples, stride, org, w64 * sub // 8, h64 * sub // 8)


def recon_luma(depth, cur, refs, stride, org, w64, h64, level, mv, ref_idx, qp, flags, qp_cells=None, nthreads=0):
    """(recon plane, levels, num_sig, dist) of x265hip_inter_recon_refs: padded luma planes, mv [nctu * 85, 2], ref_idx per block."""
    run = lambda r, q: O.inter_recon(depth, cur, stride, org, refs[r], stride, org, w64, h64, level, mv, qp if q is None else q, intra_slice=flags,
                                     nthreads=nthreads)
    return _per_block(run, ref_idx, w64, h64, level, False, stride, org, qp_cells)


def recon_chroma(depth, cur, refs, stride, org, w64, h64, level, mv, ref_idx, qp, flags, qp_cells=None, nthreads=0):
    """The same for one chroma plane (flat padded planes, sample (0,0) at element org)."""
    run = lambda r, q: O.inter_recon_chroma(depth, cur.reshape(-1), refs[r].reshape(-1), stride, org, w64, h64, level, mv, qp if q is None else q,
                                            intra_slice=flags, nthreads=nthreads)
    return _per_block(run, ref_idx, w64, h64, level, True, stride, org, qp_cells)


class FiveRef:
    """The six-stripe case on the host: padded planes and every reference's records."""

    def __init__(self, depth, subme, rng_r=12, w=768, h=192, seed=31, lam=4.0):
        self.depth, self.subme, self.range = depth, subme, rng_r
        cur, refs = five_ref_lumas(depth, w, h, seed)
        self.cur, self.stride, self.org, self.w64, self.h64 = F.pad_plane(cur)
        self.refs = [F.pad_plane(r)[0] for r in refs]
        self.nctu = (self.w64 // 64) * (self.h64 // 64)
        self.recs = [BE.oracle_records(depth, self.cur, r, self.stride, self.org, self.w64, self.h64, rng_r, subme, lam) for r in self.refs]

    def expect(self, level, ref_cost=COST_DEFAULT, nrefs=4, ref_ids=None):
        """nrefs 8: the four planes twice"""
        recs = (self.recs * 2)[:nrefs]
        return select(level, self.nctu, recs, ref_cost, ref_ids)


@functools.lru_cache(maxsize=None)
def five_ref(depth, subme):
    """shared: read only"""
    return FiveRef(depth, subme)


def p_chain_refs(depth, cur_planes, refs_planes, w64, h64, rng_r, subme, level, qp, sao_rdo=None, ref_cost=None, tu_flags=2, chroma_satd=False,
                 cu_qp=None, tu_qp=None, sao=True, cores=0):
    """One P picture with several references through the oracle, stage by stage (the CPU twin of stages.MultiRefFramePipeline.run with
    chroma, deblocking and - unless sao=False - SAO applied): cur_planes = padded (Y [rows, stride], Cb, Cr) host planes, refs_planes = the
    same per reference, nearest first.  chroma_satd: the records are the chroma walk's (tests/subpel_chroma_expect.py).  cu_qp / tu_qp: the
    maps of a CuQpMaps.  Returns every stage output by name."""
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    cur = cur_planes[0]
    nctu = (w64 // 64) * (h64 // 64)
    n = len(refs_planes)
    out, recs = {}, []
    for r, ref in enumerate(refs_planes):
        if chroma_satd and subme >= 3:
            import subpel_chroma_cases as CC
            import subpel_chroma_expect as SE
            mv = SE.walk(CC.refine_inputs(depth, rng_r, cur_planes, ref, w64, h64), subme, with_reference=False)["rec"]
        else:
            mv = BE.oracle_records(depth, cur, ref[0], stride, org, w64, h64, rng_r, subme)
        out["subpel_mv%d" % r] = mv
        recs.append(mv)
    e = select(level, nctu, recs, ref_cost_bits(n) if ref_cost is None else ref_cost)
    mv = full_mv_out(level, nctu, e["mv_out"], 0)
    out.update({"ref_idx": e["ref_idx"], "ref_id": e["ref_id"], "mv_out": mv, "cost_out": e["cost"]})
    cells = (lambda c: None if tu_qp is None else np.asarray(tu_qp)[c])
    rec, lev, ns, dist = recon_luma(depth, cur, [p[0] for p in refs_planes], stride, org, w64, h64, level, mv, e["ref_idx"], qp, tu_flags, cells(0), cores)
    out.update({"levels": lev, "num_sig": ns, "dist": dist})
    bv, bh = O.deblock_bs_b(depth, w64, h64, level, mv, None, e["ref_id"], None, ns, slice_b=False)
    sc, oc = SC.chroma_geometry(w64)
    qpc = S.chroma_quant_qp(qp, depth)
    crec = [recon_chroma(depth, cur_planes[c], [p[c] for p in refs_planes], sc, oc, w64, h64, level, mv, e["ref_idx"], qpc, tu_flags, cells(c), cores)
            for c in (1, 2)]
    for i in range(2):
        out["levels_c%d" % i], out["num_sig_c%d" % i] = crec[i][1], crec[i][2]
    return SC.filter_tail(out, depth, cur_planes, rec, [crec[0][0], crec[1][0]], bv, bh, qp, w64, h64, cu_qp=cu_qp, sao=sao, sao_rdo=sao_rdo, cores=cores)


def device_outputs(pipe, dt, nrefs):
    """The same names from a stages.MultiRefFramePipeline after run() (chroma, deblocking, want_cost; the SAO names where it has SAO)."""
    g = lambda t: t.cpu().numpy()
    out, rs = SC.step_outputs(pipe, dt), pipe.rs
    out.update({"subpel_mv%d" % r: g(pipe.spl[r].out).reshape(-1, 2) for r in range(nrefs)})
    out.update({"ref_idx": g(rs.ref_idx), "ref_id": g(rs.ref_id), "mv_out": g(rs.mv_out).reshape(-1, 2),
                "cost_out": g(rs.cost_out)[:rs.nctu * rs.nblk * nrefs].reshape(-1, nrefs)})
    return out
