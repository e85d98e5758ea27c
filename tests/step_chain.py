"""What the oracle chains of the tests/*_expect.py modules and their device readers share: one search head, one loop-filter tail, one
reader of a step's outputs and one builder of the SAO decision's host inputs.  A chain is one picture pushed stage by stage through
the oracle; the GPU step tests compare a step's outputs with it name by name (bidir_expect.compare).

bench.py's oracle_chain is the one copy of the tail left outside this module, on purpose: bench.py is how every change here is
measured, so it does not move with the tests' support code."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_api as O          # noqa: E402

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")


def sao_rdo_inputs(depth, qp, slice_type):
    """The host-side inputs of x265hip_sao_rdo at quantiser QP `qp` (a step's sao_rdo record); the SAO type context starts from the slice
    type's own state (HT.SLICE_I / SLICE_P / SLICE_B)."""
    tabs = HT.load()
    cu_qp = max(qp - 6 * (depth - 8), 0)
    cm, ct = HT.sao_contexts(slice_type, cu_qp)
    return {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}


def chroma_geometry(w64):
    """(stride, element offset of sample (0, 0)) of a padded 4:2:0 chroma plane"""
    sc = w64 // 2 + 2 * F.CHROMA_MARGIN_X
    return sc, F.CHROMA_MARGIN_Y * sc + F.CHROMA_MARGIN_X


def search_head(depth, cur, ref, stride, org, w64, h64, rng_r, subme, lam=4.0, cores=0, avx2=False):
    """cur searched in and refined against ref (padded host luma planes): (best uint64 [nctu * 85] of the full search, records
    {cost, qmvx | qmvy << 16} int32 [nctu * 85, 2] of the sub-pel refinement)."""
    nctu = (w64 // 64) * (h64 // 64)
    cost = F.mv_cost_table(rng_r, lam)
    cq, qoff = F.qpel_cost_table(rng_r, lam)
    _, best = O.me_fullsearch(depth, cur, stride, org, ref, stride, org, w64, h64, rng_r, 0, nctu, cost, cost, want_surf=False, nthreads=cores, avx2=avx2)
    return best, O.subpel_refine(depth, cur, stride, org, ref, stride, org, w64, h64, rng_r, 0, nctu, best, cq, qoff, subme, nthreads=cores, avx2=avx2)


def oracle_records(*args, **kw):
    """search_head's records alone"""
    return search_head(*args, **kw)[1]


def filter_tail(out, depth, src, rec, crec, bv, bh, qp, w64, h64, cu_qp=None, sao=True, sao_rdo=None, cores=0, avx2=False):
    """Everything behind the coding, the CPU twin of stages._PictureStep._filter_tail: luma and chroma deblocking, SAO (statistics of the
    three planes, x265hip_sao_rdo's decision or the distortion-only stand-in, application) unless sao=False, and the crop and edge pad
    that stands in for the border extension.  src: the padded source planes (Y, Cb, Cr); rec, crec: the coded luma plane and the coded
    (Cb, Cr) planes; bv, bh: the Bs maps; cu_qp: the CU QP map both deblocking calls read, or None; sao_rdo: the record a step takes, or
    None.  Writes bs_ver / bs_hor, the sao_* names and recon / recon_c0 / recon_c1 into `out` and returns it."""
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    sc, oc = chroma_geometry(w64)
    nctu = (w64 // 64) * (h64 // 64)
    flat = lambda p: np.ascontiguousarray(p).reshape(-1)
    cuqp = max(qp - 6 * (depth - 8), 0)
    cu_map = None if cu_qp is None else np.ascontiguousarray(cu_qp, np.int8)
    out.update({"bs_ver": bv, "bs_hor": bh})
    dbk = O.deblock_luma(depth, flat(rec), stride, org, w64, h64, bv, bh, cuqp, qp_map=cu_map, avx2=avx2)
    cdb = O.deblock_chroma(depth, flat(crec[0]), flat(crec[1]), sc, oc, w64, h64, bv, bh, cuqp, qp_map=cu_map, avx2=avx2)
    fin, cfin = dbk, cdb
    if sao:
        cnt, off = O.sao_stats(depth, flat(src[0]), dbk.reshape(-1), stride, org, w64, h64, nthreads=cores, avx2=avx2)
        cstat = [O.sao_stats(depth, flat(src[1 + i]), cdb[i].reshape(-1), sc, oc, w64 // 2, h64 // 2, nthreads=cores, avx2=avx2, ctu=(32, 32), plane_offset=2)
                 for i in range(2)]
        if sao_rdo is not None:
            lam = np.tile(np.array(sao_rdo["lambdas"], np.int64), (nctu, 1))
            pars, _ = O.sao_rdo(depth, [cnt, cstat[0][0], cstat[1][0]], [off, cstat[0][1], cstat[1][1]], w64 // 64, h64 // 64, lam, sao_rdo["ctx_merge"],
                                sao_rdo["ctx_type"], sao_rdo["entropy_bits"], avx2=avx2)
            par, cpars = pars[0].reshape(-1), [pars[1].reshape(-1), pars[2].reshape(-1)]
        else:
            _, par = O.sao_decide(depth, cnt, off, avx2=avx2)
            cpars = [O.sao_decide(depth, cstat[i][0], cstat[i][1], avx2=avx2)[1] for i in range(2)]
        fin = O.sao_apply(depth, dbk.reshape(-1), stride, org, w64, h64, par, nthreads=cores, avx2=avx2)
        cfin = [O.sao_apply(depth, cdb[i].reshape(-1), sc, oc, w64 // 2, h64 // 2, cpars[i], nthreads=cores, avx2=avx2, ctu=(32, 32)) for i in range(2)]
        out.update({"sao_count": cnt, "sao_offset_org": off, "sao_params": par})
        for i in range(2):
            out["sao_count_c%d" % i], out["sao_params_c%d" % i] = cstat[i][0], cpars[i]
    inner = fin.reshape(rows, stride)[F.MARGIN_Y:F.MARGIN_Y + h64, F.MARGIN_X:F.MARGIN_X + w64]
    out["recon"] = np.pad(inner, ((F.MARGIN_Y, F.MARGIN_Y), (F.MARGIN_X, F.MARGIN_X)), mode="edge")
    for i in range(2):
        ci = cfin[i].reshape(-1, sc)[F.CHROMA_MARGIN_Y:F.CHROMA_MARGIN_Y + h64 // 2, F.CHROMA_MARGIN_X:F.CHROMA_MARGIN_X + w64 // 2]
        out["recon_c%d" % i] = np.pad(ci, ((F.CHROMA_MARGIN_Y, F.CHROMA_MARGIN_Y), (F.CHROMA_MARGIN_X, F.CHROMA_MARGIN_X)), mode="edge")
    return out


def step_outputs(pipe, dt):
    """What every stages._PictureStep owns after run(), under the chains' names: the TU stages' levels, numSig and SSE of Y, Cb, Cr (the
    I step's from pipe.ip), the Bs maps, the SAO buffers where the step has SAO, and the final planes viewed as dt.  The decision stages'
    names are the caller's to add."""
    g = lambda t: t.cpu().numpy()
    if hasattr(pipe, "ip"):
        tu, tc = pipe.ip, [(pipe.ip.levels_c[i], pipe.ip.num_sig_c[i], pipe.ip.dist_c[i]) for i in range(2)]
    else:
        tu, tc = pipe.rc, [(pipe.rc_c[i].levels, pipe.rc_c[i].num_sig, pipe.rc_c[i].dist) for i in range(2)]
    out = {"levels": g(tu.levels), "num_sig": g(tu.num_sig), "dist": g(tu.dist), "bs_ver": g(pipe.db.bs_ver), "bs_hor": g(pipe.db.bs_hor),
           "recon": g(pipe.final).view(dt)}
    if pipe.sao is not None:
        out.update({"sao_count": g(pipe.sao.count), "sao_offset_org": g(pipe.sao.offset_org), "sao_params": g(pipe.sao.params)})
    for i in range(2):
        out["levels_c%d" % i], out["num_sig_c%d" % i], out["dist_c%d" % i] = (g(t) for t in tc[i])
        if pipe.sao is not None:
            out["sao_count_c%d" % i], out["sao_params_c%d" % i] = g(pipe.sao_c[i].count), g(pipe.sao_c[i].params)
        out["recon_c%d" % i] = g(pipe.final_c[i]).view(dt)
    return out
