"""Expected results of the B step with several references per list (x265hip_bidir_decide_refs, x265hip_inter_recon_bi_refs and the
chroma entry, stages.MultiRefBFramePipeline), assembled from the oracle's pieces on top of tests/bidir_expect.py and
tests/multiref_expect.py as they are.

Records per reference come from O.me_fullsearch + O.subpel_refine; the per-list selection is multiref_expect.select (additions and a
strict comparison); the decision is the handful of additions and comparisons of Search::predInterSearch (search.cpp:2473-2640) with
O.phase_planes for predInterLumaPixel's samples and the table's pixelavg_pp / satd slots, each block against the two pictures it chose;
the reconstruction of block b is block b of O.inter_recon_bi / O.inter_recon_chroma_bi run over the whole picture for each pair of list
indices that occurs."""
import functools
import importlib

import numpy as np

import bidir_expect as BE
import multiref_expect as ME

O = BE.O
F = BE.F
SC = BE.SC

LEVEL_BASE = BE.LEVEL_BASE
DIR_COST = BE.DIR_COST
COST_HEAVY = ((40, 56), (40, 56))          # reference bits large enough to turn decisions at every level (the default (8, 8) does at some)
OUTCOMES = ("dir1", "dir2", "dir3_refined", "dir3_zero", "dir3_both_far", "tie01", "l0_ref0", "l0_ref1", "l1_ref0", "l1_ref1")


def b_ref_cost_bits(nrefs, lam=4):
    """lambda x (MVP_IDX_BITS + getTUBits(r, nrefs)) of one list of a B slice (search.cpp:2403-2404 without the list-selection bits)"""
    return tuple(lam * (1 + r + (1 if r < nrefs - 1 else 0)) for r in range(nrefs))


def stripe_lumas(depth, w=768, h=192, seed=51):
    """(cur, [list 0: A0, A1], [list 1: B0, B1]) luma pictures in eight vertical stripes: (0) plain motion in all four references, each
    with noise of its own, (1 - 4) only A0 / A1 / B0 / B1 shows the clip's content, (5) flat + noise everywhere (spurious vectors: the zero candidate competes), (6)
    opposite patterns in A1 and B1 that only the coincident average cancels, with louder noise in A0 and B0 (a bidirectional block with
    both indices > 0), (7) four copies of the current picture (zero vectors, equal costs in and between the lists)."""
    clip = F.synth_clip(w, h, 5, depth=depth, seed=seed)
    other = F.synth_clip(w, h, 5, depth=depth, seed=seed + 1000)
    cur = clip[2][0].copy()
    refs = [clip[1][0].copy(), clip[0][0].copy(), clip[3][0].copy(), clip[4][0].copy()]          # A0, A1, B0, B1
    src = (1, 0, 3, 4)
    r = np.random.default_rng([seed, depth])
    q = w // 8
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = cur.dtype
    for s in (1, 2, 3, 4):
        for k in range(4):
            if k != s - 1:
                refs[k][:, s * q:(s + 1) * q] = other[src[k]][0][:, s * q:(s + 1) * q]
    noise = lambda sigma: np.clip(np.rint(128 * sc + r.normal(0, sigma * sc, size=(h, q))), 0, mx).astype(dt)
    for k in range(4):          # independent noise on the plain-motion stripe: the average of two references is the better prediction
        refs[k][:, :q] = np.clip(np.rint(refs[k][:, :q] + r.normal(0, 6.0 * sc, size=(h, q))), 0, mx).astype(dt)
    cur[:, 5 * q:6 * q] = noise(3.0)
    for k in range(4):
        refs[k][:, 5 * q:6 * q] = noise(3.0)
    E = np.rint(r.normal(0, 20.0 * sc, size=(h, q)))
    cur[:, 6 * q:7 * q] = noise(1.0)
    refs[1][:, 6 * q:7 * q] = np.clip(128 * sc + E, 0, mx).astype(dt)
    refs[3][:, 6 * q:7 * q] = np.clip(128 * sc - E, 0, mx).astype(dt)
    refs[0][:, 6 * q:7 * q] = noise(60.0)
    refs[2][:, 6 * q:7 * q] = noise(60.0)
    for k in range(4):
        refs[k][:, 7 * q:] = cur[:, 7 * q:]
    return cur, refs[:2], refs[2:]


def decide(depth, cur, stride, org, w64, h64, level, mv0, mv1, idx0, idx1, phases0, phases1, ref_cost0, ref_cost1, cq, qoff, dir_cost=DIR_COST,
           ref_ids0=None, ref_ids1=None, with_reference=True):
    """The decision for every block of `level`.  mv0 / mv1: the two selections' records [nctu * 85, 2] ({cost incl. ref_cost, vector});
    idx0 / idx1: list index per block (clamped here like the kernel clamps); phases0 / phases1: BE.phases_of() per reference of each list.
    Returns dict: dir uint8 [nctu * nb], ref0 / ref1 int8, mv0 / mv1 int32 [nctu * nb, 2] (the level's entries, block order), cost int32
    [nctu * nb, 4], dir_rb0 (the dir with rb = 0) and the boolean masks dir1 / dir2 / dir3_refined / dir3_zero / tie01."""
    n, nb, base = 8 << level, (64 >> (3 + level)) ** 2, LEVEL_BASE[level]
    cw = w64 // 64
    nctu = cw * (h64 // 64)
    slots = BE.Slots(depth, n, with_reference)
    es = cur.itemsize
    tot = nctu * nb
    phases, costs = (phases0, phases1), (ref_cost0, ref_cost1)
    ids = (list(range(len(phases0))) if ref_ids0 is None else list(ref_ids0), list(range(len(phases1))) if ref_ids1 is None else list(ref_ids1))
    idx = [np.clip(np.asarray(i, np.int64), 0, len(ph) - 1) for i, ph in zip((idx0, idx1), phases)]
    recs = (np.asarray(mv0).reshape(-1, 2), np.asarray(mv1).reshape(-1, 2))
    d, d_rb0 = np.zeros(tot, np.uint8), np.zeros(tot, np.uint8)
    ref0, ref1 = np.zeros(tot, np.int8), np.zeros(tot, np.int8)
    mvo = [np.zeros((tot, 2), np.int32), np.zeros((tot, 2), np.int32)]
    cost = np.zeros((tot, 4), np.int32)
    masks = {k: np.zeros(tot, bool) for k in ("dir1", "dir2", "dir3_refined", "dir3_zero", "tie01")}
    cqi = cq.astype(np.int64)

    def choose(cref, cz, tried, cl, words):
        cbi, m = cref, list(words)
        if tried and cz < cbi:
            cbi, m = cz, [0, 0]
        return (3 if (cbi < cl[0] and cbi < cl[1]) else (1 if cl[0] <= cl[1] else 2)), cbi, m
    for ctu in range(nctu):
        cx, cy = (ctu % cw) * 64, (ctu // cw) * 64
        for z in range(nb):
            bx, by = BE.zorder(z)
            off = org + (cy + by * n) * stride + cx + bx * n           # element offset of the block in every padded plane
            b = ctu * nb + z
            ptrs, zptrs, mvc, words, cl, rb = [], [], [], [], [], 0
            for l in (0, 1):
                c, word = recs[l][ctu * 85 + base + z]
                i = int(idx[l][b])
                ph = phases[l][i]
                qx, qy = BE.unpack_mv(word)
                p = (qy & 3) * 4 + (qx & 3)
                ptrs.append(ph.ctypes.data + ((p * ph.shape[1] * stride) + off + (qy >> 2) * stride + (qx >> 2)) * es)
                zptrs.append(ph.ctypes.data + off * es)
                mvc.append(int(cqi[qoff + qx]) + int(cqi[qoff + qy]))
                words.append(int(word))
                cl.append(int(c) + dir_cost[l])
                rb += int(costs[l][i])
            fp = cur.ctypes.data + off * es
            sbi = slots.satd_of_average(fp, stride, ptrs[0], ptrs[1], stride) + mvc[0] + mvc[1] + dir_cost[2]
            tried = words[0] != 0 or words[1] != 0
            sz = slots.satd_of_average(fp, stride, zptrs[0], zptrs[1], stride) + 4 * int(cqi[qoff]) + dir_cost[2] if tried else None
            cref, cz = sbi + rb, (sz + rb if tried else -1)
            dd, cbi, m = choose(cref, cz, tried, cl, words)
            d_rb0[b] = choose(sbi, sz if tried else -1, tried, cl, words)[0]
            d[b] = dd
            ref0[b] = ids[0][int(idx[0][b])] if dd & 1 else -1
            ref1[b] = ids[1][int(idx[1][b])] if dd & 2 else -1
            if dd == 3:
                mvo[0][b], mvo[1][b] = (cbi, m[0]), (cbi, m[1])
            else:
                mvo[0][b] = (cl[0], m[0] if dd == 1 else 0)
                mvo[1][b] = (cl[1], m[1] if dd == 2 else 0)
            cost[b] = (cl[0], cl[1], cref, cz)
            masks["dir1"][b], masks["dir2"][b] = dd == 1, dd == 2
            masks["dir3_refined"][b] = dd == 3 and not (tried and cz < cref)
            masks["dir3_zero"][b] = dd == 3 and tried and cz < cref
            masks["tie01"][b] = cl[0] == cl[1]
    return dict(dir=d, ref0=ref0, ref1=ref1, mv0=mvo[0], mv1=mvo[1], cost=cost, dir_rb0=d_rb0, masks=masks, tables=slots.tables)


def expect(depth, cur, stride, org, w64, h64, level, recs0, recs1, phases0, phases1, cq, qoff, ref_cost0=None, ref_cost1=None, dir_cost=DIR_COST,
           ref_ids0=None, ref_ids1=None, with_reference=True):
    """Both stages: the per-list selection (ME.select) and the decision.  recs_l: every reference's records of list l.  Returns the
    decision's dict + sel0 / sel1 (ME.select's dicts), mv_in0 / mv_in1 (the selections' whole mv_out buffers, other levels 0) and the
    masks of OUTCOMES."""
    nctu = (w64 // 64) * (h64 // 64)
    rc = (b_ref_cost_bits(len(recs0)) if ref_cost0 is None else tuple(ref_cost0), b_ref_cost_bits(len(recs1)) if ref_cost1 is None else tuple(ref_cost1))
    sel = [ME.select(level, nctu, recs, c, ids) for recs, c, ids in ((recs0, rc[0], ref_ids0), (recs1, rc[1], ref_ids1))]
    mv_in = [BE.full_mv_out(level, nctu, s["mv_out"], 0) for s in sel]
    e = decide(depth, cur, stride, org, w64, h64, level, mv_in[0], mv_in[1], sel[0]["ref_idx"], sel[1]["ref_idx"], phases0, phases1, rc[0], rc[1], cq, qoff,
               dir_cost, ref_ids0, ref_ids1, with_reference)
    i0, i1 = sel[0]["ref_idx"], sel[1]["ref_idx"]
    m = e["masks"]
    m["dir3_both_far"] = (e["dir"] == 3) & (i0 > 0) & (i1 > 0)
    for l, i in ((0, i0), (1, i1)):
        for r in (0, 1):
            m["l%d_ref%d" % (l, r)] = i == r
    e.update(sel0=sel[0], sel1=sel[1], mv_in0=mv_in[0], mv_in1=mv_in[1], ref_cost=rc)
    return e


class Stripes:
    """The eight-stripe case on the host: padded planes, every reference's records and phases.  nrefs: (list 0, list 1) up to (2, 2)."""

    def __init__(self, depth, subme, rng_r=12, w=768, h=192, seed=51, lam=4.0):
        self.depth, self.subme, self.range = depth, subme, rng_r
        cur, l0, l1 = stripe_lumas(depth, w, h, seed)
        self.cur, self.stride, self.org, self.w64, self.h64 = F.pad_plane(cur)
        self.refs = ([F.pad_plane(y)[0] for y in l0], [F.pad_plane(y)[0] for y in l1])
        self.nctu = (self.w64 // 64) * (self.h64 // 64)
        self.cq, self.qoff = F.qpel_cost_table(rng_r, lam)
        self.recs = tuple([BE.oracle_records(depth, self.cur, r, self.stride, self.org, self.w64, self.h64, rng_r, subme, lam) for r in refs] for refs in self.refs)
        self.phases = tuple([BE.phases_of(depth, r, self.stride) for r in refs] for refs in self.refs)

    def lists(self, nrefs):
        """(planes, records, phases) of each list cut to nrefs = (n0, n1); n up to 4 repeats the list's two pictures"""
        cut = lambda x, l: (x[l] * 2)[:nrefs[l]]
        return tuple((cut(self.refs, l), cut(self.recs, l), cut(self.phases, l)) for l in range(2))

    def expect(self, level, nrefs=(2, 2), **kw):
        (_, r0, p0), (_, r1, p1) = self.lists(nrefs)
        return expect(self.depth, self.cur, self.stride, self.org, self.w64, self.h64, level, r0, r1, p0, p1, self.cq, self.qoff, **kw)


@functools.lru_cache(maxsize=None)
def stripes(depth, subme=3):
    """shared: read only"""
    return Stripes(depth, subme)


def _per_pair(run, idx0, idx1, dirs, w64, h64, level, chroma, stride, org, qp_cells=None):
    """Every block taken from run(i0, i1, q): the oracle's bi-predictive stage over the whole picture against the pair of references
    (list 0 index i0, list 1 index i1).  The index of a list a block does not use is replaced by 0: it must not matter."""
    i0 = np.where(np.asarray(dirs) & 1, np.asarray(idx0, np.int64), 0)
    i1 = np.where(np.asarray(dirs) & 2, np.asarray(idx1, np.int64), 0)
    return ME._per_block(lambda k, q: run(k // 8, k % 8, q), i0 * 8 + i1, w64, h64, level, chroma, stride, org, qp_cells)


def recon_luma(depth, cur, refs0, refs1, stride, org, w64, h64, level, mv0, mv1, idx0, idx1, dirs, qp, flags, qp_cells=None, nthreads=0):
    """(recon plane, levels, num_sig, dist) of x265hip_inter_recon_bi_refs: padded luma planes, records [nctu * 85, 2], indices (already
    inside their lists) and dir per block."""
    run = lambda a, b, q: O.inter_recon_bi(depth, cur.reshape(-1), stride, org, refs0[a].reshape(-1), refs1[b].reshape(-1), w64, h64, level, mv0, mv1,
                                           qp if q is None else q, dir_flags=dirs, intra_slice=flags, nthreads=nthreads)
    return _per_pair(run, idx0, idx1, dirs, w64, h64, level, False, stride, org, qp_cells)


def recon_chroma(depth, cur, refs0, refs1, stride, org, w64, h64, level, mv0, mv1, idx0, idx1, dirs, qp, flags, qp_cells=None, nthreads=0):
    """The same for one chroma plane (flat padded planes, sample (0,0) at element org)."""
    run = lambda a, b, q: O.inter_recon_chroma_bi(depth, cur.reshape(-1), refs0[a].reshape(-1), refs1[b].reshape(-1), stride, org, w64, h64, level, mv0, mv1,
                                                  qp if q is None else q, dir_flags=dirs, intra_slice=flags, nthreads=nthreads)
    return _per_pair(run, idx0, idx1, dirs, w64, h64, level, True, stride, org, qp_cells)


def b_chain_refs(depth, cur_planes, refs0_planes, refs1_planes, w64, h64, rng_r, subme, level, qp, sao_rdo=None, dir_cost=DIR_COST, ref_cost=None,
                 ref_ids=None, tu_flags=2, cu_qp=None, tu_qp=None, sao=True, cores=0):
    """One B picture with several references per list through the oracle, stage by stage (the CPU twin of
    stages.MultiRefBFramePipeline.run with chroma, deblocking and - unless sao=False - SAO applied).  *_planes: padded (Y [rows, stride],
    Cb, Cr) host planes, refs*_planes one triple per reference in list order; a picture in both lists is the same triple (object).
    ref_ids: (list 0, list 1) or None = the place among the distinct pictures, as the step derives them."""
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    _, _, stride, rows, org = F.padded_dims(w64, h64)
    cur = cur_planes[0]
    nctu = (w64 // 64) * (h64 // 64)
    cq, qoff = F.qpel_cost_table(rng_r)
    lists = (list(refs0_planes), list(refs1_planes))
    distinct = []
    for ref in lists[0] + lists[1]:
        if not any(ref is d for d in distinct):
            distinct.append(ref)
    slots = [[next(i for i, d in enumerate(distinct) if d is ref) for ref in lists[l]] for l in range(2)]
    ids = slots if ref_ids is None else ref_ids
    out, recs, phases = {}, [], []
    for s, ref in enumerate(distinct):
        recs.append(BE.oracle_records(depth, cur, ref[0], stride, org, w64, h64, rng_r, subme))
        phases.append(BE.phases_of(depth, ref[0], stride))
        out["subpel_mv%d" % s] = recs[-1]
    rc = ref_cost or (None, None)
    e = expect(depth, cur, stride, org, w64, h64, level, [recs[s] for s in slots[0]], [recs[s] for s in slots[1]], [phases[s] for s in slots[0]],
               [phases[s] for s in slots[1]], cq, qoff, rc[0], rc[1], dir_cost, ids[0], ids[1], with_reference=False)
    del phases
    mv0, mv1 = BE.full_mv_out(level, nctu, e["mv0"], 0), BE.full_mv_out(level, nctu, e["mv1"], 0)
    i0, i1, dirs = e["sel0"]["ref_idx"], e["sel1"]["ref_idx"], e["dir"]
    out.update({"ref_idx0": i0, "ref_idx1": i1, "sel_mv0": e["mv_in0"], "sel_mv1": e["mv_in1"], "dir": dirs, "ref0": e["ref0"], "ref1": e["ref1"],
                "mv0_out": mv0, "mv1_out": mv1, "cost_out": e["cost"]})
    cells = (lambda c: None if tu_qp is None else np.asarray(tu_qp)[c])
    rec, lev, ns, dist = recon_luma(depth, cur, [p[0] for p in lists[0]], [p[0] for p in lists[1]], stride, org, w64, h64, level, mv0, mv1, i0, i1, dirs, qp,
                                    tu_flags, cells(0), cores)
    out.update({"levels": lev, "num_sig": ns, "dist": dist})
    bv, bh = O.deblock_bs_b(depth, w64, h64, level, mv0, mv1, e["ref0"], e["ref1"], ns, slice_b=True)
    sc, oc = SC.chroma_geometry(w64)
    qpc = S.chroma_quant_qp(qp, depth)
    crec = [recon_chroma(depth, cur_planes[c], [p[c] for p in lists[0]], [p[c] for p in lists[1]], sc, oc, w64, h64, level, mv0, mv1, i0, i1, dirs, qpc,
                         tu_flags, cells(c), cores) for c in (1, 2)]
    for i in range(2):
        out["levels_c%d" % i], out["num_sig_c%d" % i] = crec[i][1], crec[i][2]
    return SC.filter_tail(out, depth, cur_planes, rec, [crec[0][0], crec[1][0]], bv, bh, qp, w64, h64, cu_qp=cu_qp, sao=sao, sao_rdo=sao_rdo, cores=cores)


def device_outputs(pipe, dt, ndistinct):
    """The same names from a stages.MultiRefBFramePipeline after run() (chroma, deblocking, want_cost; the SAO names where it has SAO)."""
    g = lambda t: t.cpu().numpy()
    out, bd = SC.step_outputs(pipe, dt), pipe.bd
    out.update({"subpel_mv%d" % s: g(pipe.spl[s].out).reshape(-1, 2) for s in range(ndistinct)})
    out.update({"ref_idx0": g(pipe.rs[0].ref_idx), "ref_idx1": g(pipe.rs[1].ref_idx), "sel_mv0": g(pipe.rs[0].mv_out).reshape(-1, 2),
                "sel_mv1": g(pipe.rs[1].mv_out).reshape(-1, 2), "dir": g(bd.dir), "ref0": g(bd.ref0), "ref1": g(bd.ref1),
                "mv0_out": g(bd.mv0_out).reshape(-1, 2), "mv1_out": g(bd.mv1_out).reshape(-1, 2), "cost_out": g(bd.cost_out).reshape(-1, 4)})
    return out
