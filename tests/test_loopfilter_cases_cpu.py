"""The inputs of the loop-filter limit tests (tests/loopfilter_cases.py) checked with the oracle alone: every case the GPU module runs must
really reach the paths it is listed for - packed statistics accumulators filled to their last bit, the largest offsets and the last band
positions, every branch and clip of the luma and chroma edge filters at both ends of the QP range - and the oracle must equal the real
SAO and Deblock classes (oracle/_ref) on these same inputs.  The censuses are plain numpy restatements; they count as evidence because
their pictures and totals equal the oracle's.  These are conditions on the inputs: a case that misses one gets another seed or other
parameters, never a looser condition."""
import ctypes
import os

import numpy as np
import pytest

import loopfilter_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ref(depth, symbol):
    path = os.path.join(ROOT, "oracle", "_ref", f"libx265ref{depth}.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    lib = ctypes.CDLL(path)
    if not hasattr(lib, symbol):
        pytest.skip(f"oracle/_ref predates {symbol}")
    return lib


def _grid(case):
    return -(-case.width // case.ctu[0]), -(-case.height // case.ctu[1])


# ---- SAO statistics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_pictures_fill_the_statistics_accumulators(depth):
    """The census's per-CTU totals equal the oracle's count / offsetOrg on every picture (which is what makes its other figures
    trustworthy), and over the case set: an aligned run of 8 (4 on the 32 x 32 footprint) samples of one row wholly in one of the classes
    1 .. 4 with every difference +mx (at 8 bits the 4 + 12-bit field holds count 8, sum 8 * 511); a run wholly in class 0 (totals minus
    classes, nothing to subtract); a wavefront's 16 x 64 samples in one class (1024 * 511 = 523264 in the 20-bit sum at 8 bits); a lane's
    16 samples in one class (16 * 8191 = 131056 at 12 bits)."""
    O = LC.oracle()
    mx = (1 << depth) - 1
    tot = {}
    for c in LC.SAO_STAT_CASES:
        if c.depth != depth:
            continue
        p = LC.sao_plane(c)
        cnt, off = O.sao_stats(depth, p.src_plane, p.rec_plane, p.stride, p.org, c.width, c.height, ctu=c.ctu, plane_offset=c.plane_offset)
        ccnt, coff, m = LC.sao_census(depth, p.src, p.rec, c.ctu, c.plane_offset)
        assert np.array_equal(ccnt, cnt) and np.array_equal(coff, off), c.id
        for k in ("full_run_class14", "full_run_class0", "full_wave", "full_lane"):
            tot[(c.ctu[0], k)] = tot.get((c.ctu[0], k), 0) + getattr(m, k)
        if (c.width, c.height) == (128, 128):
            if c.family == "flat":                    # the bottom-right CTU counts all its 64 x 64 samples in one band
                assert cnt.max() == 4096 and off.max() == 4096 * mx and cnt[3, 4].max() == 4096 and off[3, 4].max() == 4096 * mx
            if c.family == "rowsneg":
                assert off.min() == -(2048 * mx + 2048 * (mx - 1))
            if c.family == "checker":
                assert off.max() == 2048 * mx and off.min() == -2048 * mx
    print(depth, tot)
    for fp in (64, 32):
        assert tot[(fp, "full_run_class14")] > 0 and tot[(fp, "full_run_class0")] > 0 and tot[(fp, "full_lane")] > 0, tot
    assert tot[(64, "full_wave")] > 0, tot


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_statistics_and_application_equal_the_real_class(depth):
    """x265ref_sao (the real SAO class: calcSaoStatsCTU, saoStatsInitialOffset, generateLumaOffsets) on every luma picture: statistics and
    initial offsets, and the offset picture for every parameter set of the application cases."""
    O = LC.oracle()
    lib = _ref(depth, "x265ref_sao")
    lib.x265ref_sao.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for c in LC.SAO_STAT_CASES:
        if c.depth != depth or c.ctu[0] != 64:
            continue
        p = LC.sao_plane(c)
        cws, chs = _grid(c)
        nctu = cws * chs
        cnt, off = O.sao_stats(depth, p.src_plane, p.rec_plane, p.stride, p.org, c.width, c.height)
        sets = LC.apply_param_sets(depth, cws, chs)
        for ps in (sets if c.family in LC.APPLY_FAMILIES else sets[:1]):
            rcnt, roff = np.zeros((nctu, 5, 32), np.int32), np.zeros((nctu, 5, 32), np.int32)
            rout = p.rec_plane.copy()
            assert lib.x265ref_sao(p.src_plane.ctypes.data, rout.ctypes.data, c.width, c.height, ps.ctypes.data, rcnt.ctypes.data, roff.ctypes.data) == 0
            assert np.array_equal(cnt, rcnt) and np.array_equal(off, roff), c.id
            out = O.sao_apply(depth, p.rec_plane, p.stride, p.org, c.width, c.height, ps)
            a, b = LC.inner(out, p.stride, p.org, c.width, c.height), LC.inner(rout, p.stride, p.org, c.width, c.height)
            assert np.array_equal(a, b), f"{c.id}: {np.count_nonzero(a != b)} samples differ"
        if hasattr(lib, "x265ref_sao_last_initial_offsets"):
            rinit = np.zeros((nctu, 5, 32), np.int32)
            lib.x265ref_sao_last_initial_offsets.argtypes = [ctypes.c_void_p, ctypes.c_int]
            assert lib.x265ref_sao_last_initial_offsets(rinit.ctypes.data, nctu) == 0
            init = O.sao_decide(depth, cnt, off)[0]
            assert np.array_equal(init[:, :4, 1:5], rinit[:, :4, 1:5]) and np.array_equal(init[:, 4, :], rinit[:, 4, :]), c.id


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_chroma_footprint_equals_the_real_class(depth):
    """x265ref_sao_chroma (calcSaoStatsCTU(addr, 1 / 2), generateChromaOffsets) on the 32 x 32 footprint pictures."""
    O = LC.oracle()
    lib = _ref(depth, "x265ref_sao_chroma")
    lib.x265ref_sao_chroma.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    arr = lambda xs: (ctypes.c_void_p * 2)(*[x.ctypes.data for x in xs])
    for c in LC.SAO_STAT_CASES:
        if c.depth != depth or c.ctu[0] != 32:
            continue
        planes = [LC.sao_plane(c, seed=1), LC.sao_plane(c, seed=4)]
        cws, chs = _grid(c)
        nctu = cws * chs
        sets = LC.apply_param_sets(depth, cws, chs)
        for ps in (sets if c.family in LC.APPLY_FAMILIES else sets[:1]):
            rcnt, roff = [np.zeros((nctu, 5, 32), np.int32) for _ in range(2)], [np.zeros((nctu, 5, 32), np.int32) for _ in range(2)]
            rout = [p.rec.copy() for p in planes]
            assert lib.x265ref_sao_chroma(arr([p.src for p in planes]), arr(rout), 2 * c.width, 2 * c.height, arr([ps, ps]), arr(rcnt), arr(roff)) == 0
            for i, p in enumerate(planes):
                cnt, off = O.sao_stats(depth, p.src_plane, p.rec_plane, p.stride, p.org, c.width, c.height, ctu=(32, 32), plane_offset=2)
                assert np.array_equal(cnt, rcnt[i]) and np.array_equal(off, roff[i]), (c.id, i)
                out = O.sao_apply(depth, p.rec_plane, p.stride, p.org, c.width, c.height, ps, ctu=(32, 32))
                got = LC.inner(out, p.stride, p.org, c.width, c.height)
                assert np.array_equal(got, rout[i]), f"{c.id} plane {i}: {np.count_nonzero(got != rout[i])} samples differ"


# ---- SAO decision ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_decision_cases_reach_their_outcomes(depth):
    """Over the decision cases the oracle chooses offsets of +(thresh - 1) and -(thresh - 1), the band positions 0 and 28, edge types and
    the band type, merge-left and merge-up; a picture without differences gets no SAO anywhere; on the checker picture, whose edge types 0
    and 1 differ by one sample, the 8-bit decision changes between QP 0 and QP 51."""
    lim = LC.sao_lim(depth)
    f = dict.fromkeys(("plus", "minus", "bp28", "bp0", "eo", "bo", "merge_left", "merge_up", "off"), 0)
    by_id = {}
    for c in LC.decision_cases(depth):
        params, nos = LC.decide(c)
        by_id[c.id] = (params, nos)
        for pl in params:
            on = pl[:, 0] >= 0
            f["plus"] += int((pl[on, 2:6] == lim).sum()); f["minus"] += int((pl[on, 2:6] == -lim).sum())
            assert (np.abs(pl[:, 2:6]) <= lim).all()
            f["bp28"] += int(((pl[:, 0] == 4) & (pl[:, 1] == 28)).sum()); f["bp0"] += int(((pl[:, 0] == 4) & (pl[:, 1] == 0)).sum())
            f["eo"] += int((on & (pl[:, 0] < 4)).sum()); f["bo"] += int((pl[:, 0] == 4).sum())
            f["merge_left"] += int((pl[:, 6] == 1).sum()); f["merge_up"] += int((pl[:, 6] == 2).sum()); f["off"] += int((~on).sum())
        if c.family == "rowsneg" and c.planes == 1:
            assert ((params[0][:, 0] == 4) & (params[0][:, 1] == 28)).any(), c.id
        if c.family == "zero":                             # what the oracle gives: every CTU of every plane off
            assert all((pl[:, 0] == -1).all() and not pl[:, 1:6].any() for pl in params), c.id
            assert nos.tolist() == [4, 4 if c.planes == 3 else 0], c.id
    print(depth, f)
    assert all(v > 0 for v in f.values()), f
    if depth == 8:
        a, b = by_id["checker-d8-qp0-p3"][0][0], by_id["checker-d8-qp51-p3"][0][0]
        assert set(a[:, 0].tolist()) == {0, 1} and set(b[:, 0].tolist()) == {1} and not np.array_equal(a, b)


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_decision_equals_the_real_class(depth):
    """x265ref_sao_rdo (the real SAO::rdoSaoUnitCu, statistics included) on the decision pictures at QP 0 and 51 and with CTU QPs that
    alternate between them; the host tables' lambdas and context states at those QPs equal the reference's."""
    O = LC.oracle()
    lib = _ref(depth, "x265ref_sao_rdo")
    P3 = ctypes.c_void_p * 3
    lib.x265ref_sao_rdo.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    pad3 = lambda xs: P3(*([x.ctypes.data for x in xs] + [None] * (3 - len(xs))))
    lam2 = (ctypes.c_double * 70).in_dll(lib, "_ZN4x26516x265_lambda2_tabE")
    cscale = (ctypes.c_uint8 * 70).in_dll(lib, "_ZN4x26513g_chromaScaleE")
    lib.x265ref_entropy_bits_table.restype = ctypes.POINTER(ctypes.c_uint32)
    assert np.array_equal(np.ctypeslib.as_array(lib.x265ref_entropy_bits_table(), shape=(128,)), LC.tables()["entropy_bits"])
    for c in LC.decision_cases(depth):
        if c.kind != "picture":
            continue
        p = LC.decision_picture(c.family, depth)
        nctu = c.ctus_w * c.ctus_h
        ctu_qp = np.array(c.ctu_qp if c.ctu_qp is not None else (c.qp,) * nctu, dtype=np.int32)
        rparams = [np.zeros((nctu, 7), np.int32) for _ in range(3)]
        info = np.zeros(8, np.int64)
        assert lib.x265ref_sao_rdo(pad3(p.src[:c.planes]), pad3(p.rec[:c.planes]), p.width, p.height, int(c.planes == 1), c.slice_type, c.qp, ctu_qp.ctypes.data, 0,
                                   P3(*[r.ctypes.data for r in rparams]), info.ctypes.data) == 0
        counts, orgs, lam, ctx_m, ctx_t, flag = LC.decision_inputs(c)
        assert [ctx_m, ctx_t] == info[2:4].tolist(), c.id
        # the reference's lambda table is one per bit depth (constants.cpp:53-170); the host tables hold the 8-bit one
        rlam = np.array([[int(np.floor(256.0 * lam2[q])), int(np.floor(256.0 * lam2[q if c.planes == 1 else int(cscale[q])]))] for q in ctu_qp.tolist()], dtype=np.int64)
        assert rlam[0].tolist() == info[0:2].tolist(), c.id
        if depth == 8:
            assert np.array_equal(rlam, lam), c.id
        params, nos = O.sao_rdo(depth, counts, orgs, c.ctus_w, c.ctus_h, rlam, ctx_m, ctx_t, LC.tables()["entropy_bits"], sao_flag=flag)
        for pl in range(c.planes):
            bad = np.argwhere((params[pl] != rparams[pl]).any(axis=1))[:5].reshape(-1).tolist()
            assert np.array_equal(params[pl], rparams[pl]), f"{c.id} plane {pl}: CTUs {bad}: oracle {params[pl][bad].tolist()} reference {rparams[pl][bad].tolist()}"
        assert int(nos[0]) == int(info[4]) and (c.planes == 1 or int(nos[1]) == int(info[5])), c.id


def test_raw_statistics_stay_inside_what_pictures_produce():
    for depth in LC.DEPTHS:
        mx = (1 << depth) - 1
        for c in LC.decision_cases(depth):
            if c.kind != "raw":
                continue
            counts, orgs = LC.decision_inputs(c)[:2]
            for n, e in zip(counts, orgs):
                assert n.min() == 0 and n.max() == 4096 and (np.abs(e.astype(np.int64)) <= n.astype(np.int64) * mx).all()
                assert ((e == n * mx) & (n > 0)).any() and ((e == -n * mx) & (n > 0)).any() and (n == 0).mean() > 0.25
                # the decision's int products: (e * 2 + n), (n * o - e * 2) * o with |o| <= 31
                assert (np.abs(n.astype(np.int64) * 31 - 2 * e.astype(np.int64)) * 31 < 2 ** 31).all()


# ---- SAO application ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_apply_cases_clip_at_both_ends_and_change_every_class(depth):
    O = LC.oracle()
    clip0 = clipmx = 0
    changed = np.zeros((4, 5), np.int64)
    pos = set()
    for c in LC.SAO_APPLY_CASES:
        if c.depth != depth:
            continue
        p = LC.sao_plane(c)
        for ps in LC.apply_param_sets(depth, *_grid(c)):
            assert set(np.abs(ps[:, 2:6]).reshape(-1).tolist()) == {LC.sao_lim(depth)}
            pos |= set(ps[ps[:, 0] == 4, 1].tolist())
            out = LC.inner(O.sao_apply(depth, p.rec_plane, p.stride, p.org, c.width, c.height, ps, ctu=c.ctu), p.stride, p.org, c.width, c.height)
            exp, a, b, chg = LC.apply_census(depth, p.rec, out, ps, c.ctu)
            assert np.array_equal(exp, out), c.id
            clip0 += a; clipmx += b; changed += chg
    print(depth, clip0, clipmx, changed.tolist())
    assert clip0 > 0 and clipmx > 0 and (changed[:, 1:] > 0).all() and pos == {0, 28, 31}
    assert any((ps[:, 6] == 1).any() for ps in LC.apply_param_sets(depth, 2, 2))


# ---- deblocking --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_luma_deblocking_cases_reach_every_path(depth):
    """The census picture equals the oracle's deblock_luma on every case, and every counter is non-zero for both directions: units skipped
    by beta, strong and normal units, lines skipped at 10 tc, the +-tc and +-tc / 2 clips, the second sample filtered and not, the range clip
    at 0 and at max, units that pass beta with tc = 0, and strong-filter taps cut at 2 tc.  At QP 0 and 15 (beta 0) and at QP 16 / 17 with
    Bs 1 (tc 0) the picture must not change."""
    O = LC.oracle()
    tot = [dict.fromkeys(LC.LUMA_COUNTERS, 0) for _ in range(2)]
    ramps = [0, 0]
    for c in LC.luma_cases(depth):
        plane, stride, org, bv, bh, qm = LC.luma_inputs(c)
        exp = O.deblock_luma(depth, plane.reshape(-1), stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, qp_map=qm, beta_offset_div2=c.bo, tc_offset_div2=c.to)
        img = LC.deblock_picture(c.kind, depth, c.qp, c.base)
        got, cnts = LC.luma_census(depth, img, bv, bh, c.qp, qm, c.bo, c.to)
        assert np.array_equal(got, LC.inner(exp, stride, org, LC.DB_W, LC.DB_H)), c.id
        for k in range(2):
            for n, v in cnts[k].items():
                tot[k][n] += v
            if c.kind == "ramps":
                ramps[k] += cnts[k]["strong_clip"]
        if not c.qmap and c.bo == 0 and c.qp <= 15:
            assert np.array_equal(got, img) and all(cn["strong"] + cn["normal"] == 0 and cn["beta_skip"] > 0 for cn in cnts), c.id
        if not c.qmap and c.bo == 0 and c.qp in (16, 17) and c.bs == "1":
            assert np.array_equal(got, img) and all(cn["tc0_pass"] > 0 and cn["tc0_pass"] == cn["normal"] for cn in cnts), c.id
        if c.kind == "steps" and c.qp >= 18 and c.bo == 0 and not c.qmap:
            assert all(cn["strong"] > 0 and cn["normal"] > 0 for cn in cnts), c.id
    print(depth, tot, ramps)
    for k in range(2):
        assert all(v > 0 for v in tot[k].values()), (k, tot[k])
        assert ramps[k] > 0


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_chroma_deblocking_cases_reach_every_path(depth):
    O = LC.oracle()
    tot = dict.fromkeys(LC.CHROMA_COUNTERS, 0)
    for c in LC.chroma_cases(depth):
        pb, pr, stride, org, bv, bh, qm = LC.chroma_inputs(c)
        eb, er = O.deblock_chroma(depth, pb, pr, stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, qp_map=qm, cb_qp_offset=c.cb, cr_qp_offset=c.cr)
        cb, cr = LC.chroma_picture(depth, c.base, c.seed)
        gb, gr, cnt = LC.chroma_census(depth, cb, cr, bv, bh, c.qp, qm, c.cb, c.cr)
        assert np.array_equal(gb, LC.inner(eb, stride, org, LC.DB_W // 2, LC.DB_H // 2)), c.id
        assert np.array_equal(gr, LC.inner(er, stride, org, LC.DB_W // 2, LC.DB_H // 2)), c.id
        for n, v in cnt.items():
            tot[n] += v
    print(depth, tot)
    assert all(v > 0 for v in tot.values()), tot


def test_qp_map_means_round_up():
    qm = LC.qp_map_extremes(LC.DB_W, LC.DB_H).astype(np.int64)
    pairs = set(zip(qm[:, :-1].reshape(-1).tolist(), qm[:, 1:].reshape(-1).tolist())) | set(zip(qm[:-1].reshape(-1).tolist(), qm[1:].reshape(-1).tolist()))
    assert {(0, 51), (50, 51)} <= pairs or {(51, 0), (51, 50)} <= pairs
    qv, qh = LC.unit_qps(30, qm, LC.DB_W, LC.DB_H)
    assert 26 in qv and 51 in qv                               # (0 + 51 + 1) >> 1, (50 + 51 + 1) >> 1
    assert ((qm[:-1] + qm[1:]) & 1).any() and ((qm[:, :-1] + qm[:, 1:]) & 1).any()          # means that round, in both passes


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_deblocking_equals_the_real_class(depth):
    """x265ref_deblock420 (the real Deblock::deblockCTU) on the luma cases with uniform QP and Bs 1 (zero vectors, every block coded) or Bs 2
    (every block intra) on the 8 x 8 grid, and on the chroma cases without a QP map."""
    O = LC.oracle()
    lib = _ref(depth, "x265ref_deblock420")
    lib.x265ref_deblock420.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5
    nctu = (LC.DB_W // 64) * (LC.DB_H // 64)
    mv, ns = np.zeros((nctu * 85, 2), np.int32), np.ones((nctu, 64), np.uint32)
    flags = {"1": np.zeros((nctu, 64), np.uint8), "2": np.ones((nctu, 64), np.uint8)}
    cw, ch = LC.DB_W // 2, LC.DB_H // 2
    for c in LC.luma_cases(depth):
        if c.bs == "random" or c.qmap:
            continue
        plane, stride, org, bv, bh, _ = LC.luma_inputs(c)
        exp = O.deblock_luma(depth, plane.reshape(-1), stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, beta_offset_div2=c.bo, tc_offset_div2=c.to)
        got = plane.reshape(-1).copy()
        assert lib.x265ref_deblock420(got.ctypes.data, None, None, LC.DB_W, LC.DB_H, 0, mv.ctypes.data, ns.ctypes.data, flags[c.bs].ctypes.data,
                                      c.qp, c.bo, c.to, 0, 0) == 0
        assert np.array_equal(got, exp), f"{c.id}: {np.count_nonzero(got != exp)} samples differ"
    luma = LC.luma_inputs(LC.luma_cases(depth)[0])[0]
    for c in LC.chroma_cases(depth):
        if c.qmap:
            continue
        pb, pr, stride, org, bv, bh, _ = LC.chroma_inputs(c)
        eb, er = O.deblock_chroma(depth, pb, pr, stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, cb_qp_offset=c.cb, cr_qp_offset=c.cr)
        y = luma.reshape(-1).copy()
        got = [np.ascontiguousarray(x).copy() for x in LC.chroma_picture(depth, c.base, c.seed)]
        assert lib.x265ref_deblock420(y.ctypes.data, got[0].ctypes.data, got[1].ctypes.data, LC.DB_W, LC.DB_H, 0, mv.ctypes.data, ns.ctypes.data,
                                      flags["2"].ctypes.data, c.qp, 0, 0, c.cb, c.cr) == 0
        for g, e in zip(got, (eb, er)):
            assert np.array_equal(g, LC.inner(e, stride, org, cw, ch)), f"{c.id}: {np.count_nonzero(g != LC.inner(e, stride, org, cw, ch))} samples differ"
