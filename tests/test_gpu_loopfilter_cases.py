"""GPU parity at the loop filter's arithmetic limits: the cases of tests/loopfilter_cases.py (which tests/test_loopfilter_cases_cpu.py shows
to reach every path, and on which it pins the oracle against the real SAO and Deblock classes) through x265hip_sao_stats / _planes / _rdo /
_apply and x265hip_deblock_luma / _chroma.  The oracle is the only expectation and every comparison is bit for bit."""
import importlib

import numpy as np
import pytest

import loopfilter_cases as LC

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    """A host array as a device byte tensor (the entry points take a tensor's address and an element offset)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(_dev())


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).reshape(-1).copy()).to(_dev())


def _down(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def _sentinel(n, value=-1):
    import torch
    return torch.full((n,), value, dtype=torch.int32, device=_dev())


def _grid(case):
    return -(-case.width // case.ctu[0]), -(-case.height // case.ctu[1])


# ---- SAO statistics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("footprint", [64, 32])
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_stats_at_the_accumulator_limits(depth, footprint):
    """count / offsetOrg of every CTU, type and class into sentinel-filled outputs: runs, lanes, wavefronts and CTUs wholly in one class at
    differences of +-(2^depth - 1), on 2 x 2 CTUs and on a partial picture."""
    O = LC.oracle()
    for c in LC.SAO_STAT_CASES:
        if c.depth != depth or c.ctu[0] != footprint:
            continue
        p = LC.sao_plane(c)
        cws, chs = _grid(c)
        d_cnt, d_off = _sentinel(cws * chs * 160), _sentinel(cws * chs * 160)
        A.sao_stats(depth, _up(p.src_plane), p.stride, p.org, _up(p.rec_plane), p.stride, p.org, c.width, c.height, d_cnt, d_off, ctu=c.ctu,
                    plane_offset=c.plane_offset)
        cnt, off = O.sao_stats(depth, p.src_plane, p.rec_plane, p.stride, p.org, c.width, c.height, ctu=c.ctu, plane_offset=c.plane_offset)
        gc, go = _down(d_cnt, cnt), _down(d_off, off)
        assert np.array_equal(gc, cnt), f"{c.id}: count differs in CTU/type {np.argwhere((gc != cnt).any(axis=2))[:6].tolist()}"
        assert np.array_equal(go, off), f"{c.id}: offsetOrg differs in CTU/type {np.argwhere((go != off).any(axis=2))[:6].tolist()}"


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_three_plane_launch_equals_the_single_plane_entry_and_the_oracle(depth):
    """x265hip_sao_planes with Y 64 x 64 next to two 32 x 32 planes: the statistics-only call, and statistics -> parameters -> application."""
    import torch
    O = LC.oracle()
    geo = [(64, 64, (64, 64), 0), (32, 32, (32, 32), 2), (32, 32, (32, 32), 2)]
    for fam in LC.FAMILIES:
        recs, keep, singles = [], [], []
        fams = (fam, fam, LC.PARTNER[fam])
        for i, (w, h, ctu, po) in enumerate(geo):
            p = LC.sao_plane(LC.SimpleNamespace(family=fams[i], depth=depth, width=w, height=h, ctu=ctu), seed=5 + i)
            d_src, d_rec = _up(p.src_plane), _up(p.rec_plane)
            recs.append(dict(src=d_src, src_stride=p.stride, src_org=p.org, rec=d_rec, rec_stride=p.stride, rec_org=p.org, out=d_rec.clone(), width=w, height=h,
                             count=_sentinel(160), offset_org=_sentinel(160), params=_sentinel(7, 99), ctu=ctu, plane_offset=po))
            keep.append(p)
            s_cnt, s_off = _sentinel(160), _sentinel(160)
            A.sao_stats(depth, d_src, p.stride, p.org, d_rec, p.stride, p.org, w, h, s_cnt, s_off, ctu=ctu, plane_offset=po)
            singles.append((s_cnt, s_off))
        A.sao_planes(depth, [dict(q, out=None) for q in recs])
        torch.cuda.synchronize()
        expect = []
        for i, (q, p) in enumerate(zip(recs, keep)):
            w, h, ctu, po = geo[i]
            cnt, off = O.sao_stats(depth, p.src_plane, p.rec_plane, p.stride, p.org, w, h, ctu=ctu, plane_offset=po)
            assert np.array_equal(_down(q["count"], cnt), cnt) and np.array_equal(_down(q["offset_org"], off), off), f"{fam} plane {i}: statistics-only call"
            assert torch.equal(q["count"], singles[i][0]) and torch.equal(q["offset_org"], singles[i][1]), f"{fam} plane {i}"
            assert (q["params"] == 99).all()
            expect.append((cnt, off))
            q["count"].fill_(-1); q["offset_org"].fill_(-1)
        A.sao_planes(depth, recs)
        torch.cuda.synchronize()
        for i, (q, p) in enumerate(zip(recs, keep)):
            w, h, ctu, po = geo[i]
            cnt, off = expect[i]
            assert np.array_equal(_down(q["count"], cnt), cnt) and np.array_equal(_down(q["offset_org"], off), off), f"{fam} plane {i}"
            params = O.sao_decide(depth, cnt, off)[1]
            assert np.array_equal(_down(q["params"], params), params), f"{fam} plane {i}: parameters"
            out = O.sao_apply(depth, p.rec_plane, p.stride, p.org, w, h, params, ctu=ctu)
            assert np.array_equal(_down(q["out"], out), out), f"{fam} plane {i}: offset plane"


# ---- SAO decision ------------------------------------------------------------------------------------------------------------------------
def _device_rdo(case, counts, orgs, lam):
    """x265hip_sao_rdo on device tensors of statistics; returns (params per plane, numNoSao) as host arrays."""
    import torch
    nctu = case.ctus_w * case.ctus_h
    ctx_m, ctx_t = LC.HT.sao_contexts(case.slice_type, case.qp)
    params = [_sentinel(nctu * 7, 0x5a5a5a5a) for _ in range(case.planes)]
    nos = _sentinel(2)
    scratch = torch.zeros(A.sao_rdo_scratch_bytes(case.ctus_w, case.ctus_h), dtype=torch.uint8, device=_dev())
    per_ctu = case.ctu_qp is not None
    A.sao_rdo(case.depth, counts, orgs, case.ctus_w, case.ctus_h, lam[0], ctx_m, ctx_t, LC.tables()["entropy_bits"], params, scratch,
              lambda_ctu=torch.from_numpy(lam.copy()).to(_dev()) if per_ctu else None, sao_flag=(1, 1 if case.planes == 3 else 0), num_no_sao=nos)
    torch.cuda.synchronize()
    return [p.cpu().numpy().reshape(nctu, 7) for p in params], nos.cpu().numpy()


def _assert_decision(case, got, gn, exp, en):
    for pl in range(case.planes):
        bad = np.argwhere((got[pl] != exp[pl]).any(axis=1))[:5].reshape(-1).tolist()
        assert np.array_equal(got[pl], exp[pl]), f"{case.id} plane {pl}: CTUs {bad}: device {got[pl][bad].tolist()} oracle {exp[pl][bad].tolist()}"
    assert int(gn[0]) == int(en[0]) and (case.planes == 1 or int(gn[1]) == int(en[1])), f"{case.id}: numNoSao {gn.tolist()} / {en.tolist()}"


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_rdo_on_oracle_statistics(depth):
    """The decision walk on the oracle's statistics (so that a statistics bug cannot hide a walk bug) and on raw statistics with
    offsetOrg = +-count * (2^depth - 1): the lambdas of QP 0 and 51 and of CTUs alternating between them, B / P / I contexts, three planes and
    luma only - parameters of all planes and numNoSao."""
    for case in LC.decision_cases(depth):
        counts, orgs, lam, _, _, _ = LC.decision_inputs(case)
        got, gn = _device_rdo(case, [_i32(c) for c in counts], [_i32(o) for o in orgs], lam)
        exp, en = LC.decide(case)
        _assert_decision(case, got, gn, exp, en)


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_rdo_on_the_device_statistics(depth):
    """The same decision pictures with the statistics of all three planes from x265hip_sao_planes."""
    import torch
    for case in LC.decision_cases(depth):
        if case.kind != "picture":
            continue
        p = LC.decision_picture(case.family, depth)
        nctu = case.ctus_w * case.ctus_h
        recs = []
        for c in range(case.planes):
            st, og = (p.stride, p.org) if c == 0 else (p.stride_c, p.org_c)
            recs.append(dict(src=_up(p.src[c]), src_stride=st, src_org=og, rec=_up(p.rec[c]), rec_stride=st, rec_org=og, out=None, width=p.width >> (c > 0),
                             height=p.height >> (c > 0), count=_sentinel(nctu * 160), offset_org=_sentinel(nctu * 160), params=None,
                             ctu=(64, 64) if c == 0 else (32, 32), plane_offset=0 if c == 0 else 2))
        A.sao_planes(depth, recs)
        torch.cuda.synchronize()
        counts, orgs, lam, _, _, _ = LC.decision_inputs(case)
        for c in range(case.planes):
            assert np.array_equal(_down(recs[c]["count"], counts[c]), counts[c]) and np.array_equal(_down(recs[c]["offset_org"], orgs[c]), orgs[c]), f"{case.id} plane {c}"
        got, gn = _device_rdo(case, [q["count"] for q in recs], [q["offset_org"] for q in recs], lam)
        exp, en = LC.decide(case)
        _assert_decision(case, got, gn, exp, en)


# ---- SAO application ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_sao_apply_largest_offsets_last_bands_and_merge_left(depth):
    O = LC.oracle()
    for c in LC.SAO_APPLY_CASES:
        if c.depth != depth:
            continue
        p = LC.sao_plane(c)
        d_rec = _up(p.rec_plane)
        for k, ps in enumerate(LC.apply_param_sets(depth, *_grid(c))):
            d_out = d_rec.clone()
            A.sao_apply(depth, d_rec, p.stride, p.org, d_out, p.stride, p.org, c.width, c.height, _i32(ps), ctu=c.ctu)
            out = O.sao_apply(depth, p.rec_plane, p.stride, p.org, c.width, c.height, ps, ctu=c.ctu)
            got = _down(d_out, out)
            assert np.array_equal(got, out), f"{c.id} set {k}: {np.count_nonzero(got != out)} samples differ"


# ---- deblocking --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_deblock_luma_every_path_and_both_qp_ends(depth):
    """Every picture, Bs map, QP, offset and QP-map combination of the luma cases; at QP 0 / 15 (beta 0) and at QP 16 / 17 with Bs 1 (tc 0
    while beta > 0: the filter is entered) the plane must come back byte for byte, padding included."""
    O = LC.oracle()
    untouched = 0
    for c in LC.luma_cases(depth):
        plane, stride, org, bv, bh, qm = LC.luma_inputs(c)
        d_plane = _up(plane)
        A.deblock_luma(depth, d_plane, stride, org, LC.DB_W, LC.DB_H, _up(bv), _up(bh), c.qp, qp_map=None if qm is None else _up(qm),
                       beta_offset_div2=c.bo, tc_offset_div2=c.to)
        exp = O.deblock_luma(depth, plane.reshape(-1), stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, qp_map=qm, beta_offset_div2=c.bo, tc_offset_div2=c.to)
        got = _down(d_plane, exp)
        assert np.array_equal(got, exp), f"{c.id}: {np.count_nonzero(got != exp)} samples differ"
        if not c.qmap and c.bo == 0 and (c.qp <= 15 or (c.qp in (16, 17) and c.bs == "1")):
            assert np.array_equal(got, plane.reshape(-1)), f"{c.id}: the plane changed"
            untouched += 1
    assert untouched == 2 * 3 * 3 + 2 * 3


@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_deblock_chroma_qp_offsets_table_and_range_clips(depth):
    O = LC.oracle()
    for c in LC.chroma_cases(depth):
        pb, pr, stride, org, bv, bh, qm = LC.chroma_inputs(c)
        d_cb, d_cr = _up(pb), _up(pr)
        A.deblock_chroma(depth, d_cb, d_cr, stride, org, LC.DB_W, LC.DB_H, _up(bv), _up(bh), c.qp, qp_map=None if qm is None else _up(qm),
                         cb_qp_offset=c.cb, cr_qp_offset=c.cr)
        eb, er = O.deblock_chroma(depth, pb, pr, stride, org, LC.DB_W, LC.DB_H, bv, bh, c.qp, qp_map=qm, cb_qp_offset=c.cb, cr_qp_offset=c.cr)
        assert np.array_equal(_down(d_cb, eb), eb) and np.array_equal(_down(d_cr, er), er), c.id


# ---- the loop-filter tail ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qp", [51, 0])
@pytest.mark.parametrize("depth", LC.DEPTHS)
def test_loop_filter_tail_on_a_mixed_picture(depth, qp):
    """Deblock luma + chroma -> SAO statistics of the three planes -> rate-distortion decision -> application, in the order the frame steps run
    them, on a mixed 128 x 128 picture against the same chain of oracle calls."""
    import torch
    O = LC.oracle()
    p = LC.decision_picture("mixed", depth)
    case = LC.SimpleNamespace(id=f"tail-d{depth}-qp{qp}", depth=depth, qp=qp, ctu_qp=None, planes=3, slice_type=1, ctus_w=p.ctus_w, ctus_h=p.ctus_h)
    bv, bh = LC.bs_maps("random", p.w64, p.h64, seed=qp)
    d_bv, d_bh = _up(bv), _up(bh)
    d_rec = [_up(x) for x in p.rec]
    A.deblock_luma(depth, d_rec[0], p.stride, p.org, p.w64, p.h64, d_bv, d_bh, qp)
    A.deblock_chroma(depth, d_rec[1], d_rec[2], p.stride_c, p.org_c, p.w64, p.h64, d_bv, d_bh, qp)
    nctu = p.ctus_w * p.ctus_h
    recs = []
    for c in range(3):
        st, og = (p.stride, p.org) if c == 0 else (p.stride_c, p.org_c)
        recs.append(dict(src=_up(p.src[c]), src_stride=st, src_org=og, rec=d_rec[c], rec_stride=st, rec_org=og, out=d_rec[c].clone(), width=p.width >> (c > 0),
                         height=p.height >> (c > 0), count=_sentinel(nctu * 160), offset_org=_sentinel(nctu * 160), params=_sentinel(nctu * 7, 0x5a5a5a5a),
                         ctu=(64, 64) if c == 0 else (32, 32), plane_offset=0 if c == 0 else 2))
    A.sao_planes(depth, [dict(q, out=None) for q in recs])
    lam = np.array([LC.HT.sao_lambdas(LC.tables(), qp)] * nctu, dtype=np.int64)
    ctx_m, ctx_t = LC.HT.sao_contexts(case.slice_type, qp)
    nos = _sentinel(2)
    scratch = torch.zeros(A.sao_rdo_scratch_bytes(p.ctus_w, p.ctus_h), dtype=torch.uint8, device=_dev())
    A.sao_rdo(depth, [q["count"] for q in recs], [q["offset_org"] for q in recs], p.ctus_w, p.ctus_h, lam[0], ctx_m, ctx_t, LC.tables()["entropy_bits"],
              [q["params"] for q in recs], scratch, sao_flag=(1, 1), num_no_sao=nos)
    A.sao_apply_planes(depth, recs)
    torch.cuda.synchronize()
    # the oracle's chain
    e_rec = [O.deblock_luma(depth, p.rec[0].reshape(-1), p.stride, p.org, p.w64, p.h64, bv, bh, qp)]
    e_rec += list(O.deblock_chroma(depth, p.rec[1].reshape(-1), p.rec[2].reshape(-1), p.stride_c, p.org_c, p.w64, p.h64, bv, bh, qp))
    for c in range(3):
        got = _down(d_rec[c], e_rec[c])
        assert np.array_equal(got, e_rec[c]), f"deblocked plane {c}: {np.count_nonzero(got != e_rec[c])} samples differ"
    if qp == 51:
        assert all((e_rec[c] != p.rec[c].reshape(-1)).any() for c in range(3))
    else:
        assert all(np.array_equal(e_rec[c], p.rec[c].reshape(-1)) for c in range(3))          # beta = tc = 0
    counts, orgs = [], []
    for c in range(3):
        st, og = (p.stride, p.org) if c == 0 else (p.stride_c, p.org_c)
        cnt, off = O.sao_stats(depth, p.src[c].reshape(-1), e_rec[c], st, og, p.width >> (c > 0), p.height >> (c > 0), ctu=recs[c]["ctu"],
                               plane_offset=recs[c]["plane_offset"])
        assert np.array_equal(_down(recs[c]["count"], cnt), cnt) and np.array_equal(_down(recs[c]["offset_org"], off), off), f"statistics of plane {c}"
        counts.append(cnt); orgs.append(off)
    exp, en = O.sao_rdo(depth, counts, orgs, p.ctus_w, p.ctus_h, lam, ctx_m, ctx_t, LC.tables()["entropy_bits"], sao_flag=(1, 1))
    _assert_decision(case, [q["params"].cpu().numpy().reshape(nctu, 7) for q in recs], nos.cpu().numpy(), exp, en)
    assert (exp[0][:, 0] >= 0).any()
    for c in range(3):
        st, og = (p.stride, p.org) if c == 0 else (p.stride_c, p.org_c)
        out = O.sao_apply(depth, e_rec[c], st, og, p.width >> (c > 0), p.height >> (c > 0), exp[c], ctu=recs[c]["ctu"])
        got = _down(recs[c]["out"], out)
        assert np.array_equal(got, out), f"offset plane {c}: {np.count_nonzero(got != out)} samples differ"
