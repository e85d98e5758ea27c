"""GPU parity of the chroma-SATD sub-pel refinement (x265hip_subpel_refine_chroma) against the literal walk of motion.cpp:1456-1561 made
of the oracle's phase-plane samples and the oracle's / the reference's SATD slots (tests/subpel_chroma_expect.py): every one of the
nctu * 85 records, bit for bit, over a sentinel-filled output; and of the bidirectional decision with chroma
(x265hip_bidir_decide_chroma) against its formula on the oracle's captured predictions.  What the inputs reach is asserted, with the
oracle alone, in tests/test_subpel_chroma_cpu.py."""
import importlib

import numpy as np
import pytest

import subpel_cases as SC
import subpel_chroma_cases as CC
import subpel_chroma_expect as CE

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")

SENTINEL = -0x5a5a5a5b


def _refine_on_device(case, planes, chroma_satd=True, null_chroma=False):
    """The stage on a builder case, the records uploaded into a MotionSearch's `best` (no search runs).  null_chroma: the pictures carry
    chroma planes but the call passes c = NULL (hipabi.subpel_refine without `chroma`)."""
    import torch
    dev = torch.device("cuda:0")
    cc = CC.build(*case.build)
    c = cc.luma
    (cur_cb, cur_cr), (ref_cb, ref_cr) = CC.chroma_pictures(cc)
    cur, ref = P.DevicePicture(c.cur_img, dev, cur_cb, cur_cr), P.DevicePicture(c.ref_img, dev, ref_cb, ref_cr)
    assert (cur.stride, cur.org, cur.stride_c, cur.org_c) == (c.stride, c.org, cc.stride_c, cc.org_c)
    assert all(np.array_equal(cur.c_host[k], cc.cur_c[k]) and np.array_equal(ref.c_host[k], cc.ref_c[k]) for k in range(2))
    ms = P.MotionSearch(c.w64, c.h64, c.R, c.depth, dev, want_surf=False)
    ms.best.copy_(torch.from_numpy(c.best.view(np.int64).copy()))
    sp = P.SubpelRefine(ms, case.subme, dev, phase_planes=planes, chroma_satd=chroma_satd and not null_chroma)
    sp.out.fill_(SENTINEL)
    sp.run(cur, ref)
    torch.cuda.synchronize()
    return sp.out.cpu().numpy().reshape(-1, 2)


def _assert_records(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.shape[0]} PUs differ, first {bad[:5]} (ctu {bad[:5] // 85}, record {bad[:5] % 85}): "
                           f"{got[bad[:3]].tolist()} vs {exp[bad[:3]].tolist()}")


@pytest.mark.parametrize("planes", [False, True], ids=["interp", "planes"])
@pytest.mark.parametrize("case", CC.CHROMA_CASES, ids=lambda c: c.id)
def test_subpel_refine_chroma_matches_the_walk(case, planes):
    """8 and 10 bits at subme 3, 4, 5 and 7, 12 bits once, R = 8 and R = 57 once; luma candidates read from phase planes or interpolated -
    chroma is interpolated in the kernel either way."""
    exp = CE.expected(case)["rec"]
    _assert_records(_refine_on_device(case, planes), exp, case.id)
    assert np.count_nonzero(exp[:, 1] != CE.expected(case, False)["rec"][:, 1]) >= exp.shape[0] * 3 // 100          # chroma moves vectors here, not only costs


@pytest.mark.parametrize("planes", [False, True], ids=["interp", "planes"])
@pytest.mark.parametrize("case", CC.LUMA_ONLY_CASES, ids=lambda c: c.id)
def test_subme_2_ignores_the_chroma_operands(case, planes):
    """subme <= 2: bChromaSATD is off (motion.cpp:212) - the entry gives the luma-only records, which are the oracle's."""
    _assert_records(_refine_on_device(case, planes), SC.refined(case), case.id)
    assert np.array_equal(CE.expected(case)["rec"], SC.refined(case))


@pytest.mark.parametrize("planes", [False, True], ids=["interp", "planes"])
def test_null_chroma_record_is_the_luma_only_entry(planes):
    """c = NULL at subme 3 on pictures that do carry chroma: the luma-only records of the oracle's subpel_refine."""
    case = CC.CHROMA_CASES[0]
    _assert_records(_refine_on_device(case, planes, null_chroma=True), SC.refined(case), case.id)


def test_chroma_satd_needs_chroma_planes():
    import torch
    dev = torch.device("cuda:0")
    c = CC.build(*CC.CHROMA_CASES[0].build).luma
    cur, ref = P.DevicePicture(c.cur_img, dev), P.DevicePicture(c.ref_img, dev)
    ms = P.MotionSearch(c.w64, c.h64, c.R, c.depth, dev, want_surf=False)
    ms.best.copy_(torch.from_numpy(c.best.view(np.int64).copy()))
    with pytest.raises(ValueError, match="chroma planes"):
        P.SubpelRefine(ms, 3, dev, chroma_satd=True).run(cur, ref)


def test_chroma_satd_refuses_a_range_past_the_chroma_margin():
    """R = 67 fits the luma margins but its chroma tiles would be read 34 + 6 rows away, past the 40-row chroma margin: refused before
    any launch; R = 66 is the largest that fits."""
    import torch
    dev = torch.device("cuda:0")
    cc = CC.build(*CC.CHROMA_CASES[0].build)
    (cur_cb, cur_cr), (ref_cb, ref_cr) = CC.chroma_pictures(cc)
    cur, ref = P.DevicePicture(cc.luma.cur_img, dev, cur_cb, cur_cr), P.DevicePicture(cc.luma.ref_img, dev, ref_cb, ref_cr)
    ms = P.MotionSearch(cc.w64, cc.h64, 67, cc.depth, dev, want_surf=False)
    with pytest.raises(ValueError, match="chroma margin"):
        P.SubpelRefine(ms, 3, dev, chroma_satd=True).run(cur, ref)
    assert (4 * 66 + 6 + 7) // 8 + 6 <= F.CHROMA_MARGIN_Y < (4 * 67 + 6 + 7) // 8 + 6


# ---------------------------------------------------------------------------------------------------------------------------------
# x265hip_bidir_decide_chroma on the six-stripe B case (all three planes), the records being the walk's
def _b_pictures(depth, dev):
    b = CC.build_b(depth)
    pics = [P.DevicePicture(y, dev, cb, cr) for y, cb, cr in b.pics]
    assert (pics[1].stride, pics[1].org, pics[1].stride_c, pics[1].org_c) == (b.stride, b.org, b.stride_c, b.org_c)
    return b, pics


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 10])
def test_bidir_decide_chroma_matches_the_expectation(depth, level):
    """dir, ref0 / ref1, both output records (sentinel-filled: only the level's entries are written) and cost_out, for every block."""
    import torch
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    dev = torch.device("cuda:0")
    b, (ref0, cur, ref1) = _b_pictures(depth, dev)
    recs = CE.b_records(depth, 3)
    e = CE.bidir_expected(depth, 3, level)
    mv = [torch.from_numpy(r.reshape(-1).copy()).to(dev) for r in recs]
    cq, qoff = F.qpel_cost_table(b.R)
    cq_t = torch.from_numpy(cq.view(np.int16)).to(dev)
    bd = S.BidirDecide(b.nctu, b.w64, b.h64, depth, level, dev, dir_cost=CE.DIR_COST, want_cost=True, chroma_satd=True)
    for t in (bd.mv0_out, bd.mv1_out, bd.cost_out):
        t.fill_(SENTINEL)
    bd.dir.fill_(0x5a)
    bd.run(cur, ref0, ref1, mv[0], mv[1], cq_t, qoff)
    torch.cuda.synchronize()
    import bidir_expect as BE
    assert np.array_equal(bd.dir.cpu().numpy(), e["dir"]), f"dir: {np.count_nonzero(bd.dir.cpu().numpy() != e['dir'])} blocks differ"
    assert np.array_equal(bd.ref0.cpu().numpy(), e["ref0"]) and np.array_equal(bd.ref1.cpu().numpy(), e["ref1"])
    got_cost = bd.cost_out.cpu().numpy().reshape(-1, 4)
    bad = np.nonzero((got_cost != e["cost"]).any(axis=1))[0]
    assert bad.size == 0, f"cost_out: {bad.size} blocks differ, first {bad[:3]}: {got_cost[bad[:3]].tolist()} vs {e['cost'][bad[:3]].tolist()}"
    assert np.array_equal(bd.mv0_out.cpu().numpy().reshape(-1, 2), BE.full_mv_out(level, b.nctu, e["mv0"], SENTINEL))
    assert np.array_equal(bd.mv1_out.cpu().numpy().reshape(-1, 2), BE.full_mv_out(level, b.nctu, e["mv1"], SENTINEL))


def test_bidir_decide_chroma_refuses_phase_planes():
    import torch
    A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
    dev = torch.device("cuda:0")
    b, (ref0, cur, ref1) = _b_pictures(8, dev)
    recs = CE.b_records(8, 3)
    mv = [torch.from_numpy(r.reshape(-1).copy()).to(dev) for r in recs]
    cq, qoff = F.qpel_cost_table(b.R)
    cq_t = torch.from_numpy(cq.view(np.int16)).to(dev)
    out = [torch.zeros(b.nctu * 85 * 2, dtype=torch.int32, device=dev) for _ in range(2)]
    d = torch.zeros(b.nctu * 4, dtype=torch.uint8, device=dev)
    planes = [torch.zeros(15 * ref0.t.numel() * ref0.t.element_size(), dtype=torch.uint8, device=dev) for _ in range(2)]
    chroma = dict(fenc=cur.c, fenc_stride=cur.stride_c, fenc_org=cur.org_c, fref0=ref0.c, fref1=ref1.c, fref_stride=ref0.stride_c, fref_org=ref0.org_c)
    with pytest.raises(A.X265HipError, match="phase planes"):
        A.bidir_decide(8, b.w64, b.h64, 2, cur.t, cur.stride, ref0.t, ref1.t, ref0.stride, mv[0], mv[1], cq_t, qoff, CE.DIR_COST, d, out[0], out[1],
                       fenc_off=cur.org, fref_off=ref0.org, phase_planes=planes, chroma=chroma)
