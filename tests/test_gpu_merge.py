"""GPU parity of the merge stage of a P picture: x265hip_merge_decide against the walk of tests/merge_expect.py on the cases of
tests/merge_cases.py, x265hip_inter_sa8d_cost (whose body the stage shares) against the oracle's numbers, stages.MergePFramePipeline stage
by stage against the oracle chain, and MiniGop with the step as its p_step.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import intra_expect as IE
import merge_cases as C
import merge_expect as ME
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
GARBAGE = -9


def _ids(cases):
    return dict(argvalues=cases, ids=[c.id for c in cases])


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(_dev())


def _run_case(c):
    """The stage alone: every output pre-filled with garbage, two runs over the same inputs into the same buffers.  With `real` costs the
    inter costs are what x265hip_inter_sa8d_cost leaves on the device (compared with the oracle's first); with `pattern` costs, the numbers
    the walk decided against."""
    import torch
    dev = _dev()
    x = C.expectation(c)
    e = x["e"]
    ref_y, cur_y = C.luma_pair(c.field, c.level, c.depth, c.w, c.h)
    cur, ref = P.DevicePicture(cur_y, dev), P.DevicePicture(ref_y, dev)
    nctu = (c.w // 64) * (c.h // 64)
    sl = ME.level_slots(c.level, nctu)
    mv = _up(x["mv"])
    qp_map = None if x["tu_qp"] is None else _up(x["tu_qp"][0])
    lam_tab = None if x["lambda8_by_qp"] is None else _up(x["lambda8_by_qp"])
    md = S.MergeDecide(nctu, c.w, c.h, c.depth, c.level, dev, max_merge=c.max_merge, lambda8=c.lambda8, qp=x["qp"])
    md.qp_map, md.lambda8_by_qp = qp_map, lam_tab
    assert md.waves == IE.waves(c.w, c.h)
    if c.costs == "real":
        ic = S.InterSa8dCost(nctu, c.w, c.h, c.depth, c.level, dev, rng=80, lambda8=c.lambda8, qp=x["qp"])
        ic.qp_map, ic.lambda8_by_qp = qp_map, lam_tab
        ic.cost.fill_(-7)
        ic.run(cur, ref, mv)
        torch.cuda.synchronize()
        got = ic.cost.cpu().numpy().reshape(-1, 2)
        assert np.array_equal(got, x["real"]), np.flatnonzero((got != x["real"]).any(axis=1))[:8]
        cost_in, stride, offset = ic.cost, 2, 1
    else:
        cost_in, stride, offset = _up(e["inter_cost"].astype(np.int32)), 1, 0
    want = {k: e[k] for k in ("merge", "merge_idx", "mv_out", "mv_pred", "cost", "best")}
    for t, v in ((md.merge, 0xa5), (md.merge_idx, 0x5a), (md.mv_out, GARBAGE), (md.mv_pred, GARBAGE), (md.cost, -3), (md.best, -5)):
        t.fill_(v)
    other = np.setdiff1d(np.arange(nctu * 85), sl)
    for run in range(2):
        md.run(cur, ref, mv, cost_in, inter_cost_stride=stride, inter_cost_offset=offset)
        torch.cuda.synchronize()
        out, pred = md.mv_out.cpu().numpy().reshape(-1, 2), md.mv_pred.cpu().numpy().reshape(-1, 2)
        got = {"merge": md.merge.cpu().numpy(), "merge_idx": md.merge_idx.cpu().numpy(), "mv_out": out[sl], "mv_pred": pred[sl],
               "cost": md.cost.cpu().numpy().reshape(-1, 2), "best": md.best.cpu().numpy().reshape(-1, 2)}
        bad = BE.compare(got, want)
        assert not bad, (run, bad)
        assert (out[other] == GARBAGE).all() and (pred[other] == GARBAGE).all(), "slots of other levels were written"
    assert np.array_equal(mv.cpu().numpy(), x["mv"])
    return e


@pytest.mark.parametrize("c", **_ids(C.COVER_CASES))
def test_merge_decide_equals_the_walk(c):
    """192x128 at 8 bits, levels 0 - 2: every field, real and pattern inter costs, max_merge 1 / 2 / 3 / 5, lambda8 1024 and 0."""
    e = _run_case(c)
    if c.costs == "pattern":
        b = np.arange(len(e["merge"]))
        assert np.array_equal(e["merge"], (b % 3 != 0).astype(np.uint8)) and e["masks"]["tie_stays_merge"].mean() > 0.3
    if c.lambda8 == 0:                                   # the index is free: cost = sa8d, and equal candidates (the zero fill) tie
        assert np.array_equal(e["cost"][:, 0], e["cost"][:, 1]) and (c.level == 2 or e["masks"]["tie_lowest_index"].any())


@pytest.mark.parametrize("c", **_ids(C.DEEP_CASES + C.SIZE_CASES))
def test_merge_decide_at_ten_bits_under_maps_and_on_other_grids(c):
    """Level 1 at 10 bits, a qp_map with a lambda8_by_qp table, and 64x64, 64x192 (empty odd waves) and 256x64."""
    e = _run_case(c)
    assert e["merge"].any()


def _p_step(w64, h64, depth, dev, level, qp, rng, subme, max_merge=3):
    return S.MergePFramePipeline(w64, h64, depth, dev, rng=rng, subme=subme, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                                 sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P), max_merge=max_merge)


def _pair(depth, level, w, h):
    """(reference, current) Y / Cb / Cr: the quads pair of the level - vectors of up to 4 samples, equal in 2x2 groups of blocks."""
    ry, cy = C.luma_pair("quads", level, depth, w, h)
    rc, cc = C.chroma_pair("quads", level, depth, w, h)
    return (ry,) + rc, (cy,) + cc


def _padded(yuv):
    return IE.padded_planes(yuv)[0]


def _step_against_chain(depth, level, w, h, qp, max_merge=3, maps=False):
    """maps: set_qp_maps with a tu_qp / cu_qp map (both range ends, entries outside the range) and a lambda8_by_qp table."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    rng, subme = 12, 2
    ref_yuv, cur_yuv = _pair(depth, level, w, h)
    cur, ref = P.DevicePicture(cur_yuv[0], dev, cur_yuv[1], cur_yuv[2]), P.DevicePicture(ref_yuv[0], dev, ref_yuv[1], ref_yuv[2])
    pipe = _p_step(cur.w64, cur.h64, depth, dev, level, qp, rng, subme, max_merge)
    kw = {}
    if maps:
        tu = C.tu_qp_map(depth, level, w, h)
        kw = dict(tu_qp=tu, cu_qp=np.clip(tu[0].astype(np.int64) - 6 * (depth - 8), 0, 51).astype(np.int8), lambda8_by_qp=C.QE.lambda8_table(depth))
        m = S.CuQpMaps(cur.w64, cur.h64, depth, level, dev).load(kw["cu_qp"], tu)
        pipe.set_qp_maps(m, _up(kw["lambda8_by_qp"]))
        assert pipe.md.qp_map.data_ptr() == pipe.ic.qp_map.data_ptr() == m.tu_qp[0].data_ptr() and pipe.md.lambda8_by_qp is pipe.ic.lambda8_by_qp
        assert pipe.rc.qp_map.data_ptr() == m.tu_qp[0].data_ptr() and pipe.rc_c[1].qp_map.data_ptr() == m.tu_qp[2].data_ptr() and pipe.db.qp_map is m.cu_qp
    marks = []
    pipe.run(cur, ref, mark=marks.append)
    torch.cuda.synchronize()
    assert marks == ["me", "subpel", "inter_cost", "merge", "recon", "recon_chroma", "skip", "deblock", "sao_stats", "sao_rdo", "sao_apply", "border"]
    dev_out = ME.p_device_outputs(pipe, cur.host.dtype)
    cpu_out = ME.p_chain(depth, _padded(cur_yuv), _padded(ref_yuv), cur.w64, cur.h64, rng, subme, level, qp, max_merge=max_merge, sao_rdo=pipe.sao_rdo,
                         cores=B.effective_cpus(), **kw)
    bad = BE.compare(dev_out, cpu_out)
    assert not bad, bad
    assert set(pipe.checksum()) >= {"merge", "merge_idx", "mv_out", "mv_pred", "skip", "inter_cost", "levels", "recon"}
    if maps:                                       # and the picture-wide QP and lambda again
        pipe.set_qp_maps(None)
        assert pipe.md.qp_map is None and pipe.ic.lambda8_by_qp is None and pipe.rc.qp_map is None and pipe.db.qp_map is None
        pipe.run(cur, ref)
        torch.cuda.synchronize()
        plain = ME.p_chain(depth, _padded(cur_yuv), _padded(ref_yuv), cur.w64, cur.h64, rng, subme, level, qp, max_merge=max_merge, sao_rdo=pipe.sao_rdo,
                           cores=B.effective_cpus())
        bad = BE.compare(ME.p_device_outputs(pipe, cur.host.dtype), plain)
        assert not bad, bad
        assert not np.array_equal(plain["merge_cost"], cpu_out["merge_cost"]) and not np.array_equal(plain["levels"], cpu_out["levels"])
    return cpu_out


@pytest.mark.parametrize("depth,level,w,h", [(8, 2, 192, 128), (8, 1, 192, 128), (10, 0, 192, 128), (8, 1, 256, 64)])
def test_p_step_every_stage_equals_the_oracle_chain(depth, level, w, h):
    """MergePFramePipeline.run with chroma, deblocking, SAO applied with the rate-distortion parameters and sign hiding: refined vectors,
    inter costs, merge flags and indices, both vector records, luma + chroma levels, numSig, SSE, skip flags, Bs maps, SAO statistics +
    parameters and the final Y / Cb / Cr planes."""
    out = _step_against_chain(depth, level, w, h, 30 + 6 * (depth - 8))
    share = out["merge"].mean()
    assert 0.2 <= share <= 0.95, share


def test_p_step_at_the_largest_qp_most_merged_blocks_skip():
    out = _step_against_chain(8, 1, 192, 128, 51)
    merged = out["merge"] != 0
    assert merged.mean() >= 0.2 and out["skip"][merged].mean() > 0.5 and not out["skip"][~merged].any()


def test_p_step_at_qp_zero_no_block_skips():
    out = _step_against_chain(8, 1, 192, 128, 0, max_merge=5)
    assert (out["merge"] != 0).mean() >= 0.2 and not out["skip"].any()


def test_p_step_hands_qp_maps_to_every_stage():
    """set_qp_maps on the step: the TU stages quantise with the map's QPs, both candidates are priced with the lambda of the block's luma
    QP, deblocking reads the CU map - every stage against the chain under the same maps - and set_qp_maps(None) restores the plain step."""
    out = _step_against_chain(8, 1, 192, 128, 30, maps=True)
    assert 0.2 <= out["merge"].mean() <= 0.98


def test_mini_gop_with_the_step_as_p_step():
    """MiniGop with an i_step and MergePFramePipeline as p_step, gop 1, three anchors of 192x128 (the quads pair's reference, its current
    picture, the reference again): every anchor is what the step alone produces from the previous coded anchor, and blocks merge in both
    P pictures."""
    import torch
    dev = _dev()
    depth, level, qp, rng, subme = 8, 2, 30, 12, 2
    ref_yuv, cur_a = _pair(depth, level, 192, 128)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in (ref_yuv, cur_a, ref_yuv)]
    w64, h64 = pics[0].w64, pics[0].h64
    i_step = S.IFramePipeline(w64, h64, depth, dev, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                              sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_I))
    order, out = S.MiniGop(_p_step(w64, h64, depth, dev, level, qp, rng, subme), None, 1, i_step=i_step).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 1, 2]
    same = lambda a, b: all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, b))
    alone = _p_step(w64, h64, depth, dev, level, qp, rng, subme)
    prev = pics[0].like([p.clone() for p in out[0]])
    for a in (1, 2):
        alone.run(pics[a], prev)
        torch.cuda.synchronize()
        assert same(alone.final_planes(), out[a]), f"anchor {a}"
        assert float(alone.md.merge.float().mean().item()) > 0.1, a
        prev = pics[a].like([p.clone() for p in out[a]])
