"""GPU parity of AMVP in the merge walk of a P picture: x265hip_merge_decide_amvp on the cases of tests/amvp_cases.py against the restated
walk of tests/amvp_expect.py, x265hip_merge_decide / x265hip_merge_decide_col on their own cases against their unchanged expectations (the
guard of the shared kernel body), stages.MergePFramePipeline(amvp=True) stage by stage against the oracle chain with the AMVP arm, and
MiniGop with amvp.  Equal means equal."""
import importlib

import numpy as np
import pytest

import amvp_cases as C
import amvp_expect as AX
import bidir_expect as BE
import intra_expect as IE
import merge_cases as MC
import merge_expect as ME
import tmvp_cases as TC
import tmvp_expect as TX
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
GARBAGE = -9
OLD_TENSORS = ("merge", "merge_idx", "mv_out", "mv_pred", "cost", "best")
NEW_TENSORS = OLD_TENSORS + ("mvp_idx", "mvd", "amvp", "inter")


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


def _g(t):
    return t.cpu().numpy()


def _col_field(src, depth):
    col = S.ColField((src.w64 // 64) * (src.h64 // 64), src.w64, src.h64, depth, _dev())
    mv, dl = src.unit_field()
    col.col_mv.copy_(_up(mv))
    col.col_delta.copy_(_up(dl))
    return col


def _fill(md, names):
    for i, k in enumerate(names):
        getattr(md, k).fill_(GARBAGE if "mv" in k else 0x55 + i)


def _stage(c, x, **kw):
    dev = _dev()
    ref_y, cur_y = MC.luma_pair(c.field, c.level, c.depth, c.w, c.h)
    cur, ref = P.DevicePicture(cur_y, dev), P.DevicePicture(ref_y, dev)
    nctu = (c.w // 64) * (c.h // 64)
    md = S.MergeDecide(nctu, c.w, c.h, c.depth, c.level, dev, max_merge=c.max_merge, lambda8=c.lambda8, qp=x["qp"], **kw)
    md.qp_map = None if x["tu_qp"] is None else _up(x["tu_qp"][0])
    md.lambda8_by_qp = None if x["lambda8_by_qp"] is None else _up(x["lambda8_by_qp"])
    return cur, ref, nctu, md


def _got(md, sl, names):
    out = {}
    for k in names:
        a = _g(getattr(md, k))
        out[k] = a.reshape(-1, 2)[sl] if k in ("mv_out", "mv_pred") else (a if a.dtype == np.uint8 else a.reshape(-1, 2))
    return out


@pytest.mark.parametrize("ac", **_ids(C.ALL_CASES))
def test_merge_decide_amvp_equals_the_walk(ac):
    """192x128 at 8 bits, levels 0 - 2, every field kind, without temporal MVP and with the `none`, `truth_rb` and `far` fields, one case
    per level with a table of 24 entries; level 1 at 10 bits, 64x64 and 64x192.  Every output word; outputs pre-filled with garbage, the
    other levels' slots keep it; a second run on the same buffers."""
    import torch
    c, x = ac.base, C.expectation(ac)
    e = x["e"]
    cur, ref, nctu, md = _stage(c, x, amvp=True, base_bits=C.BASE_BITS)
    assert md.bit_sizes.numel() == 65537
    md.bit_sizes = _up(C.table(ac.table_len))
    sl = ME.level_slots(c.level, nctu)
    other = np.setdiff1d(np.arange(nctu * 85), sl)
    mv, sa8d = _up(x["mv"]), _up(e["inter_sa8d"].astype(np.int32))
    col = None if x["col"] is None else _col_field(x["col"], c.depth)
    _fill(md, NEW_TENSORS)
    for run in range(2):
        md.run(cur, ref, mv, inter_sa8d=sa8d, inter_sa8d_stride=1, col=col, cur_delta=None if col is None else ac.cur_delta)
        torch.cuda.synchronize()
        got = _got(md, sl, NEW_TENSORS)
        bad = BE.compare(got, {k: e[k] for k in got})
        assert not bad, (run, bad)
        out, pred = _g(md.mv_out).reshape(-1, 2), _g(md.mv_pred).reshape(-1, 2)
        assert (out[other] == GARBAGE).all() and (pred[other] == GARBAGE).all(), "slots of other levels were written"
    assert np.array_equal(_g(mv).reshape(-1, 2), x["mv"]) and np.array_equal(_g(sa8d), e["inter_sa8d"].astype(np.int32))
    with pytest.raises(ValueError):
        md.run(cur, ref, mv, sa8d)                                                # a stage with amvp takes inter_sa8d


OLD_P = [MC.COVER_CASES[i] for i in (0, 1, 8, 12 + 5, 12 + 10, 24 + 3, 24 + 7)] + MC.DEEP_CASES[:1] + MC.DEEP_CASES[3:4] + MC.SIZE_CASES[:1] + MC.SIZE_CASES[2:3]
OLD_COL = [TC.P_COVER[i] for i in (1, 4, 13 + 3, 13 + 7, 26 + 9, 26 + 11)] + TC.P_OTHER


@pytest.mark.parametrize("c", **_ids(OLD_P))
def test_merge_decide_is_what_it_was(c):
    import torch
    x = MC.expectation(c)
    e = x["e"]
    cur, ref, nctu, md = _stage(c, x)
    sl = ME.level_slots(c.level, nctu)
    _fill(md, OLD_TENSORS)
    md.run(cur, ref, _up(x["mv"]), _up(e["inter_cost"].astype(np.int32)), inter_cost_stride=1, inter_cost_offset=0)
    torch.cuda.synchronize()
    got = _got(md, sl, OLD_TENSORS)
    bad = BE.compare(got, {k: e[k] for k in got})
    assert not bad, bad
    assert set(md.checksum()) == {"merge", "merge_idx", "mv_out", "mv_pred", "merge_cost"} and not hasattr(md, "mvd")


@pytest.mark.parametrize("tc", **_ids(OLD_COL))
def test_merge_decide_col_is_what_it_was(tc):
    import torch
    c, x = tc.base, TC.expectation(tc)
    e = x["e"]
    cur, ref, nctu, md = _stage(c, x)
    sl = ME.level_slots(c.level, nctu)
    _fill(md, OLD_TENSORS)
    md.run(cur, ref, _up(x["mv"]), _up(e["inter_cost"].astype(np.int32)), inter_cost_stride=1, inter_cost_offset=0, col=_col_field(x["col"], c.depth),
           cur_delta=tc.cur_delta)
    torch.cuda.synchronize()
    got = _got(md, sl, OLD_TENSORS)
    bad = BE.compare(got, {k: e[k] for k in got})
    assert not bad, bad


def _step_kw(depth, qp, **more):
    return dict(rng=12, subme=2, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P), **more)


@pytest.mark.parametrize("depth,level,temporal", [(8, 1, False), (8, 1, True), (10, 0, False), (10, 0, True)])
def test_p_step_with_amvp_every_stage_equals_the_oracle_chain(depth, level, temporal):
    """MergePFramePipeline(amvp=True).run, without temporal MVP and with a handed field: every stage against amvp_expect.p_chain."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    w, h, qp, cur_delta, col_delta = 192, 128, 30 + 6 * (depth - 8), 2, 4
    n = 8 << level
    ry, cy = MC.luma_pair("quads", level, depth, w, h)
    rc, cc = MC.chroma_pair("quads", level, depth, w, h)
    cur, ref = P.DevicePicture(cy, dev, cc[0], cc[1]), P.DevicePicture(ry, dev, rc[0], rc[1])
    pipe = S.MergePFramePipeline(w, h, depth, dev, level=level, **_step_kw(depth, qp, amvp=True, temporal_mvp=temporal))
    src = None
    marks = []
    if temporal:
        src = TC.col_source("checker", level, w, h, lambda gbx, gby: MC.field_vector("quads", gbx, gby, w // n, h // n), TX.scale_factor(cur_delta, col_delta),
                            col_delta)
        pipe.run(cur, ref, mark=marks.append, col=_col_field(src, depth), cur_delta=cur_delta)
    else:
        pipe.run(cur, ref, mark=marks.append)
    torch.cuda.synchronize()
    assert marks[:4] == ["me", "subpel", "inter_cost", "merge"]
    pad = lambda yuv: IE.padded_planes(yuv)[0]
    cpu_out = AX.p_chain(depth, pad((cy,) + cc), pad((ry,) + rc), w, h, 12, 2, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(), col=src,
                         cur_delta=cur_delta if temporal else None)
    bad = BE.compare(AX.p_device_outputs(pipe, cur.host.dtype), cpu_out)
    assert not bad, bad
    assert {"mvp_idx", "mvd", "amvp", "inter"} <= set(pipe.checksum())


def _gop_steps(w64, h64, depth, dev, level, qp, **kw):
    common = dict(rng=12, subme=2, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True)
    temporal = dict(temporal_mvp=True) if kw.get("temporal_mvp") else {}
    i_step = S.IFramePipeline(w64, h64, depth, dev, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                              sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_I))
    p_step = S.MergePFramePipeline(w64, h64, depth, dev, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P), **common, **kw)
    b_step = S.MergeBFramePipeline(w64, h64, depth, dev, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B), **common, **temporal)
    return i_step, p_step, b_step


def test_mini_gop_with_amvp():
    """MiniGop, gop 2 over three anchors (5 pictures of 192x128), with a p_step built with amvp=True, temporal_mvp=True: MiniGop takes the
    step as it is, and every P anchor is what the step alone produces from the coded anchor and the field MiniGop hands it (the step
    alone is compared with the oracle chain above).  With amvp=False the GOP is what it is without the argument."""
    import torch
    dev = _dev()
    depth, level, qp, gop = 8, 2, 30, 2
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in BE.occluded_clip(192, 128, 5, depth, 71)]
    w64, h64 = pics[0].w64, pics[0].h64
    i_step, p_step, b_step = _gop_steps(w64, h64, depth, dev, level, qp, amvp=True, temporal_mvp=True)
    order, out = S.MiniGop(p_step, b_step, gop, i_step=i_step, temporal_mvp=True).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3] and sorted(out) == list(range(5))
    same = lambda a, b: all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, b))
    coded = lambda k: pics[k].like([p.clone() for p in out[k]])
    _, p_alone, _ = _gop_steps(w64, h64, depth, dev, level, qp, amvp=True, temporal_mvp=True)
    field = None
    for a in (2, 4):
        p_alone.run(pics[a], coded(a - gop), col=field, cur_delta=gop)
        torch.cuda.synchronize()
        assert same(p_alone.final_planes(), out[a]), f"anchor {a}"
        field = S.ColField(p_alone.nctu, w64, h64, depth, dev)
        field.col_mv.copy_(p_alone.col.col_mv)
        field.col_delta.copy_(p_alone.col.col_delta)
    assert _g(p_alone.md.inter).reshape(-1, 2)[:, 0].min() >= 2                   # base_bits are in every block's bits
    # amvp=False is today's step
    i2, p2, b2 = _gop_steps(w64, h64, depth, dev, level, qp)
    _, plain = S.MiniGop(p2, b2, gop, i_step=i2).run(pics)
    i3, p3, b3 = _gop_steps(w64, h64, depth, dev, level, qp, amvp=False)
    _, off = S.MiniGop(p3, b3, gop, i_step=i3).run(pics)
    torch.cuda.synchronize()
    assert all(same(plain[k], off[k]) for k in range(5))
    assert p2.checksum() == p3.checksum() and "mvd" not in p3.checksum()
