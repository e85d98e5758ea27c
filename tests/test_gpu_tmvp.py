"""GPU parity of the temporal merge candidate: x265hip_col_field_build against the restatement of tests/tmvp_expect.py, both _col entries
without a field against the entries without the candidate (word for word: the guard of the shared kernel bodies), both _col entries on
the cases of tests/tmvp_cases.py against the restated walks, stages.MergePFramePipeline / MergeBFramePipeline with temporal_mvp stage by
stage against the oracle chains run with the handed field, and MiniGop with temporal_mvp.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import bmerge_cases as BC
import bmerge_expect as BM
import intra_expect as IE
import merge_cases as MC
import merge_expect as ME
import tmvp_cases as C
import tmvp_expect as TX
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
GARBAGE = -9
P_TENSORS = ("merge", "merge_idx", "mv_out", "mv_pred", "cost", "best")
B_TENSORS = ("merge", "merge_idx", "dir", "ref0", "ref1", "mv0_out", "mv1_out", "mv0_pred", "mv1_pred", "cost", "best")
B_RECORDS = ("mv0_out", "mv1_out", "mv0_pred", "mv1_pred")


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
    """A stages.ColField holding the unit field of a ColSource: the field handed to the stage directly."""
    col = S.ColField((src.w64 // 64) * (src.h64 // 64), src.w64, src.h64, depth, _dev())
    mv, dl = src.unit_field()
    col.col_mv.copy_(_up(mv))
    col.col_delta.copy_(_up(dl))
    return col


def _fill(md, names, value=None):
    for i, k in enumerate(names):
        getattr(md, k).fill_(value if value is not None else (GARBAGE if "mv" in k else 0x55 + i))


@pytest.mark.parametrize("w,h,depth,level", [(192, 128, 8, 0), (192, 128, 8, 1), (192, 128, 8, 2), (192, 128, 10, 1), (64, 64, 8, 0), (64, 192, 8, 2)])
def test_col_field_build_equals_the_restatement(w, h, depth, level):
    """Outputs pre-filled with garbage; without and with intra / ref_idx; the records' other levels and cost words are not read."""
    import torch
    nctu, nblk = (w // 64) * (h // 64), 64 >> (2 * level)
    rng = np.random.default_rng([31, w, h, level])
    mv = rng.integers(-2 ** 31, 2 ** 31, (nctu * 85, 2), dtype=np.int64).astype(np.int32)
    intra = (rng.integers(0, 4, nctu * nblk) == 0).astype(np.uint8) * rng.integers(1, 256, nctu * nblk).astype(np.uint8)
    ref = rng.integers(-1, 8, nctu * nblk).astype(np.int8)
    deltas = [4, -2, 9, 1, -32768, 32767, 7, -1]
    col = S.ColField(nctu, w, h, depth, _dev())
    for kw, host in ((dict(), dict()), (dict(intra=_up(intra)), dict(intra=intra)), (dict(ref_idx=_up(ref)), dict(ref_idx=ref)),
                     (dict(intra=_up(intra), ref_idx=_up(ref)), dict(intra=intra, ref_idx=ref))):
        for poc in (3, deltas):
            col.col_mv.fill_(GARBAGE)
            col.col_delta.fill_(GARBAGE)
            col.build(_up(mv), level, poc, **kw)
            torch.cuda.synchronize()
            want_mv, want_delta = TX.compress(level, w, h, mv, poc, **host)
            assert np.array_equal(_g(col.col_mv), want_mv) and np.array_equal(_g(col.col_delta), want_delta), (sorted(kw), poc)
    assert set(col.checksum()) == {"col_mv", "col_delta"}
    col.clear()
    assert not _g(col.col_delta).any() and not _g(col.col_mv).any()


def _p_stage(c, x):
    dev = _dev()
    ref_y, cur_y = MC.luma_pair(c.field, c.level, c.depth, c.w, c.h)
    cur, ref = P.DevicePicture(cur_y, dev), P.DevicePicture(ref_y, dev)
    nctu = (c.w // 64) * (c.h // 64)
    md = S.MergeDecide(nctu, c.w, c.h, c.depth, c.level, dev, max_merge=c.max_merge, lambda8=c.lambda8, qp=x["qp"])
    md.qp_map = None if x["tu_qp"] is None else _up(x["tu_qp"][0])
    md.lambda8_by_qp = None if x["lambda8_by_qp"] is None else _up(x["lambda8_by_qp"])
    return cur, ref, nctu, md


def _b_stage(c, x):
    dev = _dev()
    r0_y, cur_y, r1_y = BC.luma_triple(c.kind, c.level, c.depth, c.w, c.h)
    cur, r0, r1 = (P.DevicePicture(y, dev) for y in (cur_y, r0_y, r1_y))
    md = S.BMergeDecide(x["nctu"], c.w, c.h, c.depth, c.level, dev, max_merge=c.max_merge, lambda8=c.lambda8, qp=x["qp"], ref_ids=x["ref_ids"])
    md.qp_map = None if x["tu_qp"] is None else _up(x["tu_qp"][0])
    md.lambda8_by_qp = None if x["lambda8_by_qp"] is None else _up(x["lambda8_by_qp"])
    return cur, r0, r1, md


OLD_P = [MC.COVER_CASES[i] for i in (0, 1, 8, 12 + 5, 12 + 10, 24 + 3, 24 + 7)] + MC.DEEP_CASES[:1] + MC.DEEP_CASES[3:4] + MC.SIZE_CASES[:1] + MC.SIZE_CASES[2:3]
OLD_B = [BC.COVER_CASES[i] for i in (0, 1, 11, 17 + 7, 17 + 12, 34 + 5, 34 + 15)] + BC.DEEP_CASES[:1] + BC.DEEP_CASES[3:4] + BC.SIZE_CASES[:1] + BC.SIZE_CASES[2:3]


@pytest.mark.parametrize("c", **_ids(OLD_P))
def test_merge_decide_col_without_a_field_writes_what_merge_decide_writes(c):
    """The same inputs through x265hip_merge_decide, through x265hip_merge_decide_col with NULL col_mv / col_delta, and with the `none`
    field (the instance with the candidate, which then never has one): every output word for word, the other levels' slots included."""
    import torch
    x = MC.expectation(c)
    cur, ref, nctu, md = _p_stage(c, x)
    mv, cost_in = _up(x["mv"]), _up(x["e"]["inter_cost"].astype(np.int32))
    _fill(md, P_TENSORS)
    md.run(cur, ref, mv, cost_in, inter_cost_stride=1, inter_cost_offset=0)
    torch.cuda.synchronize()
    old = {k: _g(getattr(md, k)).copy() for k in P_TENSORS}
    none = _col_field(TX.ColSource(c.w, c.h), c.depth)
    for col_mv, col_delta in ((None, None), (none.col_mv, none.col_delta)):
        _fill(md, P_TENSORS)
        A.merge_decide_col(md.depth, md.w64, md.h64, md.level, cur.t, cur.stride, cur.org, ref.t, ref.stride, ref.org, mv, cost_in, md.lambda8, md.max_merge,
                           md.merge, md.merge_idx, md.mv_out, md.mv_pred, md.cost, col_mv, col_delta, 3, best=md.best, inter_cost_stride=1,
                           inter_cost_offset=0, qp=md.qp, qp_map=md.qp_map, lambda8_by_qp=md.lambda8_by_qp)
        torch.cuda.synchronize()
        for k in P_TENSORS:
            assert np.array_equal(_g(getattr(md, k)), old[k]), (k, col_mv is None)


@pytest.mark.parametrize("c", **_ids(OLD_B))
def test_b_merge_decide_col_without_a_field_writes_what_b_merge_decide_writes(c):
    import torch
    x = BC.expectation(c)
    cur, r0, r1, md = _b_stage(c, x)
    dir_in, mv0, mv1, cost_in = _up(x["dir_in"]), _up(x["mv0"]), _up(x["mv1"]), _up(x["e"]["inter_cost"].astype(np.int32))
    _fill(md, B_TENSORS)
    md.run(cur, r0, r1, dir_in, mv0, mv1, cost_in, inter_cost_stride=1)
    torch.cuda.synchronize()
    old = {k: _g(getattr(md, k)).copy() for k in B_TENSORS}
    none = _col_field(TX.ColSource(c.w, c.h), c.depth)
    for col_mv, col_delta in ((None, None), (none.col_mv, none.col_delta)):
        _fill(md, B_TENSORS)
        A.b_merge_decide_col(md.depth, md.w64, md.h64, md.level, cur.t, cur.stride, r0.t, r1.t, r0.stride, dir_in, mv0, mv1, cost_in, md.lambda8, md.max_merge,
                             md.merge, md.merge_idx, md.dir, md.mv0_out, md.mv1_out, md.mv0_pred, md.mv1_pred, md.cost, col_mv, col_delta, (2, -2),
                             best=md.best, ref0=md.ref0, ref1=md.ref1, ref_ids=md.ref_ids, fenc_off=cur.org, fref_off=r0.org, inter_cost_stride=1, qp=md.qp,
                             qp_map=md.qp_map, lambda8_by_qp=md.lambda8_by_qp)
        torch.cuda.synchronize()
        for k in B_TENSORS:
            assert np.array_equal(_g(getattr(md, k)), old[k]), (k, col_mv is None)


@pytest.mark.parametrize("tc", **_ids(C.P_COVER + C.P_OTHER))
def test_merge_decide_col_equals_the_walk(tc):
    """192x128 at 8 bits, levels 0 - 2, every field and distance pair; level 1 at 10 bits, 64x64 and 64x192.  Outputs pre-filled with
    garbage, the other levels' slots keep it; a second run over the same inputs."""
    import torch
    c, x = tc.base, C.expectation(tc)
    e = x["e"]
    cur, ref, nctu, md = _p_stage(c, x)
    sl = ME.level_slots(c.level, nctu)
    other = np.setdiff1d(np.arange(nctu * 85), sl)
    mv, cost_in = _up(x["mv"]), _up(e["inter_cost"].astype(np.int32))
    col = _col_field(x["col"], c.depth)
    _fill(md, P_TENSORS)
    for run in range(2):
        md.run(cur, ref, mv, cost_in, inter_cost_stride=1, inter_cost_offset=0, col=col, cur_delta=tc.cur_delta)
        torch.cuda.synchronize()
        out, pred = _g(md.mv_out).reshape(-1, 2), _g(md.mv_pred).reshape(-1, 2)
        got = {"merge": _g(md.merge), "merge_idx": _g(md.merge_idx), "mv_out": out[sl], "mv_pred": pred[sl], "cost": _g(md.cost).reshape(-1, 2),
               "best": _g(md.best).reshape(-1, 2)}
        bad = BE.compare(got, {k: e[k] for k in got})
        assert not bad, (run, bad)
        assert (out[other] == GARBAGE).all() and (pred[other] == GARBAGE).all(), "slots of other levels were written"
    assert np.array_equal(_g(mv).reshape(-1, 2), x["mv"]) and np.array_equal(_g(col.col_mv), x["col"].unit_field()[0])
    if tc.field != "none":
        assert e["masks"]["temporal_present"].any()


@pytest.mark.parametrize("tc", **_ids(C.B_COVER + C.B_OTHER))
def test_b_merge_decide_col_equals_the_walk(tc):
    import torch
    c, x = tc.base, C.expectation(tc)
    e = x["e"]
    cur, r0, r1, md = _b_stage(c, x)
    sl = BM.level_slots(c.level, x["nctu"])
    other = np.setdiff1d(np.arange(x["nctu"] * 85), sl)
    dir_in, mv0, mv1, cost_in = _up(x["dir_in"]), _up(x["mv0"]), _up(x["mv1"]), _up(e["inter_cost"].astype(np.int32))
    col = _col_field(x["col"], c.depth)
    _fill(md, B_TENSORS)
    for run in range(2):
        md.run(cur, r0, r1, dir_in, mv0, mv1, cost_in, inter_cost_stride=1, col=col, cur_deltas=tc.cur_deltas)
        torch.cuda.synchronize()
        recs = {k: _g(getattr(md, k)).reshape(-1, 2) for k in B_RECORDS}
        got = {"merge": _g(md.merge), "merge_idx": _g(md.merge_idx), "dir": _g(md.dir), "ref0": _g(md.ref0), "ref1": _g(md.ref1),
               "cost": _g(md.cost).reshape(-1, 2), "best": _g(md.best).reshape(-1, 2)}
        got.update({k: v[sl] for k, v in recs.items()})
        bad = BE.compare(got, {k: e[k] for k in BM.OUTPUTS})
        assert not bad, (run, bad)
        assert all((v[other] == GARBAGE).all() for v in recs.values()), "slots of other levels were written"


def _step_kw(depth, qp, slice_type):
    return dict(rng=12, subme=2, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, slice_type),
                temporal_mvp=True)


def _handed_source(level, w, h, vector_of, cur_delta, col_delta):
    """The field handed to a step: checker units with the quads vectors divided out by the scale - candidates that win and units without
    motion, bottom-right tries and centres."""
    return C.col_source("checker", level, w, h, vector_of, TX.scale_factor(cur_delta, col_delta), col_delta)


@pytest.mark.parametrize("depth,level", [(8, 1), (10, 0)])
def test_p_step_with_temporal_mvp_every_stage_equals_the_oracle_chain(depth, level):
    """MergePFramePipeline(temporal_mvp=True).run with a handed field: every stage against merge_expect.p_chain with that field;
    afterwards the step's own field is the compression of its mv_out."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    w, h, qp, cur_delta, col_delta = 192, 128, 30 + 6 * (depth - 8), 2, 4
    n = 8 << level
    ry, cy = MC.luma_pair("quads", level, depth, w, h)
    rc, cc = MC.chroma_pair("quads", level, depth, w, h)
    cur, ref = P.DevicePicture(cy, dev, cc[0], cc[1]), P.DevicePicture(ry, dev, rc[0], rc[1])
    pipe = S.MergePFramePipeline(w, h, depth, dev, level=level, **_step_kw(depth, qp, HT.SLICE_P))
    src = _handed_source(level, w, h, lambda gbx, gby: MC.field_vector("quads", gbx, gby, w // n, h // n), cur_delta, col_delta)
    marks = []
    pipe.run(cur, ref, mark=marks.append, col=_col_field(src, depth), cur_delta=cur_delta)
    torch.cuda.synchronize()
    assert marks[:4] == ["me", "subpel", "inter_cost", "merge"]
    pad = lambda yuv: IE.padded_planes(yuv)[0]
    cpu_out = ME.p_chain(depth, pad((cy,) + cc), pad((ry,) + rc), w, h, 12, 2, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(), col=src,
                         cur_delta=cur_delta)
    bad = BE.compare(ME.p_device_outputs(pipe, cur.host.dtype), cpu_out)
    assert not bad, bad
    nctu = (w // 64) * (h // 64)
    want_mv, want_delta = TX.compress(level, w, h, ME.records(cpu_out["mv_out"][:, 1], cpu_out["mv_out"][:, 0], level, nctu), cur_delta)
    assert np.array_equal(_g(pipe.col.col_mv), want_mv) and np.array_equal(_g(pipe.col.col_delta), want_delta)
    with pytest.raises(ValueError):
        pipe.run(cur, ref, col=pipe.col, cur_delta=cur_delta)                     # the step's own field is overwritten by the run
    with pytest.raises(ValueError):
        pipe.run(cur, ref)                                                        # temporal_mvp needs cur_delta
    with pytest.raises(ValueError):
        S.MergePFramePipeline(w, h, depth, dev, level=level).run(cur, ref, cur_delta=2)


@pytest.mark.parametrize("depth,level", [(8, 1), (10, 0)])
def test_b_step_with_temporal_mvp_every_stage_equals_the_oracle_chain(depth, level):
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    w, h, qp, cur_deltas, col_delta = 192, 128, 30 + 6 * (depth - 8), (1, -1), 2
    n = 8 << level
    ys, cs = BC.luma_triple("quads", level, depth, w, h), BC.chroma_triple("quads", level, depth, w, h)
    yuv = [(ys[i],) + cs[i] for i in range(3)]
    r0, cur, r1 = (P.DevicePicture(y, dev, u, v) for (y, u, v) in yuv)
    pipe = S.MergeBFramePipeline(w, h, depth, dev, level=level, **_step_kw(depth, qp, HT.SLICE_B))
    src = _handed_source(level, w, h, lambda gbx, gby: BC.kind_motion("quads", gbx, gby, w // n, h // n)[1], cur_deltas[0], col_delta)
    pipe.run(cur, r0, r1, col=_col_field(src, depth), cur_deltas=cur_deltas)
    torch.cuda.synchronize()
    hp = [IE.padded_planes(p)[0] for p in yuv]
    cpu_out = BM.merge_b_chain(depth, hp[1], hp[0], hp[2], w, h, 12, 2, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(), col=src,
                               cur_deltas=cur_deltas)
    bad = BE.compare(BM.device_outputs(pipe, cur.host.dtype), cpu_out)
    assert not bad, bad
    with pytest.raises(ValueError):
        pipe.run(cur, r0, r1)                                                     # temporal_mvp needs cur_deltas
    with pytest.raises(ValueError):
        S.MergeBFramePipeline(w, h, depth, dev, level=level).run(cur, r0, r1, cur_deltas=(1, -1))


def _gop_steps(w64, h64, depth, dev, level, qp, temporal):
    common = dict(rng=12, subme=2, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True)
    kw = dict(temporal_mvp=True) if temporal else {}
    i_step = S.IFramePipeline(w64, h64, depth, dev, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                              sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_I))
    p_step = S.MergePFramePipeline(w64, h64, depth, dev, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P), **common, **kw)
    b_step = S.MergeBFramePipeline(w64, h64, depth, dev, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B), **common, **kw)
    return i_step, p_step, b_step


def test_mini_gop_with_temporal_mvp():
    """MiniGop(temporal_mvp=True), gop 2 over three anchors (5 pictures of 192x128).  Every picture is what its step alone produces from
    the coded anchors and the field MiniGop has to hand it: the first P anchor a field without motion (the I anchor's), the second the
    first's own field with cur_delta = gop, the B pictures their later anchor's field with cur_deltas = (1, -1) - scaled vectors.  The
    steps alone are compared with the oracle chains above.  With temporal_mvp=False MiniGop is what it was."""
    import torch
    dev = _dev()
    depth, level, qp, gop = 8, 2, 30, 2
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in BE.occluded_clip(192, 128, 5, depth, 71)]
    w64, h64 = pics[0].w64, pics[0].h64
    i_step, p_step, b_step = _gop_steps(w64, h64, depth, dev, level, qp, True)
    order, out = S.MiniGop(p_step, b_step, gop, i_step=i_step, temporal_mvp=True).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3] and sorted(out) == list(range(5))
    same = lambda a, b: all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, b))
    coded = lambda k: pics[k].like([p.clone() for p in out[k]])
    _, p_alone, b_alone = _gop_steps(w64, h64, depth, dev, level, qp, True)
    nctu = p_alone.nctu
    fields = {}
    for a, col in ((2, None), (4, "of 2")):
        p_alone.run(pics[a], coded(a - gop), col=None if col is None else fields[a - gop], cur_delta=gop)
        torch.cuda.synchronize()
        assert same(p_alone.final_planes(), out[a]), f"anchor {a}"
        f = S.ColField(nctu, w64, h64, depth, dev)
        f.col_mv.copy_(p_alone.col.col_mv)
        f.col_delta.copy_(p_alone.col.col_delta)
        fields[a] = f
        assert (_g(f.col_delta) == gop).all()                                # every block of a P anchor is inter: the whole field has motion
        assert np.array_equal(_g(f.col_mv), TX.compress(level, w64, h64, _g(p_alone.md.mv_out).reshape(-1, 2), gop)[0])
        b_alone.run(pics[a - 1], coded(a - gop), coded(a), col=f, cur_deltas=(1, -1))
        torch.cuda.synchronize()
        assert same(b_alone.final_planes(), out[a - 1]), f"picture {a - 1}"
    # the first P anchor saw no candidate: its walk is the walk without temporal MVP; the field the second one saw changes its list
    _, p_old, b_old = _gop_steps(w64, h64, depth, dev, level, qp, False)
    p_old.run(pics[2], coded(0))
    torch.cuda.synchronize()
    assert same(p_old.final_planes(), out[2])
    # temporal_mvp=False is today's MiniGop, and the refusals
    i2, p2, b2 = _gop_steps(w64, h64, depth, dev, level, qp, False)
    _, plain = S.MiniGop(p2, b2, gop, i_step=i2).run(pics)
    i3, p3, b3 = _gop_steps(w64, h64, depth, dev, level, qp, False)
    _, off = S.MiniGop(p3, b3, gop, i_step=i3, temporal_mvp=False).run(pics)
    torch.cuda.synchronize()
    assert all(same(plain[k], off[k]) for k in range(5)) and same(plain[2], out[2])
    with pytest.raises(ValueError, match="temporal_mvp"):
        S.MiniGop(p3, b_step, gop, i_step=i3, temporal_mvp=True)              # a p_step built without it
    with pytest.raises(ValueError, match="temporal_mvp"):
        S.MiniGop(p_step, b3, gop, i_step=i3, temporal_mvp=True)
    with pytest.raises(ValueError, match="several references"):
        S.MiniGop(p_step, b_step, gop, i_step=i3, p_refs=2, temporal_mvp=True)
    with pytest.raises(ValueError, match="several references"):
        S.MiniGop(p_step, b_step, gop, i_step=i3, b_refs=(2, 1), temporal_mvp=True)
