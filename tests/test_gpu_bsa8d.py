"""GPU parity of the sa8d choice of a B picture's blocks: x265hip_b_sa8d_decide against tests/bsa8d_expect.py on the cases of
tests/bsa8d_cases.py, stages.Sa8dBFramePipeline stage by stage against the oracle chain with and without b_intra, and MiniGop with the
step as its b_step.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import bsa8d_cases as C
import bsa8d_expect as BX
import intra_inter_cases as PC
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
GARBAGE = -0x5a5a5a5b


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(_dev())


def _run_kernel(c):
    """One launch on a case with every output pre-filled with garbage: dir, ref0 / ref1, the whole mv*_out buffers (only the level's entries
    may change) and cost against the expectation."""
    import torch
    x = C.kernel_expectation(c)
    e = x["e"]
    dev = _dev()
    cur, r0, r1 = (P.DevicePicture(x["ys"][i], dev) for i in (1, 0, 2))
    st = S.BSa8dDecide(x["nctu"], x["w64"], x["h64"], c.depth, c.level, dev, rng=57, lambda8=c.lambda8, qp=x["qp"])
    assert (st.base_bits, st.bi_bits_delta, st.dir_cost) == (BX.BASE_BITS, BX.BI_BITS_DELTA, BX.DIR_COST)
    assert np.array_equal(st.bit_sizes.cpu().numpy(), BX.IX.s_bitsizes(232))
    if c.table_len != 232:
        st.bit_sizes = st.bit_sizes[:c.table_len].contiguous()
    if x["tu_qp"] is not None:
        st.qp_map, st.lambda8_by_qp = _up(x["tu_qp"][0]), _up(x["lambda8_by_qp"])
    st.dir.fill_(0xa5)
    st.ref0.fill_(0x5a)
    st.ref1.fill_(0x5a)
    for t in (st.mv0_out, st.mv1_out, st.cost):
        t.fill_(GARBAGE)
    st.run(cur, r0, r1, _up(x["recs"][0]), _up(x["recs"][1]))
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy()
    got = {"dir": g(st.dir), "ref0": g(st.ref0), "ref1": g(st.ref1), "mv0_out": g(st.mv0_out).reshape(-1, 2), "mv1_out": g(st.mv1_out).reshape(-1, 2),
           "cost": g(st.cost).reshape(-1, 4)}
    want = {"dir": e["dir"], "ref0": e["ref0"], "ref1": e["ref1"], "mv0_out": BE.full_mv_out(c.level, x["nctu"], e["mv0"], GARBAGE),
            "mv1_out": BE.full_mv_out(c.level, x["nctu"], e["mv1"], GARBAGE), "cost": e["cost"]}
    bad = BE.compare(got, want)
    assert not bad, bad
    return x


@pytest.mark.parametrize("c", C.SEARCHED_CASES, ids=lambda c: c.id)
def test_kernel_on_searched_records(c):
    """Levels 0 - 2 at 8 and 10 bits, 12 bits at level 1, on the records the oracle's search and refinement leave for the 192x128 pictures:
    every outcome of the decision occurs."""
    m = _run_kernel(c)["e"]["masks"]
    assert all(v.any() for v in m.values()), {k: int(v.sum()) for k, v in m.items()}


@pytest.mark.parametrize("c", C.FAR_CASES, ids=lambda c: c.id)
def test_kernel_on_far_vectors_of_every_phase(c):
    """Synthetic records: all 16 phases in both lists (8 at level 2), components up to the search range of 57 samples, into the padded
    border; zero vectors in one list, in both (the zero pair is not tried) and equal record costs."""
    x = _run_kernel(c)
    nb, base = 64 >> (2 * c.level), (0, 64, 80)[c.level]
    for l in (0, 1):
        words = x["recs"][l].reshape(x["nctu"], 85, 2)[:, base:base + nb, 1].reshape(-1)
        vec = np.array([BE.unpack_mv(w) for w in words])
        assert len({(int(a) & 3, int(b) & 3) for a, b in vec}) >= (16 if c.level < 2 else 8) and np.abs(vec).max() == 4 * 57
    flags = x["e"]["cost"][:, 3]
    assert ((flags & BX.FLAG_ZERO_TRIED) == 0).any() and (flags & BX.FLAG_ZERO_WON).any() and (flags & BX.FLAG_LIST1).any()


@pytest.mark.parametrize("c", C.POINT_CASES + C.GRID_CASES + C.HOSTILE_CASES + C.TIE_CASES, ids=lambda c: c.id)
def test_kernel_operating_points_grids_clips_and_ties(c):
    """lambda8 = 0; a QP map with a lambda table; a 100-entry bit table (longer components take its last entry); grids one CTU wide, one
    CTU high and 256x192; black / white checker pictures on which every filter sum clips; ref1 == ref0 with equal vectors at lambda8 = 0,
    where both lists cost exactly what one does and the block must stay single-list."""
    x = _run_kernel(c)
    e = x["e"]
    if c.hostile:
        mx = (1 << c.depth) - 1
        assert all((y == 0).any() and (y == mx).any() for y in x["ys"])
    if c.same_ref:
        searched = (e["cost"][:, 3] & BX.FLAG_ZERO_WON) == 0
        assert searched.any() and (e["dir"][searched] == 1).all()
    if c.table_len == 100:
        full = C.kernel_expectation(c._replace(table_len=232, id=c.id + "-full"))["e"]
        assert (full["cost"][:, :3] != e["cost"][:, :3]).any()


def _b_step(w64, h64, depth, dev, level, qp, b_intra, rng=C.RANGE, subme=C.SUBME):
    return S.Sa8dBFramePipeline(w64, h64, depth, dev, rng=rng, subme=subme, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                                sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B), b_intra=b_intra)


@pytest.mark.parametrize("depth,level,b_intra,wide", [(8, 2, False, False), (8, 2, True, False), (8, 1, False, False), (8, 1, True, False), (10, 0, False, False),
                                                      (10, 0, True, False), (8, 2, True, True)])
def test_b_step_every_stage_equals_the_oracle_chain(depth, level, b_intra, wide):
    """Sa8dBFramePipeline.run with chroma, deblocking, SAO applied with the rate-distortion parameters and sign hiding on 192x128 and once
    on 256x192, with and without b_intra: refined vectors of both lists, dir / ref ids / decided vectors / the four cost words, intra flags
    and modes, luma + chroma levels, numSig, SSE, Bs maps, SAO statistics + parameters and the final Y / Cb / Cr planes - and the same
    again from a second run over the finished buffers."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    qp = 30 + 6 * (depth - 8)
    pics = C.pictures(depth, 256, 192) if wide else C.pictures(depth)
    r0, cur, r1 = (P.DevicePicture(y, dev, u, v) for (y, u, v) in pics)
    pipe = _b_step(cur.w64, cur.h64, depth, dev, level, qp, b_intra)
    hp = [PC.padded(p) for p in pics]
    cpu_out = BX.sa8d_b_chain(depth, hp[1], hp[0], hp[2], cur.w64, cur.h64, C.RANGE, C.SUBME, level, qp, b_intra, sao_rdo=pipe.sao_rdo,
                              cores=B.effective_cpus(), avx2=BX.O.host_has_avx2())
    for run in range(2):
        marks = []
        pipe.run(cur, r0, r1, mark=marks.append)
        torch.cuda.synchronize()
        assert marks == ["me0", "subpel0", "me1", "subpel1", "b_sa8d", "recon", "recon_chroma"] + (["intra"] if b_intra else []) + \
                        ["deblock", "sao_stats", "sao_rdo", "sao_apply", "border"]
        bad = BE.compare(BX.device_outputs(pipe, cur.host.dtype), cpu_out)
        assert not bad, (run, bad)
    assert all((cpu_out["dir"] == d).any() for d in (1, 2, 3)), np.bincount(cpu_out["dir"], minlength=4).tolist()
    if b_intra:
        intra = cpu_out["intra"].astype(bool)
        assert (intra & (cpu_out["dir"] == 3)).any() and (intra & (cpu_out["dir"] != 3)).any() and not intra.all()
        assert (cpu_out["bs_ver"] == 2).any() and (cpu_out["bs_ver"] < 2).any()
        assert set(pipe.checksum()) >= {"mode", "intra", "dir", "b_cost", "levels", "recon"}
    else:
        assert not (cpu_out["bs_ver"] == 2).any() and "intra" not in cpu_out


def test_b_step_hands_qp_maps_to_the_decision():
    """set_qp_maps on the step: the decision prices every block with the lambda of its own luma quantiser QP (a map with both range ends
    and entries outside the range), the intra walk gets the three planes, and set_qp_maps(None) restores the picture-wide lambda."""
    import torch
    QE = C.QE
    dev = _dev()
    depth, level, qp = 8, 1, 30
    pics = C.pictures(depth)
    r0, cur, r1 = (P.DevicePicture(y, dev, u, v) for (y, u, v) in pics)
    pipe = _b_step(cur.w64, cur.h64, depth, dev, level, qp, True)
    tu = PC.tu_qp_map(depth, level)
    lam = QE.lambda8_table(depth)
    maps = S.CuQpMaps(cur.w64, cur.h64, depth, level, dev).load(np.clip(tu[0], 0, 51), tu)
    pipe.set_qp_maps(maps, _up(lam))
    assert pipe.bd.qp_map.data_ptr() == maps.tu_qp[0].data_ptr() and pipe.ii.qp_map is maps.tu_qp and pipe.ii.lambda8_by_qp is pipe.bd.lambda8_by_qp
    x = C.kernel_expectation(C._case(depth, level))
    plain = x["e"]
    for with_maps in (True, False):
        if not with_maps:
            pipe.set_qp_maps(None)
        pipe.run(cur, r0, r1)
        torch.cuda.synchronize()
        recs = [pipe.spl[l].out.cpu().numpy().reshape(-1, 2) for l in (0, 1)]
        assert all(np.array_equal(a, b) for a, b in zip(recs, x["recs"]))
        want = BX.decide(depth, x["cur"], x["refs"], x["w64"], x["h64"], level, recs, table=BX.IX.s_bitsizes(4 * C.RANGE + 4), qp=qp, tu_qp=tu,
                         lambda8_by_qp=lam, with_reference=False) if with_maps else plain
        assert np.array_equal(pipe.bd.cost.cpu().numpy().reshape(-1, 4), want["cost"]) and np.array_equal(pipe.bd.dir.cpu().numpy(), want["dir"])
        if with_maps:
            assert (want["cost"][:, :3] != plain["cost"][:, :3]).any()


def test_mini_gop_with_the_step_as_b_step():
    """MiniGop with an i_step, IntraPFramePipeline as p_step and Sa8dBFramePipeline(b_intra) as b_step, gop 3, three anchors (7 pictures of
    192x128): every B picture equals the oracle chain fed the two coded anchors around it, and the anchors equal those of a run with the
    old BFramePipeline as b_step - B pictures change nothing a P picture sees."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    depth, level, qp, gop = 8, 2, 30, 3
    clip = BE.occluded_clip(C.WIDTH, C.HEIGHT, 7, depth, 71)
    new = C.cell_kind(*np.mgrid[0:C.HEIGHT, 0:C.WIDTH]) == ord("N")
    for k in (1, 2, 4, 5):                                     # content the anchors lack, in the B pictures only
        clip[k][0][new] = C.pictures(depth)[1][0][new]
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    w64, h64 = pics[0].w64, pics[0].h64

    def steps(b_step):
        i_step = S.IFramePipeline(w64, h64, depth, dev, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                                  sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_I))
        p_step = S.IntraPFramePipeline(w64, h64, depth, dev, rng=C.RANGE, subme=C.SUBME, level=level, qp=qp, deblock=True, sao=True, chroma=True,
                                       sao_apply=True, sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P))
        return S.MiniGop(p_step, b_step, gop, i_step=i_step)
    b_step = _b_step(w64, h64, depth, dev, level, qp, True)
    order, out = steps(b_step).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 3, 1, 2, 6, 4, 5] and sorted(out) == list(range(7))
    old = S.BFramePipeline(w64, h64, depth, dev, rng=C.RANGE, subme=C.SUBME, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                           sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B))
    _, out_old = steps(old).run(pics)
    torch.cuda.synchronize()
    for a in (0, 3, 6):
        for g, e in zip(out[a], out_old[a]):
            assert torch.equal(g.reshape(-1), e.reshape(-1)), f"anchor {a} depends on the B step"
    dt = pics[0].host.dtype
    shape = pics[0].host.shape
    host = {k: [p.cpu().numpy().view(dt).reshape(-1) for p in planes] for k, planes in out.items()}
    cores, avx2 = B.effective_cpus(), BX.O.host_has_avx2()
    intra_blocks = 0
    for a in (3, 6):
        r0, r1 = ((host[i][0].reshape(shape), host[i][1], host[i][2]) for i in (a - gop, a))
        for k in range(a - gop + 1, a):
            ob = BX.sa8d_b_chain(depth, BE.padded_planes(clip[k])[0], r0, r1, w64, h64, C.RANGE, C.SUBME, level, qp, True, sao_rdo=b_step.sao_rdo,
                                 cores=cores, avx2=avx2)
            for name, g, e in zip(("Y", "Cb", "Cr"), host[k], (ob["recon"], ob["recon_c0"], ob["recon_c1"])):
                e = e.reshape(-1)
                assert g.shape == e.shape and np.array_equal(g, e), f"picture {k} {name}: {int(np.count_nonzero(g != e))} of {e.size} samples differ"
            intra_blocks += int(ob["intra"].sum())
            assert any(not torch.equal(g.reshape(-1), e.reshape(-1)) for g, e in zip(out[k], out_old[k])), f"picture {k}: the new step changed nothing"
    assert intra_blocks > 0
