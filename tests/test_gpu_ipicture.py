"""GPU parity of the I-picture stage (x265hip_intra_picture, stages.IntraPicture), of the I step (stages.IFramePipeline) and of the
mini-GOP driver with an i_step against the coding-order walk of tests/intra_expect.py and the oracle chain behind it: the walk ->
deblock_bs_inter(intra = all ones) -> deblock_luma / deblock_chroma -> sao_stats / sao_rdo / sao_apply -> border extension.  The stage
alone also runs on the hostile pictures and operating points of tests/intra_cases.py: the edge filter's clip, ties, a rate term of 2^36,
both ends of the QP range, no chroma planes.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import intra_cases as IC
import intra_expect as IE
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")

_cache = {}


def _case(depth, w, h, level, flags, strong):
    """The walk's expectation on intra_expect.test_picture at the mid operating point, computed once per case and shared (nothing modifies
    it): the dict intra_cases.expectation returns for its cases."""
    key = (depth, w, h, level, flags, strong)
    if key not in _cache:
        yuv = IE.test_picture(depth, w, h)
        pl, w64, h64 = IE.padded_planes(yuv)
        qp = 30 + 6 * (depth - 8)
        qpc = S.chroma_quant_qp(qp, depth)
        init = IE.garbage_planes(depth, [np.asarray(p).reshape(-1).shape for p in pl])
        e = IE.expect(depth, pl, w64, h64, level, qp, qp_c=(qpc, qpc), flags=flags, strong=strong, recon_init=init, with_reference=False)
        _cache[key] = dict(yuv=yuv, w64=w64, h64=h64, qp=qp, qp_c=(qpc, qpc), lambda8=IE.LAMBDA8, mode_bits=IE.MODE_BITS, init=init, e=e)
    return _cache[key]


def _run(x, depth, level, flags, strong, chroma=True):
    """x: a picture, an operating point, the recon planes' contents before the run and the walk's expectation (_case /
    intra_cases.expectation).  Two runs into recon planes pre-filled with garbage; every output and the whole planes against the walk."""
    import torch
    dev = torch.device("cuda:0")
    yuv, w64, h64, init, e = x["yuv"], x["w64"], x["h64"], x["init"], x["e"]
    cur = P.DevicePicture(yuv[0], dev, yuv[1], yuv[2])
    dt = cur.host.dtype

    def up(a):
        return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int16)).to(dev)
    ip = S.IntraPicture((w64 // 64) * (h64 // 64), w64, h64, depth, level, x["qp"], dev, flags=flags, chroma=chroma, qp_c=x["qp_c"], lambda8=x["lambda8"],
                        mode_bits=x["mode_bits"], strong_intra_smoothing=strong, want_cost=True)
    assert ip.waves == IE.waves(w64, h64)
    runs = []
    for _ in range(2):                                   # the second run goes into the buffers the first one left
        if not runs:
            rec = [up(p.copy()) for p in init]           # recon planes pre-filled with garbage
        ip.run(cur, rec[0], rec[1:] if chroma else None)
        torch.cuda.synchronize()
        got = {"mode": ip.mode.cpu().numpy(), "cost": ip.cost.cpu().numpy().reshape(-1, 2), "levels": ip.levels.cpu().numpy(),
               "num_sig": ip.num_sig.cpu().numpy(), "dist": ip.dist.cpu().numpy(), "recon": rec[0].cpu().numpy().view(dt)}
        for c in range(2 if chroma else 0):
            got.update({"levels_c%d" % c: ip.levels_c[c].cpu().numpy(), "num_sig_c%d" % c: ip.num_sig_c[c].cpu().numpy(),
                        "dist_c%d" % c: ip.dist_c[c].cpu().numpy(), "recon_c%d" % c: rec[1 + c].cpu().numpy().view(dt)})
        runs.append(got)
    want = {k: v for k, v in e.items() if k not in ("masks", "tables")}
    assert set(want) == set(runs[0])
    # whole planes are compared: the margins of the recon planes stay as they were pre-filled
    bad = BE.compare(runs[0], want)
    assert not bad, bad
    # a second run over a finished reconstruction changes nothing
    again = BE.compare(runs[1], want)
    assert not again, again
    assert set(ip.checksum()) >= ({"mode", "levels", "num_sig", "dist", "levels_c0", "levels_c1"} if chroma else {"mode", "levels", "num_sig", "dist"})
    return e


def _run_kernel(depth, w, h, level, flags, strong):
    return _run(_case(depth, w, h, level, flags, strong), depth, level, flags, strong)


def _run_case(c):
    """One case of tests/intra_cases.py (what each is listed for is asserted, with the walk alone, by tests/test_intra_cases_cpu.py)."""
    x = IC.expectation(c)
    assert x["qp_c"][0] == S.chroma_quant_qp(x["qp"], c.depth)
    return _run(x, c.depth, c.level, c.flags, c.strong, c.chroma)


def _ids(cases):
    return dict(argvalues=cases, ids=[c.id for c in cases])


@pytest.mark.parametrize("depth,level,sign_hide,strong", [(8, 0, True, True), (8, 0, False, True), (8, 1, True, True), (8, 1, False, True), (8, 2, True, True),
                                                          (10, 0, True, True), (10, 0, False, True), (10, 1, True, True), (10, 1, False, True), (10, 2, True, True),
                                                          (12, 1, True, True), (8, 2, False, False), (10, 2, False, True), (10, 2, True, False)])
def test_intra_picture_equals_the_walk(depth, level, sign_hide, strong):
    """256x192 (4x3 CTUs: the smallest grid with a CTU that has all eight neighbours and two lags of the wavefront), levels 0 / 1 / 2 at 8 and
    10 bits each with sign hiding on and off, 12 bits at level 1, strong smoothing on and off at level 2; recon planes pre-filled with garbage; two
    runs.  Bit for bit: mode, cost, levels, num_sig, dist and the Y / Cb / Cr planes."""
    flags = H.TU_INTRA_SLICE | (H.TU_SIGN_HIDE if sign_hide else 0)
    e = _run_kernel(depth, 256, 192, level, flags, strong)
    m = e["masks"]
    assert m["dc"].any() and m["planar"].any() and m["angular_lt18"].any() and m["angular_ge18"].any() and m["non_mpm"].any() and m["bits_flip"].any()
    if level == 2:
        assert m["strong_taken"].any() == strong and (not strong or m["strong_refused"].any())


@pytest.mark.parametrize("w,h", [(64, 64), (64, 192), (256, 64)])
@pytest.mark.parametrize("depth,level", [(8, 1), (10, 2)])
def test_intra_picture_degenerate_grids(w, h, depth, level):
    """One CTU, one CTU column (every odd wave is empty), one CTU row."""
    _run_kernel(depth, w, h, level, H.TU_INTRA_SLICE | H.TU_SIGN_HIDE, True)


@pytest.mark.parametrize("c", **_ids(IC.CLIPPING_CASES))
def test_intra_picture_on_clipping_content(c):
    """192x128 (3x2 CTUs).  edge_clip pictures at two operating points, all depths, levels 0 and 1: the winners are modes 10 / 26 whose edge
    filter leaves the sample range at both bounds; edges at 8 / 10 bits, levels 0 - 2, sign hiding on and off, strong smoothing off; noise at
    12 bits, levels 0 and 2: reconstructions at 0 and max that the next blocks predict from, chroma coded everywhere."""
    m = _run_case(c)["masks"]
    if c.kind == "edge_clip":
        assert m["edge_clip_lo"].any() and m["edge_clip_hi"].any()
    else:
        assert m["recon_at_limit"].any() and m["chroma_coded"].any()


@pytest.mark.parametrize("c", **_ids(IC.QP_END_CASES))
def test_intra_picture_at_the_ends_of_the_qp_range(c):
    """The largest QP (51 / 63 / 75, lambda8 0) on edges, flat_hi and flat_lo at every depth and level: next to nothing is coded, the picture
    is neighbour substitution carried from block to block with ties everywhere.  QP 0 on edges and noise: the largest levels, at 12 bits
    (levels 1 and 2) both int16 limits."""
    e = _run_case(c)
    if c.point == "qp-max":
        assert e["masks"]["cost_tie"].any() or c.kind == "edges"
    elif c.depth == 12:
        assert e["masks"]["level_sat"].any()


@pytest.mark.parametrize("c", **_ids(IC.TIE_CASES))
def test_intra_picture_ties_follow_the_scan_order(c):
    """halves with mode bits (3, 3, 6) and (6, 3, 2) at 8 / 10 bits, levels 0 - 2, and flat_hi with lambda8 0: most blocks are exact ties,
    and the winner is the first of the tied modes in the order DC, planar, 2 .. 34 - not the most probable one."""
    assert _run_case(c)["masks"]["cost_tie"].any()


@pytest.mark.parametrize("c", **_ids(IC.COST_CASES))
def test_intra_picture_cost_near_its_int32_bound(c):
    """lambda8 2^24 with mode_bits 4096 (bits * lambda8 = 2^36, every reported cost 2^28 + sad) at 8 / 12 bits, levels 0 and 2, and with
    (1, 4095, 4096) - the losers' costs near 2^28, the winner's small - at 10 bits, level 1."""
    e = _run_case(c)
    assert (e["cost"][:, 1] >= 1 << 28).all() or c.point == "big-cost-mpm"


@pytest.mark.parametrize("c", **_ids(IC.LUMA_ONLY_CASES))
def test_intra_picture_without_chroma(c):
    """IntraPicture(chroma=False): luma mode, cost, levels, num_sig, dist and the Y plane equal the walk without chroma (which
    test_intra_cases_cpu.test_luma_does_not_read_chroma shows equal to the luma outputs of the walk with it)."""
    e = _run_case(c)
    assert "recon_c0" not in e and int(e["num_sig"].sum()) > 0


def _i_step(w64, h64, depth, dev, level, qp):
    return S.IFramePipeline(w64, h64, depth, dev, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True,
                            sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_I), want_cost=True)


@pytest.mark.parametrize("depth,width,height", [(8, 256, 192), (10, 256, 192), (8, 1920, 1080)])
def test_i_step_every_stage_equals_the_oracle_chain(depth, width, height):
    """IFramePipeline.run at level 2 with chroma, deblocking, SAO applied with the rate-distortion parameters and sign hiding, at 256x192
    and 1920x1088: modes, luma + chroma levels, numSig, SSE, Bs maps (2 on every block edge), SAO statistics + parameters and the final
    Y / Cb / Cr planes."""
    import torch
    B = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    qp, level = 30 + 12 * (depth == 10), 2
    yuv = IE.test_picture(depth, width, height) if width == 256 else F.synth_clip(width, height, 1, depth=depth, seed=29)[0]
    cur = P.DevicePicture(yuv[0], dev, yuv[1], yuv[2])
    pipe = _i_step(cur.w64, cur.h64, depth, dev, level, qp)
    marks = []
    pipe.run(cur, mark=marks.append)
    torch.cuda.synchronize()
    assert marks == ["intra", "deblock", "sao_stats", "sao_rdo", "sao_apply", "border"]
    dev_out = IE.i_device_outputs(pipe, cur.host.dtype)
    cpu_out = IE.i_chain(depth, IE.padded_planes(yuv)[0], cur.w64, cur.h64, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(), avx2=IE.O.host_has_avx2())
    bad = BE.compare(dev_out, cpu_out)
    assert not bad, bad
    assert int(cpu_out["num_sig"].sum()) > 0 and len(np.unique(cpu_out["mode"])) > 3
    # every block edge inside the picture has Bs 2
    bv = cpu_out["bs_ver"].reshape(cur.h64 // 4, cur.w64 // 8)
    assert (bv[:, 4::4] == 2).all()
    assert set(pipe.checksum()) >= {"mode", "levels", "recon"}


def test_mini_gop_with_an_i_step():
    """MiniGop with an i_step, gop 3, 7 pictures of 256x192: picture 0 is what IFramePipeline alone produces, the first P picture is coded
    from it (and so differs from the run without an i_step), and MiniGop(p, b, gop) without the argument reproduces the old behaviour:
    picture 0 passes through uncoded and the anchors are the P chain from the source picture."""
    import torch
    dev = torch.device("cuda:0")
    depth, W, Hh, R, subme, level, gop, qp = 8, 256, 192, 12, 3, 2, 3, 30
    clip = BE.occluded_clip(W, Hh, 7, depth, 71)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    w64, h64 = pics[0].w64, pics[0].h64
    srdo_p = sao_rdo_inputs(depth, qp, HT.SLICE_P)

    def p_step():
        return S.FramePipeline(w64, h64, depth, dev, rng=R, subme=subme, level=level, qp=qp, want_surf=False, deblock=True, sao=True, chroma=True,
                               sao_apply=True, sign_hide=True, sao_rdo=srdo_p)

    def b_step():
        return S.BFramePipeline(w64, h64, depth, dev, rng=R, subme=subme, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                                sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B))
    order_i, out_i = S.MiniGop(p_step(), b_step(), gop, i_step=_i_step(w64, h64, depth, dev, level, qp)).run(pics)
    order_0, out_0 = S.MiniGop(p_step(), b_step(), gop).run(pics)
    torch.cuda.synchronize()
    assert order_i == order_0 == [0, 3, 1, 2, 6, 4, 5] and sorted(out_i) == sorted(out_0) == list(range(7))
    same = lambda a, b: all(torch.equal(x.reshape(-1), y.reshape(-1)) for x, y in zip(a, b))
    # picture 0: the I step alone
    alone = _i_step(w64, h64, depth, dev, level, qp)
    alone.run(pics[0])
    torch.cuda.synchronize()
    assert same(alone.final_planes(), out_i[0]) and not same(out_i[0], pics[0].planes())
    # the first P picture is predicted from the coded picture 0
    assert not same(out_i[3], out_0[3])
    chain = p_step()
    chain.run(pics[3], pics[0].like([p.clone() for p in alone.final_planes()]))
    torch.cuda.synchronize()
    assert same(chain.final_planes(), out_i[3])
    # without the argument: picture 0 as it is, anchors = the P chain from the source picture
    assert same(out_0[0], pics[0].planes())
    ref = pics[0]
    chain = p_step()
    for a in (3, 6):
        chain.run(pics[a], ref)
        torch.cuda.synchronize()
        assert same(chain.final_planes(), out_0[a]), f"anchor {a}"
        ref = pics[a].like([p.clone() for p in chain.final_planes()])
