"""GPU parity of the intra-in-inter stages of a P picture: x265hip_inter_sa8d_cost against the oracle's numbers, x265hip_intra_in_inter
against the coding-order walk of tests/intra_inter_expect.py on the pictures and operating points of tests/intra_inter_cases.py,
stages.IntraPFramePipeline stage by stage against the oracle chain, and MiniGop with the step as its p_step.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import intra_expect as IE
import intra_inter_cases as C
import intra_inter_expect as IX
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")


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


COST_CASES = [C._case(k, d, l) for d in (8, 10) for l, k in ((0, "split"), (1, "swapped"), (2, "split"))] + [C._case("swapped", 12, 1)] + \
             [C._case("split", 8, 1, maps="map-lambda"), C._case("swapped", 10, 2, "qp-max")]


@pytest.mark.parametrize("c", **_ids(COST_CASES))
def test_inter_sa8d_cost_equals_the_oracle(c):
    """Levels 0 - 2 at 8 and 10 bits, 12 bits at level 1: {sa8d, cost} of every block bit for bit.  The vectors are the cases': the true
    sub-pel shift on one side, the 16 phases (all of them at levels 0 and 1) and up to 50 samples (into the extended border) on the other.  A second launch with a
    100-entry table prices the longer components with the table's last entry; one case has a QP map and a lambda table, one lambda8 0."""
    import torch
    x = C.inter_expectation(c)
    dev = _dev()
    cur = P.DevicePicture(x["cur"][0], dev)
    ref = P.DevicePicture(x["ref"][0], dev)
    vec = np.array(C.vectors(c.kind, c.level))
    assert len({(int(a) & 3, int(b) & 3) for a, b in vec}) >= (15 if c.level < 2 else 8) and np.abs(vec).max() >= 4 * 45
    st = S.InterSa8dCost((x["w64"] // 64) * (x["h64"] // 64), x["w64"], x["h64"], c.depth, c.level, dev, rng=57,
                         base_bits=IX.BASE_BITS, lambda8=x["lambda8"], qp=x["qp"])
    assert np.array_equal(st.bit_sizes.cpu().numpy(), x["table"])
    if x["tu_qp"] is not None:
        st.qp_map, st.lambda8_by_qp = _up(x["tu_qp"][0]), _up(x["lambda8_by_qp"])
    st.cost.fill_(-7)
    st.run(cur, ref, _up(x["mv"]))
    torch.cuda.synchronize()
    got = st.cost.cpu().numpy().reshape(-1, 2)
    want = x["inter"]["inter_cost"]
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    # a short table: components of 100 quarter samples and more take its last entry
    short = IX.inter_side(c.depth, x["pcur"], x["pref"], x["w64"], x["h64"], c.level, x["mv"], x["qp"], x["qp_c"], c.flags, chroma=False, tu_qp=x["tu_qp"],
                          lambda8=max(x["lambda8"], 512), lambda8_by_qp=x["lambda8_by_qp"], table=x["table"][:100])["inter_cost"]
    st.bit_sizes, st.lambda8 = st.bit_sizes[:100].contiguous(), max(x["lambda8"], 512)
    st.run(cur, ref, _up(x["mv"]))
    torch.cuda.synchronize()
    assert np.array_equal(st.cost.cpu().numpy().reshape(-1, 2), short)
    assert (short[:, 1] != want[:, 1]).any() or x["lambda8_by_qp"] is not None


def _run_stage(c, x):
    """The stage alone on a case: the oracle's inter coding uploaded as the stage's input, mode / intra / cost pre-filled with garbage, two
    runs into the same buffers - the second over what the first left: a block reads only blocks before it in coding order, and those
    hold their final reconstruction either way, so the result is the same - everything against the walk x["e"]."""
    import torch
    dev = _dev()
    e, it = x["e"], x["inter"]
    w64, h64 = x["w64"], x["h64"]
    nctu = (w64 // 64) * (h64 // 64)
    cur = P.DevicePicture(x["cur"][0], dev, x["cur"][1], x["cur"][2]) if c.chroma else P.DevicePicture(x["cur"][0], dev)
    dt = cur.host.dtype
    ii = S.IntraInInter(nctu, w64, h64, c.depth, c.level, x["qp"], dev, flags=c.flags, chroma=c.chroma, qp_c=x["qp_c"], lambda8=x["lambda8"],
                        mode_bits=x["mode_bits"], want_cost=True)
    if x["tu_qp"] is not None:
        ii.qp_map = _up(x["tu_qp"])
        ii.lambda8_by_qp = None if x["lambda8_by_qp"] is None else _up(x["lambda8_by_qp"])
    rc = S.InterRecon(nctu, w64, h64, c.depth, c.level, x["qp"], dev, intra_slice=c.flags)
    rc_c = [S.InterReconChroma(nctu, w64, h64, c.depth, c.level, x["qp_c"][i], dev, intra_slice=c.flags) for i in range(2)] if c.chroma else None
    sfx = ["", "_c0", "_c1"] if c.chroma else [""]
    # the numbers the walk decided against (the oracle's costs, or the supplied tie pattern): one word per block, stride 1
    ic = _up(e["inter_cost"].astype(np.int32))
    want = {k: v for k, v in e.items() if k not in ("masks", "tables", "inter_cost")}
    for run in range(2):
        if run == 0:
            rec = [_up(it["recon" + s]) for s in sfx]
            for st, s in zip([rc] + (rc_c or []), sfx):
                st.levels.copy_(_up(it["levels" + s]))
                st.num_sig.copy_(_up(it["num_sig" + s]))
                st.dist.copy_(_up(it["dist" + s]))
            ii.mode.fill_(0xa5)
            ii.intra.fill_(0x5a)
            ii.cost.fill_(-3)
        ch = None
        if c.chroma:
            ch = dict(fenc=cur.c, recon=rec[1:], stride=cur.stride_c, org=cur.org_c, qp=ii.qp_c, levels=[r.levels for r in rc_c],
                      num_sig=[r.num_sig for r in rc_c], dist=[r.dist for r in rc_c])
        H.intra_in_inter(c.depth, w64, h64, c.level, x["qp"], c.flags, x["lambda8"], x["mode_bits"], cur.t, cur.stride, cur.org, rec[0], ii.mode, rc.levels,
                         rc.num_sig, rc.dist, ic, ii.intra, inter_cost_stride=1, inter_cost_offset=0, chroma=ch, cost=ii.cost, qp_map=ii.qp_map,
                         lambda8_by_qp=ii.lambda8_by_qp)
        torch.cuda.synchronize()
        got = {"mode": ii.mode.cpu().numpy(), "intra": ii.intra.cpu().numpy(), "cost": ii.cost.cpu().numpy().reshape(-1, 2), "levels": rc.levels.cpu().numpy(),
               "num_sig": rc.num_sig.cpu().numpy(), "dist": rc.dist.cpu().numpy(), "recon": rec[0].cpu().numpy().view(dt)}
        for i in range(2 if c.chroma else 0):
            got.update({"levels_c%d" % i: rc_c[i].levels.cpu().numpy(), "num_sig_c%d" % i: rc_c[i].num_sig.cpu().numpy(), "dist_c%d" % i: rc_c[i].dist.cpu().numpy(),
                        "recon_c%d" % i: rec[1 + i].cpu().numpy().view(dt)})
        assert set(got) == set(want)
        bad = BE.compare(got, want)
        assert not bad, (run, bad)
    return e


def _run_case(c):
    return _run_stage(c, C.expectation(c))


@pytest.mark.parametrize("c", **_ids(C.MID_CASES))
def test_intra_in_inter_equals_the_walk(c):
    """192x128, split and swapped at the mid QP with sign hiding on and off, levels 0 - 2, 8 bits; 10 and 12 bits: intra, mode, cost,
    levels, numSig, dist and the Y / Cb / Cr planes bit for bit."""
    m = _run_case(c)["masks"]
    assert m["intra_won"].any() and m["inter_won"].any() and m["intra_reads_inter_recon_across_ctu"].any()


@pytest.mark.parametrize("c", **_ids(C.WHOLE_CASES + C.QP_END_CASES))
def test_intra_in_inter_whole_pictures_and_qp_ends(c):
    """All-new and pure-shift pictures (one candidate wins nearly everywhere), QP 0 and the largest QP (lambda8 0)."""
    _run_case(c)


@pytest.mark.parametrize("c", **_ids(C.TIE_CASES))
def test_intra_in_inter_ties_stay_inter(c):
    """Supplied inter costs of intra cost - 1 / + 0 / + 1 by block index modulo 3: a tie stays inter."""
    e = _run_case(c)
    b = np.arange(len(e["intra"]))
    assert np.array_equal(e["intra"], (b % 3 == 2).astype(np.uint8)) and e["masks"]["tie_stays_inter"].mean() > 0.3


@pytest.mark.parametrize("c", **_ids(C.MAP_CASES))
def test_intra_in_inter_under_qp_maps(c):
    """A tu_qp map with 0, 1, max - 1, max and entries outside the range, with and without a lambda8_by_qp table."""
    _run_case(c)


@pytest.mark.parametrize("c", **_ids(C.LUMA_ONLY_CASES))
def test_intra_in_inter_without_chroma(c):
    e = _run_case(c)
    assert "recon_c0" not in e and e["intra"].any()


@pytest.mark.parametrize("w,h", [(64, 128), (192, 64)])
def test_intra_in_inter_degenerate_grids(w, h):
    """One CTU column (every odd wave is empty) and one CTU row: the top-left w x h of the split pair, level 1, 8 bits."""
    c = C._case("split", 8, 1)
    ref, cur = C.pictures(c.kind, c.depth)
    crop = lambda yuv: (yuv[0][:h, :w], yuv[1][:h // 2, :w // 2], yuv[2][:h // 2, :w // 2])
    ref, cur = crop(ref), crop(cur)
    pr, pc = C.padded(ref), C.padded(cur)
    qp, lambda8, mode_bits = C.IC.point("mid", 8)
    qpc = C.IC.chroma_qp(qp, 8)
    nctu = (w // 64) * (h // 64)
    mv = IX.mv_records([C.SHIFTS["split"] if (b // 3) % 2 else (4 * (b % 9) - 13, 7 - 3 * (b % 5)) for b in range(nctu * 16)], 1, nctu)
    it = IX.inter_side(8, pc, pr, w, h, 1, mv, qp, (qpc, qpc), c.flags)
    e = IX.walk(8, pc, w, h, 1, qp, it, qp_c=(qpc, qpc), flags=c.flags, lambda8=lambda8, mode_bits=mode_bits)
    assert e["intra"].any() and not e["intra"].all()
    _run_stage(c, dict(ref=ref, cur=cur, w64=w, h64=h, qp=qp, qp_c=(qpc, qpc), lambda8=lambda8, mode_bits=mode_bits, tu_qp=None, lambda8_by_qp=None, inter=it, e=e))


def _p_step(w64, h64, depth, dev, level, qp, rng, subme):
    return S.IntraPFramePipeline(w64, h64, depth, dev, rng=rng, subme=subme, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                                 sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P))


def _wide_pair(depth):
    """256x192: the split pair tiled and cropped (4x3 CTUs)."""
    ref, cur = C.pictures("split", depth)
    tile = lambda p, h, w: np.tile(p, (2, 2))[:h, :w]
    return tuple(tile(p, 192 >> (i > 0), 256 >> (i > 0)) for i, p in enumerate(ref)), tuple(tile(p, 192 >> (i > 0), 256 >> (i > 0)) for i, p in enumerate(cur))


@pytest.mark.parametrize("depth,level,wide", [(8, 2, False), (8, 1, False), (10, 0, False), (8, 2, True)])
def test_p_step_every_stage_equals_the_oracle_chain(depth, level, wide):
    """IntraPFramePipeline.run with chroma, deblocking, SAO applied with the rate-distortion parameters and sign hiding on 192x128 and once
    on 256x192: refined vectors, inter costs, intra flags, modes, luma + chroma levels, numSig, SSE, Bs maps (2 on the edges of intra
    blocks), SAO statistics + parameters and the final Y / Cb / Cr planes."""
    import torch
    B = importlib.import_module("bench")
    dev = _dev()
    qp, rng, subme = 30 + 6 * (depth - 8), 12, 2
    ref_yuv, cur_yuv = _wide_pair(depth) if wide else C.pictures("split", depth)
    cur, ref = P.DevicePicture(cur_yuv[0], dev, cur_yuv[1], cur_yuv[2]), P.DevicePicture(ref_yuv[0], dev, ref_yuv[1], ref_yuv[2])
    pipe = _p_step(cur.w64, cur.h64, depth, dev, level, qp, rng, subme)
    marks = []
    pipe.run(cur, ref, mark=marks.append)
    torch.cuda.synchronize()
    assert marks == ["me", "subpel", "recon", "recon_chroma", "inter_cost", "intra", "deblock", "sao_stats", "sao_rdo", "sao_apply", "border"]
    dev_out = IX.p_device_outputs(pipe, cur.host.dtype)
    cpu_out = IX.p_chain(depth, C.padded(cur_yuv), C.padded(ref_yuv), cur.w64, cur.h64, rng, subme, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(),
                         avx2=IE.O.host_has_avx2())
    bad = BE.compare(dev_out, cpu_out)
    assert not bad, bad
    share = cpu_out["intra"].mean()
    assert 0.2 <= share <= 0.8, share
    assert (cpu_out["bs_ver"] == 2).any() and (cpu_out["bs_ver"] < 2).any()
    assert set(pipe.checksum()) >= {"mode", "intra", "inter_cost", "levels", "recon"}


def test_mini_gop_with_the_step_as_p_step():
    """MiniGop with an i_step and IntraPFramePipeline as p_step, gop 1, three anchors of 192x128 (the split pair's reference, its current picture, the reference again): every
    anchor is what the step alone produces from the previous coded anchor, and intra blocks appear in both P pictures."""
    import torch
    dev = _dev()
    depth, level, qp, rng, subme = 8, 2, 30, 12, 2
    ref_yuv, cur_a = C.pictures("split", depth)
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
        share = float(alone.ii.intra.float().mean().item())
        assert 0.1 < share < 0.9, (a, share)
        prev = pics[a].like([p.clone() for p in out[a]])
