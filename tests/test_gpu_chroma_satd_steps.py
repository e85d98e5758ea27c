"""GPU parity of the P and B steps with chroma SATD (FramePipeline / BFramePipeline / MiniGop with chroma_satd=True) at 256 x 192: the
sub-pel records against the walk of tests/subpel_chroma_expect.py, the bidirectional decision against its formula on the oracle's captured
predictions, and every later stage against the oracle chain fed with those records.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import qp_map_expect as QE
import subpel_chroma_expect as CE

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")

W, H, R, SUBME, LEVEL = 256, 192, 12, 3, 2


def _qp(depth):
    return 30 + 12 * (depth == 10)


def _p_step(w64, h64, depth, dev, chroma_satd, **kw):
    return S.FramePipeline(w64, h64, depth, dev, rng=R, subme=SUBME, level=LEVEL, qp=_qp(depth), want_surf=False, deblock=True, chroma=True, sign_hide=True,
                           chroma_satd=chroma_satd, **kw)


def _b_step(w64, h64, depth, dev):
    return S.BFramePipeline(w64, h64, depth, dev, rng=R, subme=SUBME, level=LEVEL, qp=_qp(depth), deblock=True, chroma=True, sign_hide=True, want_cost=True,
                            chroma_satd=True)


def _pictures(clip, dev):
    return [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]


@pytest.mark.parametrize("mode", ["plain", "planes", "parallel", "split"])
@pytest.mark.parametrize("depth", [8, 10])
def test_p_step_with_chroma_satd_equals_the_chain(depth, mode):
    """One closed-loop step of every run mode that reaches the refinement: plain, luma candidates from phase planes, parallel planes, and
    parallel planes in two parts.  The records are the chroma walk's and differ from the luma-only refinement's."""
    import torch
    dev = torch.device("cuda:0")
    clip = BE.occluded_clip(W, H, 2, depth, 31)
    pics = _pictures(clip, dev)
    kw = {"plain": {}, "planes": {"subpel_planes": True}, "parallel": {"parallel_planes": True}, "split": {"parallel_planes": True, "split": 2}}[mode]
    pipe = _p_step(pics[0].w64, pics[0].h64, depth, dev, True, **kw)
    pipe.run(pics[1], pics[0])
    torch.cuda.synchronize()
    pad = [BE.padded_planes(c)[0] for c in clip]
    want = CE.p_chain(depth, pad[1], pad[0], pics[0].w64, pics[0].h64, R, SUBME, LEVEL, _qp(depth), True)
    bad = BE.compare(QE.step_outputs(pipe, pics[0].host.dtype, "p"), want)
    assert not bad, bad
    luma = CE.p_chain(depth, pad[1], pad[0], pics[0].w64, pics[0].h64, R, SUBME, LEVEL, _qp(depth), False)
    assert np.count_nonzero(want["subpel_mv"][:, 1] != luma["subpel_mv"][:, 1]) > want["subpel_mv"].shape[0] // 50          # vectors, not only costs
    assert int(want["num_sig"].sum()) > 0


@pytest.mark.parametrize("depth", [8, 10])
def test_p_step_without_chroma_satd_is_the_luma_only_chain(depth):
    import torch
    dev = torch.device("cuda:0")
    clip = BE.occluded_clip(W, H, 2, depth, 31)
    pics = _pictures(clip, dev)
    pipe = _p_step(pics[0].w64, pics[0].h64, depth, dev, False)
    pipe.run(pics[1], pics[0])
    torch.cuda.synchronize()
    pad = [BE.padded_planes(c)[0] for c in clip]
    want = CE.p_chain(depth, pad[1], pad[0], pics[0].w64, pics[0].h64, R, SUBME, LEVEL, _qp(depth), False)
    bad = BE.compare(QE.step_outputs(pipe, pics[0].host.dtype, "p"), want)
    assert not bad, bad


def _b_outputs(pipe, dt):
    out = QE.step_outputs(pipe, dt, "b")
    g = lambda t: t.cpu().numpy()
    out.update({"subpel_mv0": g(pipe.spl[0].out).reshape(-1, 2), "subpel_mv1": g(pipe.spl[1].out).reshape(-1, 2), "ref0": g(pipe.bd.ref0), "ref1": g(pipe.bd.ref1),
                "cost_out": g(pipe.bd.cost_out).reshape(-1, 4)})
    return out


@pytest.mark.parametrize("depth", [8, 10])
def test_b_step_with_chroma_satd_equals_the_chain(depth):
    """Both lists' records, dir / ref ids / decided vectors / costs, luma + chroma levels, numSig, SSE, Bs maps and the final planes."""
    import torch
    dev = torch.device("cuda:0")
    clip = BE.occluded_clip(W, H, 3, depth, 33)
    pics = _pictures(clip, dev)
    pipe = _b_step(pics[0].w64, pics[0].h64, depth, dev)
    pipe.run(pics[1], pics[0], pics[2])
    torch.cuda.synchronize()
    pad = [BE.padded_planes(c)[0] for c in clip]
    want = CE.b_chain(depth, pad, pics[0].w64, pics[0].h64, R, SUBME, LEVEL, _qp(depth))
    masks = want.pop("masks")
    bad = BE.compare(_b_outputs(pipe, pics[0].host.dtype), want)
    assert not bad, bad
    assert all((want["dir"] == d).any() for d in (1, 2, 3)), np.bincount(want["dir"], minlength=4).tolist()
    print({k: round(float(m.mean()), 3) for k, m in masks.items()})


def test_mini_gop_of_five_pictures_with_chroma_satd():
    """gop 2, 5 pictures in display order: anchors 0, 2, 4 form the P chain, 1 and 3 are B pictures between the coded anchors; both steps
    measure chroma.  The final planes of all five equal the chains run in coding order on the CPU."""
    import torch
    dev = torch.device("cuda:0")
    depth, gop = 8, 2
    clip = BE.occluded_clip(W, H, 5, depth, 35)
    pics = _pictures(clip, dev)
    w64, h64 = pics[0].w64, pics[0].h64
    order, out = S.MiniGop(_p_step(w64, h64, depth, dev, True), _b_step(w64, h64, depth, dev), gop).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3]
    dt = pics[0].host.dtype
    pad = [BE.padded_planes(c)[0] for c in clip]
    planes_of = lambda o: (o["recon"], o["recon_c0"], o["recon_c1"])
    want = {0: pad[0]}
    for a in (2, 4):
        want[a] = planes_of(CE.p_chain(depth, pad[a], want[a - gop], w64, h64, R, SUBME, LEVEL, _qp(depth), True))
        want[a - 1] = planes_of(CE.b_chain(depth, [want[a - gop], pad[a - 1], want[a]], w64, h64, R, SUBME, LEVEL, _qp(depth)))
    for k in range(5):
        for name, g, e in zip(("Y", "Cb", "Cr"), out[k], want[k]):
            g, e = g.cpu().numpy().view(dt).reshape(-1), np.asarray(e).reshape(-1)
            assert g.shape == e.shape and np.array_equal(g, e), f"picture {k} {name}: {int(np.count_nonzero(g != e))} of {e.size} samples differ"


def test_refused_modes_raise():
    import torch
    dev = torch.device("cuda:0")
    with pytest.raises(ValueError, match="search"):
        S.FramePipeline(W, H, 8, dev, rng=R, subme=SUBME, chroma=True, chroma_satd=True, search="hex")
    with pytest.raises(ValueError, match="chroma=True"):
        S.FramePipeline(W, H, 8, dev, rng=R, subme=SUBME, chroma_satd=True)
    with pytest.raises(ValueError, match="chroma=True"):
        S.BFramePipeline(W, H, 8, dev, rng=R, subme=SUBME, chroma_satd=True)
    with pytest.raises(ValueError, match="chroma_satd"):
        S.BandedFramePipeline(W, H, 8, dev, band_rows=1, rng=R, subme=SUBME, chroma=True, chroma_satd=True)
