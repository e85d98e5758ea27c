"""GPU parity of the B-picture step (stages.BFramePipeline) and of the mini-GOP driver (stages.MiniGop) against the oracle chain
me_fullsearch x2 -> subpel_refine x2 -> the bidirectional decision (tests/bidir_expect.py) -> inter_recon_bi / inter_recon_chroma_bi with the
decided dir -> deblock_bs_b -> deblock_luma / deblock_chroma -> sao_stats / sao_rdo / sao_apply -> border extension.  Equal means equal."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import bipred_cases as BC
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")


def _b_step(w64, h64, depth, dev, rng, subme, level, qp, subpel_planes=False):
    return S.BFramePipeline(w64, h64, depth, dev, rng=rng, subme=subme, level=level, qp=qp, deblock=True, sao=True, chroma=True, sao_apply=True,
                            sign_hide=True, subpel_planes=subpel_planes, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B), want_cost=True)


def _check_b_step(depth, width, height, rng, subme, level, seed, subpel_planes, min_values, clip=None):
    import torch
    B = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    qp = 30 + 12 * (depth == 10)
    if clip is None:
        clip = BE.occluded_clip(width, height, 3, depth, seed)
    cur, r0, r1 = (P.DevicePicture(clip[i][0], dev, clip[i][1], clip[i][2]) for i in (1, 0, 2))
    pipe = _b_step(cur.w64, cur.h64, depth, dev, rng, subme, level, qp, subpel_planes)
    marks = []
    pipe.run(cur, r0, r1, mark=marks.append)
    torch.cuda.synchronize()
    assert marks == ["me0", "subpel0", "me1", "subpel1", "bidir", "recon", "recon_chroma", "deblock", "sao_stats", "sao_rdo", "sao_apply", "border"]
    dev_out = BE.b_device_outputs(pipe, cur.host.dtype)
    hp = [BE.padded_planes(clip[i])[0] for i in (1, 0, 2)]
    cpu_out = BE.b_chain(depth, hp[0], hp[1], hp[2], cur.w64, cur.h64, rng, subme, level, qp, sao_rdo=pipe.sao_rdo, cores=B.effective_cpus(),
                         avx2=BE.O.host_has_avx2())
    bad = BE.compare(dev_out, cpu_out)
    assert not bad, bad
    assert sum(np.asarray(v).size for v in cpu_out.values()) > min_values
    assert all((cpu_out["dir"] == d).any() for d in (1, 2, 3)), np.bincount(cpu_out["dir"], minlength=4).tolist()
    assert int(cpu_out["num_sig"].sum()) > 0 and (cpu_out["bs_ver"] > 0).any() and (cpu_out["bs_hor"] > 0).any()
    assert set(pipe.checksum()) >= {"best0", "best1", "subpel0", "subpel1", "dir", "levels", "recon"}
    return cpu_out


@pytest.mark.parametrize("depth,level,subpel_planes", [(8, 2, False), (10, 2, True), (8, 1, True), (10, 1, False)])
def test_b_step_every_stage_equals_the_oracle_chain(depth, level, subpel_planes):
    """BFramePipeline.run at 1024x576 with chroma, deblocking, SAO applied with the rate-distortion parameters and sign hiding, 32x32 and
    16x16 blocks: vectors of both lists, dir / ref ids / decided vectors / costs, luma + chroma levels, numSig, SSE, Bs maps, SAO
    statistics + parameters and the final Y / Cb / Cr planes."""
    _check_b_step(depth, 1024, 576, 12, 3, level, 23, subpel_planes, 2_500_000)


def test_b_step_3840x2160_with_the_bench_settings():
    """The B twin of test_whole_4k_frame_every_stage_equals_oracle_chain: one 3840x2160 8-bit B picture with the bench's settings (range 57,
    subme 3, 32x32 blocks, sub-pel candidates from phase planes) against the chain, all CTUs."""
    _check_b_step(8, 3840, 2160, 57, 3, 2, 265, True, 25_000_000)


@pytest.mark.parametrize("case,level,subpel_planes", BC.B_STEP_CASES, ids=lambda v: v.id if isinstance(v, BC.BiCase) else str(v))
def test_b_step_on_clipping_content(case, level, subpel_planes):
    """The whole B step on the three Y / Cb / Cr pictures of a tests/bipred_cases.py input, 256x128 at the bench's range 57 and subme 3: the
    device's own searches find the planted far vectors in two `edges` references, and every later stage works on predictions that clip."""
    c = BC.build_bi(*case.build)
    cpu_out = _check_b_step(c.depth, case.width, case.height, c.R, 3, level, case.seed, subpel_planes, 100_000, clip=c.yuv)
    inner = cpu_out["recon"][F.MARGIN_Y:F.MARGIN_Y + c.h64, F.MARGIN_X:F.MARGIN_X + c.w64]
    assert (inner == 0).any() and (inner == (1 << c.depth) - 1).any()


@pytest.mark.parametrize("depth", [8, 10])
def test_mini_gop_closed_loop(depth):
    """MiniGop, gop 3, 7 pictures of 512x320 in display order: anchors 0, 3, 6 form the P chain (3 from the source picture 0, 6 from the
    coded picture 3), pictures 1, 2 / 4, 5 are B pictures between the coded anchors.  The final planes of all 7 pictures equal the same
    chain run in coding order on the CPU, and the anchors equal what FramePipeline.run alone produces for them: B pictures change nothing
    a P picture sees."""
    import torch
    B = importlib.import_module("bench")
    dev = torch.device("cuda:0")
    W, H, R, subme, level, gop = 512, 320, 12, 3, 2, 3
    qp = 30 + 12 * (depth == 10)
    clip = BE.occluded_clip(W, H, 7, depth, 71)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    w64, h64 = pics[0].w64, pics[0].h64
    srdo_p = sao_rdo_inputs(depth, qp, HT.SLICE_P)

    def p_step():
        return S.FramePipeline(w64, h64, depth, dev, rng=R, subme=subme, level=level, qp=qp, want_surf=False, deblock=True, sao=True, chroma=True,
                               sao_apply=True, sign_hide=True, sao_rdo=srdo_p)
    b_step = _b_step(w64, h64, depth, dev, R, subme, level, qp)
    order, out = S.MiniGop(p_step(), b_step, gop).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 3, 1, 2, 6, 4, 5] and sorted(out) == list(range(7))
    dt = pics[0].host.dtype
    got = {k: [p.cpu().numpy().view(dt).reshape(-1) for p in planes] for k, planes in out.items()}

    # the same in coding order on the CPU
    cores, avx2 = B.effective_cpus(), BE.O.host_has_avx2()
    nctu = (w64 // 64) * (h64 // 64)
    want = {0: [p.reshape(-1) for p in BE.padded_planes(clip[0])[0]]}
    dirs = set()
    for a in (3, 6):
        prev = want[a - gop]
        shape = pics[0].host.shape
        _, o = B.oracle_chain(F, clip, R, subme, level, qp, depth, nctu, cores, avx2, ref_planes=(prev[0].reshape(shape), prev[1], prev[2]), cur_index=a,
                              sao_rdo=srdo_p)
        want[a] = [o["recon"].reshape(-1), o["recon_c0"].reshape(-1), o["recon_c1"].reshape(-1)]
        for k in range(a - gop + 1, a):
            r0 = (prev[0].reshape(shape), prev[1], prev[2])
            r1 = (want[a][0].reshape(shape), want[a][1], want[a][2])
            ob = BE.b_chain(depth, BE.padded_planes(clip[k])[0], r0, r1, w64, h64, R, subme, level, qp, sao_rdo=b_step.sao_rdo, cores=cores, avx2=avx2)
            want[k] = [ob["recon"].reshape(-1), ob["recon_c0"].reshape(-1), ob["recon_c1"].reshape(-1)]
            dirs |= set(np.unique(ob["dir"]).tolist())
    for k in range(7):
        for name, g, e in zip(("Y", "Cb", "Cr"), got[k], want[k]):
            assert g.shape == e.shape and np.array_equal(g, e), f"picture {k} {name}: {int(np.count_nonzero(g != e))} of {e.size} samples differ"
    assert dirs == {1, 2, 3}

    # the P chain of the anchors alone
    alone = p_step()
    ref = pics[0]
    for a in (3, 6):
        alone.run(pics[a], ref)
        torch.cuda.synchronize()
        for g, e in zip(alone.final_planes(), out[a]):
            assert torch.equal(g.reshape(-1), e.reshape(-1)), f"anchor {a}: the P chain alone differs from the mini-GOP's anchor"
        ref = pics[a].like([p.clone() for p in alone.final_planes()])
