"""GPU: x265hip_subpel_refine_levels (a subset of the PU levels per launch) against the one-launch result of x265hip_subpel_refine, which
tests/test_gpu_subpel.py holds against the oracle - and the frame pipeline's default parallel schedule with three of the four levels
refined off the critical path against the same schedule with the single launch."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest

import subpel_cases as SC
import subpel_chroma_cases as CC
from step_chain import sao_rdo_inputs

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")

SENTINEL = -0x5a5a5a5b
LBASE = (0, 64, 80, 84, 85)
MASKS = [(0,), (1,), (2,), (3,), (0, 1, 3), (0, 1, 2, 3)]


def _level_of_record(nctu):
    lv = np.zeros(85, np.int64)
    for l in range(4):
        lv[LBASE[l]:LBASE[l + 1]] = l
    return np.tile(lv, nctu)


@functools.lru_cache(maxsize=None)
def _searched(depth, kind, chroma=False):
    """A 128 x 128 picture (2 x 2 CTUs: the CTU index moves in both directions) of clipping (`edges`) or noise content, searched over +-8 on
    the device: (cur, ref, MotionSearch) with the integer minima in place.  Shared between the cases: read only."""
    import torch
    dev = torch.device("cuda:0")
    if chroma:
        cc = CC.build(depth, 128, 128, 8, kind, 31)
        c = cc.luma
        (cur_cb, cur_cr), (ref_cb, ref_cr) = CC.chroma_pictures(cc)
        cur, ref = P.DevicePicture(c.cur_img, dev, cur_cb, cur_cr), P.DevicePicture(c.ref_img, dev, ref_cb, ref_cr)
    else:
        c = SC.build(depth, 128, 128, 8, kind, 31)
        cur, ref = P.DevicePicture(c.cur_img, dev), P.DevicePicture(c.ref_img, dev)
    ms = P.MotionSearch(cur.w64, cur.h64, 8, depth, dev, want_surf=False)
    ms.run(cur, ref)
    torch.cuda.synchronize()
    assert ms.nctu == 4
    return cur, ref, ms


def _check_masks(depth, kind, subme, planes, chroma):
    import torch
    cur, ref, ms = _searched(depth, kind, chroma)
    dev = cur.t.device
    sp = P.SubpelRefine(ms, subme, dev, phase_planes=planes, chroma_satd=chroma)
    sp.out.fill_(SENTINEL)
    sp.run(cur, ref)                                       # the existing one-launch entry
    torch.cuda.synchronize()
    want = sp.out.cpu().numpy().reshape(-1, 2).copy()
    assert not (want == SENTINEL).all(axis=1).any()
    frac = (want[:, 1] & 3) | ((want[:, 1] >> 16) & 3)
    assert np.count_nonzero(frac) > want.shape[0] // 10    # the refinement moves vectors off the integer grid
    lv = _level_of_record(ms.nctu)
    for levels in MASKS:
        sp.out.fill_(SENTINEL)
        sp.run(cur, ref, prepared=True, levels=levels)
        torch.cuda.synchronize()
        got = sp.out.cpu().numpy().reshape(-1, 2)
        sel = np.isin(lv, levels)
        bad = np.nonzero((got[sel] != want[sel]).any(axis=1))[0]
        assert bad.size == 0, f"levels {levels}: {bad.size} selected records differ from the one-launch result, first {np.nonzero(sel)[0][bad[:5]]}"
        assert (got[~sel] == SENTINEL).all(), f"levels {levels}: {np.count_nonzero((got[~sel] != SENTINEL).any(axis=1))} unselected records were written"
    # union: the level the reconstruction reads, then the other three into the same buffer (a mask instead of a list this time)
    sp.out.fill_(SENTINEL)
    sp.run(cur, ref, prepared=True, levels=1 << 2)
    sp.run(cur, ref, prepared=True, levels=0b1011)
    torch.cuda.synchronize()
    assert np.array_equal(sp.out.cpu().numpy().reshape(-1, 2), want), "level 2 then {0, 1, 3}: not the one-launch buffer"


@pytest.mark.parametrize("planes", [False, True], ids=["interp", "planes"])
@pytest.mark.parametrize("subme", [3, 5])
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("kind", ["edges", "noise"])
def test_selected_levels_equal_the_one_launch_records_and_nothing_else_is_written(kind, depth, subme, planes):
    """Each single level (its own kernel, grid (ctus, 1)), {0, 1, 3} (one launch of three grid rows through the level table) and all four
    through x265hip_subpel_refine_levels over a sentinel-filled `out`: the selected records bit for bit those of x265hip_subpel_refine,
    every other record still the sentinel; and level 2 followed by {0, 1, 3} rebuilds the whole buffer.  subme 3 / 5 = 4 / 8 directions;
    8- and 16-bit samples, candidates interpolated from LDS patches (dynamic LDS sized per mask) or read from the phase planes."""
    _check_masks(depth, kind, subme, planes, False)


def test_selected_levels_with_chroma_satd():
    """The chroma-SATD flavour (x265hip_subpel_chroma given, subme 3, 8 bits, phase planes): the same two checks."""
    _check_masks(8, "edges", 3, True, True)


def test_deferred_levels_leave_every_output_of_the_default_schedule(monkeypatch):
    """FramePipeline in its default parallel schedule with the SAO decision on, 256 x 128, three closed-loop steps with swap_output: with
    X265HIP_SUBPEL_DEFER=1 (level 2 in front of the reconstruction, levels 0 / 1 / 3 on the side stream) every array of bench.stage_outputs
    and the three reconstructed planes equal those of X265HIP_SUBPEL_DEFER=0 (one launch) after each step.  Three steps: the second and
    third run with swapped minima buffers, rewritten phase planes and an `out` that already holds the previous picture's records."""
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench as B
    dev = torch.device("cuda:0")
    depth, W, Hh, qp = 8, 256, 128, 30
    clip = F.synth_clip(W, Hh, 4, depth=depth, seed=71)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    pipes, refs = [], []
    for defer in ("0", "1"):
        monkeypatch.setenv("X265HIP_SUBPEL_DEFER", defer)      # read once, at construction
        pipes.append(S.FramePipeline(pics[0].w64, pics[0].h64, depth, dev, rng=12, subme=3, level=2, qp=qp, want_surf=False, lookahead=(W, Hh),
                                     deblock=True, sao=True, chroma=True, sao_apply=True, sign_hide=True, subpel_planes=True, parallel_planes=True,
                                     sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P)))
        refs.append(pics[0].like([p.clone() for p in pics[0].planes()]))
    monkeypatch.delenv("X265HIP_SUBPEL_DEFER")
    assert pipes[0].subpel_defer is None and pipes[1].subpel_defer is not None
    dt = pics[0].host.dtype
    for k in (1, 2, 3):
        outs = []
        for pipe, ref in zip(pipes, refs):
            pipe.sp.out.fill_(SENTINEL)                        # a record no launch of this step wrote would show
            rec = pipe.run(pics[k], ref)
            torch.cuda.synchronize()
            o = B.stage_outputs(pipe, dt)
            o["recon"] = rec.cpu().numpy().view(dt)
            outs.append(o)
            new = pipe.swap_output(ref.planes())
            assert new is not None
            ref.t, ref.c = new[0], list(new[1:3])
        assert not (outs[0]["subpel_mv"] == SENTINEL).all(axis=1).any()
        assert outs[0].keys() == outs[1].keys()
        for name in outs[0]:
            assert np.array_equal(outs[0][name], outs[1][name]), f"step {k}: {name} differs between the one-launch and the deferred schedule"
