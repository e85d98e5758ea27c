"""GPU parity: sub-pel refinement stage (x265hip_subpel_refine) vs the oracle's restatement of
motion.cpp:1448-1664 driven through the oracle's luma_hpp/vpp/hvpp + sad/satd primitives."""
import importlib
import os
import sys

import numpy as np
import pytest

import subpel_cases as SC

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("depth,subme", [(8, 2), (8, 0), (8, 1), (8, 3), (8, 5), (8, 7), (10, 2), (10, 7), (12, 3)])
def test_subpel_refine_matches_oracle(depth, subme, planes):
    """planes: the candidates are read from the reference picture's phase planes (x265hip_phase_planes) instead of being interpolated
    per candidate tile - the same decisions either way."""
    _check_subpel(256, 128, depth, subme, planes, seed=40 + subme)


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("width,height,depth,subme", [(384, 320, 8, 2), (576, 448, 8, 3), (576, 448, 10, 2)])
def test_subpel_refine_xcd_ctu_order_matches_oracle(width, height, depth, subme, planes):
    """The kernel takes CTU xcd_swizzle(blockIdx.x, gridDim.x): with 8 CTUs that is the identity map.  30 CTUs (6 x 5) and 63 CTUs (9 x 7):
    each XCD gets a contiguous run of CTUs, and the last 6 / 7 CTUs form the tail past the last multiple of 8."""
    nctu = (width // 64) * (height // 64)
    assert nctu % 8 != 0 and nctu // 8 > 1, nctu
    _check_subpel(width, height, depth, subme, planes, seed=90 + nctu + depth)


def _check_subpel(width, height, depth, subme, planes, seed):
    import torch
    dev = torch.device("cuda:0")
    # sub-pel motion: frame 1 is frame 0 shifted by a non-integer amount (bilinear mix) plus noise
    rng = np.random.default_rng([41, depth, subme])
    clip = F.synth_clip(width, height, 2, depth=depth, seed=seed)
    y0 = clip[0][0].astype(np.float32)
    sh = np.roll(y0, (1, 2), axis=(0, 1))
    y1 = np.clip(np.rint(0.6 * y0 + 0.4 * sh + rng.normal(0, 1.0, size=y0.shape)), 0, (1 << depth) - 1).astype(clip[0][0].dtype)
    cur, ref = P.DevicePicture(y1, dev), P.DevicePicture(clip[0][0], dev)
    ms = P.MotionSearch(cur.w64, cur.h64, 8, depth, dev, want_surf=False)
    ms.run(cur, ref)
    sp = P.SubpelRefine(ms, subme, dev, phase_planes=planes)
    sp.run(cur, ref)
    torch.cuda.synchronize()
    O = _oracle()
    best = ms.best.cpu().numpy().view(np.uint64)
    exp = O.subpel_refine(depth, cur.host, cur.stride, cur.org, ref.host, ref.stride, ref.org, cur.w64, cur.h64, 8,
                          0, ms.nctu, best, sp.cost_q_host, sp.qoff, subme)
    got = sp.out.cpu().numpy().reshape(-1, 2)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {got.shape[0]} PUs differ, first {bad[:5]}: {got[bad[:3]]} vs {exp[bad[:3]]}"
    # the refinement must actually move some vectors off the integer grid
    frac = (exp[:, 1] & 3) | ((exp[:, 1] >> 16) & 3)
    assert np.count_nonzero(frac) > exp.shape[0] // 10


# ---------------------------------------------------------------------------------------------------------------------------------
# Hostile content with records written by the test (tests/subpel_cases.py; what every case reaches is asserted, with the oracle alone,
# in tests/test_subpel_cases_cpu.py): clipped samples, zero-cost keys, vectors anywhere in a +-57 window.
SENTINEL = -0x5a5a5a5b


def _refine_on_device(case, planes, wide_fenc=False):
    """x265hip_subpel_refine on a builder case, the records uploaded into a MotionSearch's `best` (no search runs).  wide_fenc: the current
    picture sits in a buffer 64 samples wider than the reference's, at another origin - hipabi.subpel_refine with its own fenc_stride / fenc_off."""
    import torch
    A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
    dev = torch.device("cuda:0")
    c = SC.build(*case.build)
    cur, ref = P.DevicePicture(c.cur_img, dev), P.DevicePicture(c.ref_img, dev)
    assert (cur.stride, cur.org) == (c.stride, c.org) and np.array_equal(cur.host, c.cur) and np.array_equal(ref.host, c.ref)
    ms = P.MotionSearch(c.w64, c.h64, c.R, c.depth, dev, want_surf=False)
    ms.best.copy_(torch.from_numpy(c.best.view(np.int64).copy()))
    sp = P.SubpelRefine(ms, case.subme, dev, phase_planes=planes)
    sp.out.fill_(SENTINEL)
    if not wide_fenc:
        sp.run(cur, ref)
    else:
        rows, stride = c.cur.shape[0] + 5, c.stride + 64
        org = 3 * stride + 40 + c.org // c.stride * stride + c.org % c.stride          # the padded plane's corner at row 3, column 40
        wide = np.full((rows, stride), (1 << c.depth) - 1 if c.depth > 8 else 0x5a, c.cur.dtype)
        wide[3:3 + c.cur.shape[0], 40:40 + c.stride] = c.cur
        wide_t = torch.from_numpy(wide if c.depth == 8 else wide.view(np.int16)).to(dev)
        sp.prepare(ref)
        A.subpel_refine(c.depth, c.w64, c.h64, c.R, case.subme, wide_t, stride, ref.t, ref.stride, ms.best, sp.cost_q, sp.qoff, sp.out,
                        fenc_off=org, fref_off=ref.org, phase_planes=sp.planes)
    torch.cuda.synchronize()
    return sp.out.cpu().numpy().reshape(-1, 2)


def _assert_records(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.shape[0]} PUs differ, first {bad[:5]} (ctu {bad[:5] // 85}, record {bad[:5] % 85}): "
                           f"{got[bad[:3]].tolist()} vs {exp[bad[:3]].tolist()}")


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("case", SC.SUBPEL_CASES, ids=lambda c: c.id)
def test_subpel_refine_hostile_content_matches_oracle(case, planes):
    """Every one of the nctu * 85 records, bit for bit, over a sentinel-filled output: `edges` / `noise` / `inverse` pictures clip the h, v and
    hv filters at both ends, three keys in ten cost zero (the shortcut, at every level), the vectors fill a +-57 (13, 8) window up to its
    edge, `inverse` at 12 bits feeds the packed Hadamard differences of full amplitude, the flat pairs leave the decision to the mv cost."""
    _assert_records(_refine_on_device(case, planes), SC.refined(case), case.id)


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("case", SC.STRIDE_CASES, ids=lambda c: c.id)
def test_subpel_refine_with_a_source_stride_of_its_own(case, planes):
    """fenc_stride != fref_stride: DevicePicture gives both planes one stride, so a mix-up of the two would otherwise go unseen."""
    _assert_records(_refine_on_device(case, planes, wide_fenc=True), SC.refined(case), case.id)
