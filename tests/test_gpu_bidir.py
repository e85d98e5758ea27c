"""GPU parity of x265hip_bidir_decide against the expectation assembled from the oracle (tests/bidir_expect.py): dir, ref0, ref1,
mv0_out, mv1_out and cost_out of every block, equal - all of it is integer arithmetic.  The kernel is fed the ORACLE's records of the two
refinements, so a difference here is the decision kernel's own."""
import functools
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import bipred_cases as BC

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

PREFILL = -0x5a5a5a5b           # what mv*_out hold before the launch: entries of other levels must keep it


@functools.lru_cache(maxsize=2)
def _six_stripe(depth, subme):
    return BE.SixStripe(depth, subme)


def _up(a, dev):
    import torch
    return torch.from_numpy(a if a.dtype != np.uint16 else a.view(np.int16)).to(dev)


def _run_kernel(depth, level, cur, refs, stride, org, w64, h64, recs, cq, qoff, dir_cost, use_planes, ref_ids=(0, 1)):
    """One x265hip_bidir_decide launch on padded host planes + host records; returns the outputs as host arrays."""
    import torch
    dev = torch.device("cuda:0")
    nctu = (w64 // 64) * (h64 // 64)
    nb = (64 >> (3 + level)) ** 2
    tc, t0, t1 = _up(cur, dev), _up(refs[0], dev), _up(refs[1], dev)
    planes = None
    if use_planes:
        nbytes = t0.numel() * t0.element_size()
        planes = [torch.empty(15 * nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        for t, pl in zip((t0, t1), planes):
            A.phase_planes(depth, t, 0, pl, stride, cur.shape[0])
    m0, m1 = (torch.from_numpy(np.ascontiguousarray(r, dtype=np.int32).reshape(-1)).to(dev) for r in recs)
    d = torch.zeros(nctu * nb, dtype=torch.uint8, device=dev)
    r0, r1 = torch.full((nctu * nb,), 77, dtype=torch.int8, device=dev), torch.full((nctu * nb,), 77, dtype=torch.int8, device=dev)
    o0 = torch.full((nctu * 85 * 2,), PREFILL, dtype=torch.int32, device=dev)
    o1 = torch.full((nctu * 85 * 2,), PREFILL, dtype=torch.int32, device=dev)
    co = torch.zeros(nctu * nb * 4, dtype=torch.int32, device=dev)
    A.bidir_decide(depth, w64, h64, level, tc, stride, t0, t1, stride, m0, m1, _up(cq, dev), qoff, dir_cost, d, o0, o1, ref0=r0, ref1=r1,
                   cost_out=co, ref_ids=ref_ids, fenc_off=org, fref_off=org, phase_planes=planes)
    torch.cuda.synchronize()
    assert torch.equal(m0.cpu(), torch.from_numpy(np.ascontiguousarray(recs[0], dtype=np.int32).reshape(-1)))       # inputs untouched
    return dict(dir=d.cpu().numpy(), ref0=r0.cpu().numpy(), ref1=r1.cpu().numpy(), mv0_out=o0.cpu().numpy().reshape(-1, 2),
                mv1_out=o1.cpu().numpy().reshape(-1, 2), cost=co.cpu().numpy().reshape(-1, 4))


def _assert_equal(got, e, level, nctu, what):
    for k in ("dir", "ref0", "ref1", "cost"):
        bad = np.nonzero((got[k] != e[k]).reshape(len(e["dir"]), -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} of {len(e['dir'])} blocks; first {bad[:4].tolist()}: device {got[k][bad[:4]].tolist()}, expected {e[k][bad[:4]].tolist()}"
    for k, lv in (("mv0_out", "mv0"), ("mv1_out", "mv1")):
        want = BE.full_mv_out(level, nctu, e[lv], PREFILL)
        bad = np.nonzero((got[k] != want).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} records; first {bad[:4].tolist()}: device {got[k][bad[:4]].tolist()}, expected {want[bad[:4]].tolist()}"


@pytest.mark.parametrize("use_planes", [False, True], ids=["interpolate", "phase_planes"])
@pytest.mark.parametrize("subme", [2, 3])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 10])
def test_bidir_decide_equals_the_expectation_on_the_six_stripe_picture(depth, level, subme, use_planes):
    """Every outcome of the decision occurs on this picture (tests/test_bidir_cpu.py checks the shares); entries of other levels in
    mv*_out stay as pre-filled."""
    c = _six_stripe(depth, subme)
    e = c.expect(level, ref_ids=(4, 9))
    got = _run_kernel(depth, level, c.cur, c.refs, c.stride, c.org, c.w64, c.h64, c.recs, c.cq, c.qoff, BE.DIR_COST, use_planes, ref_ids=(4, 9))
    _assert_equal(got, e, level, c.nctu, f"depth {depth} level {level} subme {subme}")
    assert all(e["masks"][k].any() for k in BE.OUTCOMES)


def test_bidir_decide_12bit():
    """x265hip_me_fullsearch, x265hip_subpel_refine and this entry take 12-bit planes (16-bit samples, depth 12 in the rounding and the
    clip); the records come from the oracle's 12-bit build."""
    c = BE.SixStripe(12, 3)
    assert int(c.cur.max()) > 1023
    for level in (0, 2):
        e = c.expect(level)
        got = _run_kernel(12, level, c.cur, c.refs, c.stride, c.org, c.w64, c.h64, c.recs, c.cq, c.qoff, BE.DIR_COST, False)
        _assert_equal(got, e, level, c.nctu, f"12-bit level {level}")
        assert set(np.unique(e["dir"])) == {1, 2, 3}


@pytest.mark.parametrize("dir_cost,only", [((0, 0, 10000), "uni"), ((10000, 10000, 0), "bi")])
def test_dir_cost_decides(dir_cost, only):
    """The list-selection costs matter: a prohibitive bidirectional cost leaves no dir 3, prohibitive uni-directional costs leave only
    dir 3 - in the expectation (not by construction of the test) and on the device.  10 000 is prohibitive where no block cost comes near
    it: the 8x8 and 16x16 blocks of the 8-bit picture.  A 32x32 block of stripe (e) gains more than 10 000 from the averaged prediction, so
    at level 2 the device is compared with the expectation without that claim."""
    c = _six_stripe(8, 3)
    for level in (0, 1, 2):
        e = c.expect(level, dir_cost=dir_cost)
        if level < 2 and only == "uni":
            assert not (e["dir"] == 3).any() and (e["dir"] == 1).any() and (e["dir"] == 2).any()
        elif level < 2:
            assert (e["dir"] == 3).all()
        got = _run_kernel(8, level, c.cur, c.refs, c.stride, c.org, c.w64, c.h64, c.recs, c.cq, c.qoff, dir_cost, level == 1)
        _assert_equal(got, e, level, c.nctu, f"dir_cost {dir_cost} level {level}")


@pytest.mark.parametrize("depth", [8, 10])
def test_bidir_decide_3840x2160(depth):
    """The geometry of the existing B-picture test (picture 1 of a 3840x2160 clip between pictures 0 and 2, range 12, subme 3, 32x32
    blocks): all 8160 blocks against the expectation, interpolating and reading phase planes."""
    B = importlib.import_module("bench")
    clip = F.synth_clip(3840, 2160, 3, depth=depth, seed=21)
    pl = [F.pad_plane(clip[i][0]) for i in (1, 0, 2)]
    cur, stride, org, w64, h64 = pl[0]
    refs = (pl[1][0], pl[2][0])
    nctu = (w64 // 64) * (h64 // 64)
    rng_r, level = 12, 2
    cost = F.mv_cost_table(rng_r)
    cq, qoff = F.qpel_cost_table(rng_r)
    cores = B.effective_cpus()
    recs, phases = [], []
    for ref in refs:
        _, best = BE.O.me_fullsearch(depth, cur, stride, org, ref, stride, org, w64, h64, rng_r, 0, nctu, cost, cost, want_surf=False, nthreads=cores)
        recs.append(BE.O.subpel_refine(depth, cur, stride, org, ref, stride, org, w64, h64, rng_r, 0, nctu, best, cq, qoff, 3, nthreads=cores))
        phases.append(BE.phases_of(depth, ref, stride))
    e = BE.expect(depth, cur, stride, org, w64, h64, level, recs, phases, cq, qoff)
    del phases
    # plain motion between its neighbours: most blocks average both lists, some keep one (every outcome is met on the six-stripe picture)
    assert len(e["dir"]) == 8160 and (e["dir"] == 3).any() and (e["dir"] != 3).any() and e["masks"]["dir3_refined"].any()
    for use_planes in (False, True):
        got = _run_kernel(depth, level, cur, refs, stride, org, w64, h64, recs, cq, qoff, BE.DIR_COST, use_planes)
        _assert_equal(got, e, level, nctu, f"4K depth {depth} planes {use_planes}")


@pytest.mark.parametrize("case,level,use_planes", BC.BIDIR_CASES, ids=lambda v: v.id if isinstance(v, BC.BiCase) else str(v))
def test_bidir_decide_on_clipping_content(case, level, use_planes):
    """Two `edges` references and a current picture planted for every outcome (tests/bipred_cases.py): both clips of the kernel's own
    interpolation, phase-plane reads at vectors up to 57 samples from the block, records with a zero cost key under non-zero vectors and
    full-amplitude differences at 12 bits.  tests/test_bipred_cases_cpu.py asserts that every outcome occurs on at least 3 % of the blocks."""
    c = BC.build_bi(*case.build)
    e = BC.decided(case, level)
    cq, qoff = F.qpel_cost_table(c.R)
    got = _run_kernel(c.depth, level, c.cur, c.refs, c.stride, c.org, c.w64, c.h64, BC.refined_bi(case), cq, qoff, BE.DIR_COST, use_planes)
    _assert_equal(got, e, level, c.nctu, f"{case.id} level {level} planes {use_planes}")
    assert all(e["masks"][k].any() for k in BE.OUTCOMES)
