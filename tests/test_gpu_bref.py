"""GPU parity of the B step with several references per list: x265hip_bidir_decide_refs against the expectation of tests/bref_expect.py
(the eight-stripe picture and a 2 x 2-CTU picture, both flavours, hand-made list indices), x265hip_inter_recon_bi_refs and the chroma
entry against the per-pair assembly of the oracle's bi-predictive stages (also past the persistent kernels' first pass),
stages.MultiRefBFramePipeline stage by stage against b_chain_refs, and stages.MiniGop with b_refs.  Every comparison is bit for bit;
output buffers start as sentinels."""
import functools
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import bref_expect as BR
import qp_map_expect as QE
from step_chain import sao_rdo_inputs
from test_gpu_tu_passes import _assert_plane, _dev_plane, _fill_outputs, _mvs, _nthreads, _passes, _phases, _picture, _sentinel

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")

PREFILL = -0x5a5a5a5b           # what mv*_out hold before the launch: entries of other levels must keep it
IDS = ((4, 9), (9, 2))          # picture ids: list 0's second picture is list 1's first


def _up(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


@functools.lru_cache(maxsize=None)
def _small(depth):
    """2 x 2 CTUs of the same eight stripes (16 samples each)"""
    return BR.Stripes(depth, 3, w=128, h=128, seed=53)


def _decide_on_device(case, level, refs0, refs1, mv0, mv1, idx0, idx1, cost0, cost1, ids0, ids1, use_planes, optional=True, dir_cost=BE.DIR_COST):
    """One x265hip_bidir_decide_refs launch on padded host planes + host records; returns the outputs as host arrays."""
    import torch
    dev = torch.device("cuda:0")
    nb = case.nctu * (64 >> (2 * level))
    tc = _up(case.cur, dev)
    uploaded = {}

    def plane(p):                       # one device copy (and one set of phase planes) per distinct host plane
        if id(p) not in uploaded:
            t = _up(p, dev)
            pl = None
            if use_planes:
                pl = torch.empty(15 * t.numel() * t.element_size(), dtype=torch.uint8, device=dev)
                A.phase_planes(case.depth, t, 0, pl, case.stride, case.cur.shape[0])
            uploaded[id(p)] = (t, pl)
        return uploaded[id(p)]
    l0, l1 = [plane(p) for p in refs0], [plane(p) for p in refs1]
    hm = [np.ascontiguousarray(m, np.int32).reshape(-1) for m in (mv0, mv1)]
    hi = [np.ascontiguousarray(i, np.int8) for i in (idx0, idx1)]
    m0, m1, i0, i1 = (torch.from_numpy(x).to(dev) for x in hm + hi)
    d = torch.full((nb,), 0x5a, dtype=torch.uint8, device=dev)
    r0, r1 = (torch.full((nb,), 77, dtype=torch.int8, device=dev) if optional else None for _ in range(2))
    o0, o1 = (torch.full((case.nctu * 85 * 2,), PREFILL, dtype=torch.int32, device=dev) for _ in range(2))
    co = torch.full((nb * 4,), PREFILL, dtype=torch.int32, device=dev) if optional else None
    A.bidir_decide_refs(case.depth, case.w64, case.h64, level, tc, case.stride, [t for t, _ in l0], [t for t, _ in l1], case.stride, m0, m1, i0, i1, cost0, cost1,
                        _up(case.cq, dev), case.qoff, dir_cost, d, o0, o1, ref0=r0, ref1=r1, cost_out=co, ref_ids0=ids0, ref_ids1=ids1, fenc_off=case.org,
                        fref_off=case.org, phase_planes0=[p for _, p in l0] if use_planes else None, phase_planes1=[p for _, p in l1] if use_planes else None)
    torch.cuda.synchronize()
    for t, h in zip((m0, m1, i0, i1), hm + hi):
        assert np.array_equal(t.cpu().numpy(), h), "an input changed"
    g = lambda t: None if t is None else t.cpu().numpy()
    return dict(dir=g(d), ref0=g(r0), ref1=g(r1), mv0_out=g(o0).reshape(-1, 2), mv1_out=g(o1).reshape(-1, 2), cost=None if co is None else g(co).reshape(-1, 4))


def _assert_decision(got, e, level, nctu, what):
    for k in ("dir", "ref0", "ref1", "cost"):
        if got[k] is None:
            continue
        bad = np.nonzero((got[k] != e[k]).reshape(len(e["dir"]), -1).any(axis=1))[0]
        assert bad.size == 0, (f"{what}: {k} differs on {bad.size} of {len(e['dir'])} blocks; first {bad[:4].tolist()}: device {got[k][bad[:4]].tolist()}, "
                               f"expected {e[k][bad[:4]].tolist()}")
    for k, lv in (("mv0_out", "mv0"), ("mv1_out", "mv1")):
        want = BE.full_mv_out(level, nctu, e[lv], PREFILL)          # entries of other levels still hold the pre-fill
        bad = np.nonzero((got[k] != want).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} records; first {bad[:4].tolist()}: device {got[k][bad[:4]].tolist()}, expected {want[bad[:4]].tolist()}"


def _decide_case(case, level, nrefs, cost, ids, use_planes, optional=True):
    (p0, _, _), (p1, _, _) = case.lists(nrefs)
    e = case.expect(level, nrefs=nrefs, ref_cost0=cost[0], ref_cost1=cost[1], ref_ids0=ids[0], ref_ids1=ids[1], with_reference=False)
    got = _decide_on_device(case, level, p0, p1, e["mv_in0"], e["mv_in1"], e["sel0"]["ref_idx"], e["sel1"]["ref_idx"], e["ref_cost"][0], e["ref_cost"][1],
                            ids[0], ids[1], use_planes, optional)
    return got, e


@pytest.mark.parametrize("use_planes", [False, True], ids=["interpolate", "phase_planes"])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 10])
def test_decision_equals_the_expectation_on_the_eight_stripe_picture(depth, level, use_planes):
    """Two references per list, picture ids (4, 9) / (9, 2), the default reference bits and COST_HEAVY: every outcome occurs on this picture
    (tests/test_bref_cpu.py asserts the shares) and the reference bits turn decisions."""
    case = BR.stripes(depth)
    what = f"depth {depth} level {level} planes {use_planes}"
    for cost in ((None, None), BR.COST_HEAVY):
        got, e = _decide_case(case, level, (2, 2), cost, IDS, use_planes)
        _assert_decision(got, e, level, case.nctu, f"{what} ref_cost {e['ref_cost']}")
        assert all(e["masks"][k].any() for k in BR.OUTCOMES), what
        assert set(np.unique(e["ref0"])) == {-1, 4, 9} and set(np.unique(e["ref1"])) == {-1, 9, 2}, what
    assert (e["dir"] != e["dir_rb0"]).any(), what


@pytest.mark.parametrize("nrefs", [(1, 1), (2, 1), (2, 2), (4, 3)])
@pytest.mark.parametrize("depth", [8, 10])
def test_decision_with_every_list_length_on_two_by_two_ctus(depth, nrefs):
    """128 x 128, levels 0 - 2, both flavours; lists longer than two repeat their pictures (the first copy wins).  At level 1 the optional
    outputs are left NULL."""
    case = _small(depth)
    ids = (tuple(range(10, 10 + nrefs[0])), tuple(range(20, 20 + nrefs[1])))
    for level in (0, 1, 2):
        for use_planes in (False, True):
            got, e = _decide_case(case, level, nrefs, (None, None), ids, use_planes, optional=level != 1)
            _assert_decision(got, e, level, case.nctu, f"depth {depth} nrefs {nrefs} level {level} planes {use_planes}")
            assert e["ref_cost"] == (A.b_ref_cost_bits(nrefs[0]), A.b_ref_cost_bits(nrefs[1])) and len(set(np.unique(e["dir"]))) >= 2


def test_decision_12bit():
    case = BR.Stripes(12, 3, w=256, h=128, seed=55)
    assert int(case.cur.max()) > 1023
    for use_planes in (False, True):
        got, e = _decide_case(case, 1, (2, 2), (None, None), IDS, use_planes)
        _assert_decision(got, e, 1, case.nctu, f"12-bit planes {use_planes}")
        assert set(np.unique(e["dir"])) == {1, 2, 3}


@pytest.mark.parametrize("use_planes", [False, True], ids=["interpolate", "phase_planes"])
@pytest.mark.parametrize("depth,level", [(8, 0), (10, 1), (8, 2)])
def test_decision_with_alternating_and_out_of_range_ref_idx(depth, level, use_planes):
    """Hand-made indices that change from block to block, independently per list, over four and three DISTINCT planes - at levels 0 and 1
    the lanes of one wavefront read different planes - with entries outside the lists (clamped).  The records are the selections' own."""
    case = BR.stripes(depth)
    a0, a1, b0, b1 = case.refs[0] + case.refs[1]
    pa0, pa1, pb0, pb1 = case.phases[0] + case.phases[1]
    l0, l1, ph0, ph1 = [a0, a1, b0, b1], [b1, a0, b0], [pa0, pa1, pb0, pb1], [pb1, pa0, pb0]
    sel = case.expect(level, with_reference=False)
    nb = len(sel["dir"])
    idx0 = (np.arange(nb) % 4).astype(np.int8)
    idx1 = ((np.arange(nb) // 3) % 3).astype(np.int8)
    idx0[5::16], idx0[9::16], idx1[2::8], idx1[7::8] = -3, 11, 3, -128
    cost0, cost1, ids0, ids1 = (8, 12, 16, 16), (40, 4, 20), (1, 2, 3, 4), (4, 1, 3)
    e = BR.decide(depth, case.cur, case.stride, case.org, case.w64, case.h64, level, sel["mv_in0"], sel["mv_in1"], idx0, idx1, ph0, ph1, cost0, cost1,
                  case.cq, case.qoff, ref_ids0=ids0, ref_ids1=ids1, with_reference=False)
    got = _decide_on_device(case, level, l0, l1, sel["mv_in0"], sel["mv_in1"], idx0, idx1, cost0, cost1, ids0, ids1, use_planes)
    _assert_decision(got, e, level, case.nctu, f"alternating ref_idx, depth {depth} level {level} planes {use_planes}")
    assert set(np.unique(e["dir"])) == {1, 2, 3} and set(np.unique(e["ref0"])) == {-1, 1, 2, 3, 4} and set(np.unique(e["ref1"])) == {-1, 4, 1, 3}


@pytest.mark.parametrize("depth", [8, 10])
def test_one_reference_per_list_with_zero_reference_bits_is_bidir_decide(depth):
    """The identity of the contract, device against device: x265hip_bidir_decide on the same picture and records."""
    import torch
    dev = torch.device("cuda:0")
    case = BR.stripes(depth)
    recs = [case.recs[0][0], case.recs[1][0]]
    nb0 = case.nctu * 85 * 2
    for level in (0, 1, 2):
        nb = case.nctu * (64 >> (2 * level))
        for use_planes in (False, True):
            zero = np.zeros(nb, np.int8)
            got = _decide_on_device(case, level, case.refs[0][:1], case.refs[1][:1], recs[0], recs[1], zero, zero, (0,), (0,), (4,), (9,), use_planes)
            tc, t0, t1 = _up(case.cur, dev), _up(case.refs[0][0], dev), _up(case.refs[1][0], dev)
            planes = None
            if use_planes:
                planes = [torch.empty(15 * t0.numel() * t0.element_size(), dtype=torch.uint8, device=dev) for _ in range(2)]
                for t, pl in zip((t0, t1), planes):
                    A.phase_planes(depth, t, 0, pl, case.stride, case.cur.shape[0])
            d = torch.zeros(nb, dtype=torch.uint8, device=dev)
            r0, r1 = (torch.full((nb,), 77, dtype=torch.int8, device=dev) for _ in range(2))
            o0, o1 = (torch.full((nb0,), PREFILL, dtype=torch.int32, device=dev) for _ in range(2))
            co = torch.zeros(nb * 4, dtype=torch.int32, device=dev)
            A.bidir_decide(depth, case.w64, case.h64, level, tc, case.stride, t0, t1, case.stride, _up(recs[0].reshape(-1), dev), _up(recs[1].reshape(-1), dev),
                           _up(case.cq, dev), case.qoff, BE.DIR_COST, d, o0, o1, ref0=r0, ref1=r1, cost_out=co, ref_ids=(4, 9), fenc_off=case.org,
                           fref_off=case.org, phase_planes=planes)
            torch.cuda.synchronize()
            twin = dict(dir=d, ref0=r0, ref1=r1, mv0_out=o0, mv1_out=o1, cost=co)
            for k, t in twin.items():
                assert np.array_equal(got[k].reshape(-1), t.cpu().numpy().reshape(-1)), f"depth {depth} level {level} planes {use_planes}: {k} differs from bidir_decide"
            assert set(np.unique(got["dir"])) == {1, 2, 3}


# ---- the TU entries ---------------------------------------------------------------------------------------------------------------
def _assert_outputs(st, elev, ens, edist, what):
    assert np.array_equal(st.levels.cpu().numpy(), elev), f"{what}: levels differ"
    assert np.array_equal(st.num_sig.cpu().numpy().view(np.uint32), ens), f"{what}: numSig differs"
    assert np.array_equal(st.dist.cpu().numpy().view(np.uint64), edist), f"{what}: SSE differs"
    assert (ens > 1).any() and np.count_nonzero(elev) > 500, f"{what}: a degenerate case ({np.count_nonzero(elev)} levels)"


def _tu_inputs(rng, nctu, nb, nrefs, all_pairs=True):
    """records of every phase for both lists, dir mixed 1 / 2 / 3 from block to block, indices alternating independently per list (every
    pair of indices meets every dir) - and a sentinel (90, far outside every list) in the index of the list a block does not use"""
    mv0, mv1 = _mvs(rng, nctu), _mvs(rng, nctu)
    dirs = ((np.arange(nb) + np.arange(nb) // (nrefs[0] * nrefs[1])) % 3 + 1).astype(np.uint8)
    idx0 = (np.arange(nb) % nrefs[0]).astype(np.int8)
    idx1 = ((np.arange(nb) // nrefs[0] + 1) % nrefs[1]).astype(np.int8)
    dev0, dev1 = idx0.copy(), idx1.copy()
    dev0[dirs == 2], dev1[dirs == 1] = 90, 90
    assert set(np.unique(dirs)) == {1, 2, 3}
    assert not all_pairs or len({(int(a), int(b)) for a, b in zip(idx0[dirs == 3], idx1[dirs == 3])}) == nrefs[0] * nrefs[1]
    return mv0, mv1, dirs, idx0, idx1, dev0, dev1


def _luma_vs_assembly(depth, level, w, h, seed, nrefs, inputs, qp, flags, what, qp_cells=None):
    import torch
    dev = torch.device("cuda:0")
    mv0, mv1, dirs, idx0, idx1, dev0, dev1 = inputs
    nctu = (w // 64) * (h // 64)
    n = 1 + nrefs[0] + nrefs[1]
    clip = F.synth_clip(w, h, n, depth=depth, seed=seed)
    pads = [F.pad_plane(clip[k][0]) for k in range(n)]
    stride, org = pads[0][1], pads[0][2]
    pics = [P.DevicePicture(clip[k][0], dev) for k in range(n)]
    assert np.array_equal(pics[0].host, pads[0][0]), "DevicePicture pads like frames.pad_plane"
    r0, r1 = list(range(1, 1 + nrefs[0])), list(range(1 + nrefs[0], n))
    st = S.InterReconBiRefs(nctu, w, h, depth, level, qp, dev, intra_slice=flags)
    _fill_outputs(st)
    if qp_cells is not None:
        st.qp_map = _up(np.asarray(qp_cells, np.int8).reshape(-1), dev)
    recon = torch.full_like(pics[0].t, _sentinel(depth))
    st.run(pics[0], [pics[k] for k in r0], [pics[k] for k in r1], recon, _up(mv0.reshape(-1), dev), _up(mv1.reshape(-1), dev), _up(dev0, dev), _up(dev1, dev),
           dir_flags=_up(dirs, dev))
    torch.cuda.synchronize()
    erec, elev, ens, edist = BR.recon_luma(depth, pads[0][0], [pads[k][0] for k in r0], [pads[k][0] for k in r1], stride, org, w, h, level, mv0, mv1, idx0, idx1,
                                           dirs, qp, flags, qp_cells, _nthreads())
    _assert_outputs(st, elev, ens, edist, what)
    _assert_plane(recon.cpu().numpy().view(pads[0][0].dtype), erec, stride, org, w, h, _sentinel(depth), what)


def _chroma_vs_assembly(depth, level, w, h, seed, nrefs, inputs, qps, flags, what, qp_cells=None):
    import torch
    dev = torch.device("cuda:0")
    mv0, mv1, dirs, idx0, idx1, dev0, dev1 = inputs
    nctu = (w // 64) * (h // 64)
    n = 1 + nrefs[0] + nrefs[1]
    clip = F.synth_clip(w, h, n, depth=depth, seed=seed)
    pads = [[F.pad_chroma(clip[k][c], w, h) for c in (1, 2)] for k in range(n)]
    stride, org = pads[0][0][1], pads[0][0][2]
    r0, r1 = list(range(1, 1 + nrefs[0])), list(range(1 + nrefs[0], n))
    d = [_up(x.reshape(-1), dev) for x in (mv0, mv1)] + [_up(x, dev) for x in (dev0, dev1, dirs)]
    for c in range(2):
        planes = [pads[k][c][0] for k in range(n)]
        dp = [_dev_plane(p, dev) for p in planes]
        st = S.InterReconChromaBiRefs(nctu, w, h, depth, level, qps[c], dev, intra_slice=flags)
        _fill_outputs(st)
        if qp_cells is not None:
            st.qp_map = _up(np.asarray(qp_cells[c], np.int8).reshape(-1), dev)
        recon = torch.full_like(dp[0], _sentinel(depth))
        st.run(dp[0], [dp[k] for k in r0], [dp[k] for k in r1], recon, stride, org, d[0], d[1], d[2], d[3], dir_flags=d[4])
        torch.cuda.synchronize()
        erec, elev, ens, edist = BR.recon_chroma(depth, planes[0], [planes[k] for k in r0], [planes[k] for k in r1], stride, org, w, h, level, mv0, mv1, idx0, idx1,
                                                 dirs, qps[c], flags, None if qp_cells is None else qp_cells[c], _nthreads())
        _assert_outputs(st, elev, ens, edist, f"plane {c}, {what}")
        _assert_plane(recon.cpu().numpy().view(planes[0].dtype), erec, stride, org, w // 2, h // 2, _sentinel(depth), f"plane {c}, {what}")


@pytest.mark.parametrize("depth,level,flags", [(8, 0, 2), (8, 1, 0), (8, 2, 2), (10, 0, 0), (10, 1, 2), (10, 2, 0)])
def test_tu_entries_equal_the_per_pair_assembly(depth, level, flags):
    """256 x 128, three references in list 0 and two in list 1, every pair of indices on bidirectional blocks, the next block's plane
    different for each list, vectors of every phase, a sentinel in the unused list's index.  flags 2: sign hiding."""
    w, h, nrefs = 256, 128, (3, 2)
    nctu = (w // 64) * (h // 64)
    nb = nctu * (64 >> (2 * level))
    inputs = _tu_inputs(np.random.default_rng([61, depth, level]), nctu, nb, nrefs)
    if level < 2:
        assert len(_phases(inputs[0], nctu, level, 3)) == 16 and len(_phases(inputs[1], nctu, level, 3)) == 16
    qp = 26 + 6 * (depth - 8)
    what = f"{depth}-bit level {level} flags {flags}"
    _luma_vs_assembly(depth, level, w, h, 610 + depth, nrefs, inputs, qp, flags, what)
    _chroma_vs_assembly(depth, level, w, h, 620 + depth, nrefs, inputs, (qp - 5, qp - 8), flags, what)


@pytest.mark.parametrize("depth,level", [(8, 2), (10, 1)])
def test_tu_entries_with_a_qp_map(depth, level):
    w, h, nrefs = 256, 128, (2, 2)
    nctu = (w // 64) * (h // 64)
    nb = nctu * (64 >> (2 * level))
    rng = np.random.default_rng([63, depth, level])
    inputs = _tu_inputs(rng, nctu, nb, nrefs)
    vals = QE.map_values(depth)[2:6]
    cells = [QE.cells_of_blocks(rng.choice(vals, size=nb), w, h, level) for _ in range(3)]
    assert len(np.unique(QE.blocks_of_cells(cells[0], w, h, level))) >= 3
    what = f"{depth}-bit level {level} with a qp_map"
    _luma_vs_assembly(depth, level, w, h, 630 + depth, nrefs, inputs, 30, 2, what, cells[0])
    _chroma_vs_assembly(depth, level, w, h, 640 + depth, nrefs, inputs, (30, 30), 2, what, cells[1:])


@pytest.mark.parametrize("depth,level", [(8, 1), (10, 2), (8, 2)])
def test_inter_recon_bi_refs_multi_pass(depth, level):
    """The persistent 16 / 32-point luma instances past their first resident pass."""
    n = 8 << level
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_BI_REFS, n, depth, False, (64 // n) ** 2)
    what = f"bi refs luma {n}x{n} {depth}-bit: " + _passes(nb, g, tail=level == 2)
    inputs = _tu_inputs(np.random.default_rng([65, depth, level]), (w // 64) * (h // 64), nb, (2, 2))
    _luma_vs_assembly(depth, level, w, h, 650 + level, (2, 2), inputs, 30 + 6 * (depth - 8), 2, what)


@pytest.mark.parametrize("depth", [8, 10])
def test_inter_recon_chroma_bi_refs_multi_pass(depth):
    """The persistent 16-point chroma instance past its first pass."""
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_CHROMA_BI_REFS, 16, depth, False, 4)
    what = f"bi refs chroma 16x16 {depth}-bit: " + _passes(nb, g, tail=True)
    inputs = _tu_inputs(np.random.default_rng([67, depth]), (w // 64) * (h // 64), nb, (2, 2))
    _chroma_vs_assembly(depth, 2, w, h, 670 + depth, (2, 2), inputs, (32, 29), 2, what)


@pytest.mark.parametrize("depth,level", [(8, 0), (10, 1), (8, 2)])
def test_copies_of_one_plane_in_every_slot_are_inter_recon_bi(depth, level):
    """Device against device: every slot of list l holds list l's one picture - x265hip_inter_recon_bi / _chroma_bi on the same inputs."""
    import torch
    dev = torch.device("cuda:0")
    w, h = 256, 128
    nctu = (w // 64) * (h // 64)
    nb = nctu * (64 >> (2 * level))
    mv0, mv1, dirs, _, _, dev0, dev1 = _tu_inputs(np.random.default_rng([69, depth, level]), nctu, nb, (4, 3), all_pairs=False)
    clip = F.synth_clip(w, h, 3, depth=depth, seed=690 + depth)
    pics = [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]
    d = [_up(x.reshape(-1), dev) for x in (mv0, mv1)] + [_up(x, dev) for x in (dev0, dev1, dirs)]
    qp = 28 + 6 * (depth - 8)
    a, b = S.InterReconBiRefs(nctu, w, h, depth, level, qp, dev, intra_slice=2), S.InterReconBi(nctu, w, h, depth, level, qp, dev, intra_slice=2)
    ra, rb = torch.full_like(pics[0].t, _sentinel(depth)), torch.full_like(pics[0].t, _sentinel(depth))
    _fill_outputs(a)
    a.run(pics[1], [pics[0]] * 4, [pics[2]] * 3, ra, d[0], d[1], d[2], d[3], dir_flags=d[4])
    b.run(pics[1], pics[0], pics[2], rb, d[0], d[1], dir_flags=d[4])
    ca, cb = (cls(nctu, w, h, depth, level, qp - 6, dev, intra_slice=2) for cls in (S.InterReconChromaBiRefs, S.InterReconChromaBi))
    rca, rcb = torch.full_like(pics[1].c[0], _sentinel(depth)), torch.full_like(pics[1].c[0], _sentinel(depth))
    _fill_outputs(ca)
    ca.run(pics[1].c[0], [pics[0].c[0]] * 4, [pics[2].c[0]] * 3, rca, pics[1].stride_c, pics[1].org_c, d[0], d[1], d[2], d[3], dir_flags=d[4])
    cb.run(pics[1].c[0], pics[0].c[0], pics[2].c[0], rcb, pics[1].stride_c, pics[1].org_c, d[0], d[1], dir_flags=d[4])
    torch.cuda.synchronize()
    for x, y, name in ((a, b, "luma"), (ca, cb, "Cb")):
        assert torch.equal(x.levels, y.levels) and torch.equal(x.num_sig, y.num_sig) and torch.equal(x.dist, y.dist), name
        assert int(x.num_sig.sum()) > 0
    assert torch.equal(ra, rb) and torch.equal(rca, rcb)


# ---- the step and the mini-GOP ---------------------------------------------------------------------------------------------------
W, H, R = 256, 192, 12


def _step(depth, dev, qp, max_refs=(2, 2), level=2, sao=True, **kw):
    return S.MultiRefBFramePipeline(W, H, depth, dev, max_refs=max_refs, rng=R, subme=3, level=level, qp=qp, deblock=True, sao=sao, chroma=True, sao_apply=sao,
                                    sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_B) if sao else None, want_cost=True, **kw)


def _pics(clip, dev):
    return [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]


@pytest.mark.parametrize("depth,level,subpel_planes", [(8, 2, False), (10, 2, True), (8, 1, True)])
def test_step_every_stage_equals_the_oracle_chain(depth, level, subpel_planes):
    """MultiRefBFramePipeline.run at 256x192 with lists (2, 2) in HEVC's default order - picture 2 from [1, 0] and [3, 1]: picture 1 sits in
    both lists and is searched once - chroma, deblocking on picture ids, SAO with the rate-distortion decision, sign hiding."""
    import torch
    dev = torch.device("cuda:0")
    qp = 30 + 12 * (depth == 10)
    clip = BE.occluded_clip(W, H, 5, depth, 91)
    pics = _pics(clip, dev)
    pipe = _step(depth, dev, qp, level=level, subpel_planes=subpel_planes)
    marks = []
    pipe.run(pics[2], [pics[1], pics[0]], [pics[3], pics[1]], mark=marks.append)
    torch.cuda.synchronize()
    assert marks == [m % r for r in range(3) for m in ("me%d", "subpel%d")] + ["ref_select", "bidir", "recon", "recon_chroma", "deblock", "sao_stats", "sao_rdo",
                                                                                "sao_apply", "border"]
    assert pipe.slots == ([0, 1], [2, 0])
    hp = [BE.padded_planes(c)[0] for c in clip]
    cpu = BR.b_chain_refs(depth, hp[2], [hp[1], hp[0]], [hp[3], hp[1]], W, H, R, 3, level, qp, sao_rdo=pipe.sao_rdo, cores=_nthreads())
    bad = BE.compare(BR.device_outputs(pipe, pics[0].host.dtype, 3), cpu)
    assert not bad, bad
    assert set(np.unique(cpu["dir"])) == {1, 2, 3} and len(np.unique(cpu["ref_idx0"])) == 2 and len(np.unique(cpu["ref_idx1"])) == 2
    # picture 1 (id 0) is used through both lists
    assert (cpu["ref0"] == 0).any() and (cpu["ref1"] == 0).any()
    assert int(cpu["num_sig"].sum()) > 0 and (cpu["bs_ver"] > 0).any() and (cpu["bs_hor"] > 0).any()
    assert [p.shape for p in pipe.final_planes()] == [p.shape for p in pics[2].planes()]


@pytest.mark.parametrize("depth", [8, 10])
def test_one_reference_per_list_with_zero_reference_bits_is_the_b_step(depth):
    import torch
    from test_gpu_bpicture import _b_step
    dev = torch.device("cuda:0")
    qp = 30 + 12 * (depth == 10)
    pics = _pics(BE.occluded_clip(W, H, 3, depth, 93), dev)
    bp = _b_step(W, H, depth, dev, R, 3, 2, qp)
    bp.run(pics[1], pics[0], pics[2])
    pipe = _step(depth, dev, qp, max_refs=(1, 1), ref_cost=((0,), (0,)))
    pipe.run(pics[1], [pics[0]], [pics[2]])
    torch.cuda.synchronize()
    for g, e in zip(pipe.final_planes(), bp.final_planes()):
        assert torch.equal(g, e), "one reference per list: not the B step's picture"
    for k in ("dir", "ref0", "ref1", "mv0_out", "mv1_out", "cost_out"):
        assert torch.equal(getattr(pipe.bd, k), getattr(bp.bd, k)), k
    assert torch.equal(pipe.rc.levels, bp.rc.levels) and int(pipe.rc.num_sig.sum()) > 0 and set(np.unique(pipe.bd.dir.cpu().numpy())) == {1, 2, 3}


def test_a_shared_picture_object_equals_cloned_pictures():
    """The search-once path: the same DevicePicture in both lists against a clone of it in list 1, with the ids a caller would give the
    clone (equal for the same picture).  Every stage output and the final planes are equal; the shared run searches three pictures."""
    import torch
    dev = torch.device("cuda:0")
    depth, qp = 8, 30
    clip = BE.occluded_clip(W, H, 5, depth, 95)
    pics = _pics(clip, dev)
    twin = P.DevicePicture(clip[1][0], dev, clip[1][1], clip[1][2])
    outs, marks = [], []
    for l1, ids in (([pics[3], pics[1]], None), ([pics[3], twin], ((0, 1), (2, 0)))):
        pipe = _step(depth, dev, qp, sao=False)
        m = []
        pipe.run(pics[2], [pics[1], pics[0]], l1, mark=m.append, ref_ids=ids)
        torch.cuda.synchronize()
        marks.append(m)
        bd = pipe.bd
        outs.append([t.clone() for t in (pipe.rs[0].ref_idx, pipe.rs[1].ref_idx, bd.dir, bd.ref0, bd.ref1, bd.mv0_out, bd.mv1_out, pipe.rc.levels, pipe.db.bs_ver,
                                         pipe.db.bs_hor, *pipe.final_planes())])
    assert sum(x.startswith("me") for x in marks[0]) == 3 and sum(x.startswith("me") for x in marks[1]) == 4
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][3] == 0).any() and (outs[0][4] == 0).any()


def test_step_with_qp_maps():
    import torch
    dev = torch.device("cuda:0")
    depth, qp, level = 8, 30, 2
    clip = [tuple(p) for p in QE.varied_clip(BE.occluded_clip(W, H, 5, depth, 97), depth)]
    pics = _pics(clip, dev)
    l0, l1 = [pics[1], pics[0]], [pics[3], pics[1]]
    pipe = _step(depth, dev, qp, sao=False)
    pipe.run(pics[2], l0, l1)
    torch.cuda.synchronize()
    uniform = pipe.checksum()
    aq = S.AdaptiveQuant(W, H, depth, dev, qg_size=16, aq_mode=2, aq_strength=1.0)
    offs, _, _, _ = aq.run(pics[2], cb=pics[2].c[0], cr=pics[2].c[1], stride_c=pics[2].stride_c, org_c=pics[2].org_c)
    maps = S.CuQpMaps(W, H, depth, level, dev, qg_size=16).run(qp + 0.3, offs)
    assert len(np.unique(maps.cu_qp_host)) >= 3
    pipe.set_qp_maps(maps)
    pipe.run(pics[2], l0, l1)
    torch.cuda.synchronize()
    assert pipe.checksum() != uniform
    hp = [BE.padded_planes(c)[0] for c in clip]
    cpu = BR.b_chain_refs(depth, hp[2], [hp[1], hp[0]], [hp[3], hp[1]], W, H, R, 3, level, qp, cu_qp=maps.cu_qp_host, tu_qp=maps.tu_qp_host, sao=False,
                          cores=_nthreads())
    bad = BE.compare(BR.device_outputs(pipe, pics[0].host.dtype, 3), cpu)
    assert not bad, bad
    pipe.set_qp_maps(None)
    pipe.run(pics[2], l0, l1)
    torch.cuda.synchronize()
    assert pipe.checksum() == uniform


def test_step_refuses_chroma_satd_and_bad_lists():
    import torch
    dev = torch.device("cuda:0")
    with pytest.raises(ValueError):
        S.MultiRefBFramePipeline(W, H, 8, dev, chroma=True, chroma_satd=True)
    pipe = S.MultiRefBFramePipeline(W, H, 8, dev, max_refs=(2, 1), rng=R)
    pics = _pics(BE.occluded_clip(W, H, 3, 8, 99), dev)
    with pytest.raises(ValueError):
        pipe.run(pics[1], [pics[0]], [pics[2], pics[0]])
    with pytest.raises(ValueError):
        pipe.run(pics[1], [pics[0], pics[2]], [pics[2]], ref_ids=((1, 2), (3,)))          # one picture with two ids


def test_mini_gop_with_three_p_and_three_two_b_references():
    """MiniGop(p_refs=3, b_refs=(3, 2)), gop 2, 7 pictures: every B picture equals b_chain_refs fed list 0 = the coded anchors before it,
    newest first, and list 1 = the later anchor + the one before; the anchors equal those of the same mini-GOP with b_refs=(1, 1) - B
    pictures change nothing an anchor sees - and b_refs=(1, 1) is today's driver."""
    import torch
    from test_gpu_bpicture import _b_step
    from test_gpu_multiref import _step as _p_step
    dev = torch.device("cuda:0")
    depth, qp, gop = 8, 30, 2
    clip = BE.occluded_clip(W, H, 7, depth, 89)
    pics = _pics(clip, dev)
    p_step = _p_step(depth, dev, qp, max_refs=3)
    b_step = _step(depth, dev, qp, max_refs=(3, 2))
    order, out = S.MiniGop(p_step, b_step, gop, p_refs=3, b_refs=(3, 2)).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3, 6, 5] and sorted(out) == list(range(7))
    today_b = _b_step(W, H, depth, dev, R, 3, 2, qp)
    o1, out1 = S.MiniGop(p_step, today_b, gop, p_refs=3).run(pics)
    o2, out2 = S.MiniGop(p_step, today_b, gop, p_refs=3, b_refs=(1, 1)).run(pics)
    torch.cuda.synchronize()
    assert o1 == o2 == order
    for k in out1:
        for g, e in zip(out2[k], out1[k]):
            assert torch.equal(g, e), f"picture {k}: b_refs=(1, 1) is not today's mini-GOP"
    for a in (0, 2, 4, 6):
        for g, e in zip(out[a], out1[a]):
            assert torch.equal(g, e), f"anchor {a} changed with the B pictures' references"
    dt, shape = pics[0].host.dtype, pics[0].host.shape
    host = lambda k: tuple(p.cpu().numpy().view(dt).reshape(shape if i == 0 else -1) for i, p in enumerate(out[k]))
    anchors = {a: host(a) for a in (0, 2, 4, 6)}          # one triple per coded anchor: a picture in both lists is the same object
    used0, used1 = set(), set()
    for k in (1, 3, 5):
        before = [anchors[a] for a in range(k - 1, -1, -gop)]
        l0, l1 = before[:3], ([anchors[k + 1]] + before)[:2]
        o = BR.b_chain_refs(depth, BE.padded_planes(clip[k])[0], l0, l1, W, H, R, 3, 2, qp, sao_rdo=b_step.sao_rdo, cores=_nthreads())
        used0 |= set(np.unique(o["ref_idx0"]).tolist())
        used1 |= set(np.unique(o["ref_idx1"]).tolist())
        for name, g, e in zip(("Y", "Cb", "Cr"), out[k], (o["recon"], o["recon_c0"], o["recon_c1"])):
            g, e = g.cpu().numpy().view(dt).reshape(-1), e.reshape(-1)
            assert np.array_equal(g, e), f"B picture {k} {name}: {int(np.count_nonzero(g != e))} of {e.size} samples differ"
    assert len(used0) >= 2 and len(used1) >= 2, (used0, used1)
