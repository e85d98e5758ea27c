"""GPU parity of the P step with several references: x265hip_ref_select against the expectation of tests/multiref_expect.py on the
six-stripe picture, x265hip_inter_recon_refs and the chroma entries against the per-block assembly of the oracle's single-reference
stages (also past the persistent kernels' first pass), stages.MultiRefFramePipeline stage by stage against p_chain_refs, and
stages.MiniGop with p_refs.  Every comparison is bit for bit; output buffers start as sentinels."""
import importlib

import numpy as np
import pytest

import bidir_expect as BE
import multiref_expect as ME
import qp_map_expect as QE
from step_chain import sao_rdo_inputs
from test_gpu_tu_passes import _assert_plane, _dev_plane, _fill_outputs, _mvs, _nthreads, _passes, _phases, _picture, _sentinel

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")

PREFILL = 0x5a5a5a5a


def _up(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _select_on_device(case, level, ref_cost, nrefs, ref_ids, optional=True):
    import torch
    dev = torch.device("cuda:0")
    nb = case.nctu * (64 >> (2 * level))
    hosts = (case.recs * 2)[:nrefs]
    recs = [_up(r.reshape(-1), dev) for r in hosts]
    idx = torch.full((nb,), 0x5a, dtype=torch.int8, device=dev)
    rid = torch.full((nb,), 0x5a, dtype=torch.int8, device=dev) if optional else None
    cost = torch.full((nb * nrefs,), PREFILL, dtype=torch.int32, device=dev) if optional else None
    mvo = torch.full((case.nctu * 85 * 2,), PREFILL, dtype=torch.int32, device=dev)
    A.ref_select(case.depth, case.w64, case.h64, level, recs, ref_cost, idx, mvo, ref_id=rid, cost_out=cost, ref_ids=ref_ids)
    torch.cuda.synchronize()
    for r, h in zip(recs, hosts):
        assert np.array_equal(r.cpu().numpy(), h.reshape(-1)), "an input changed"
    g = lambda t: None if t is None else t.cpu().numpy()
    return g(idx), g(rid), g(cost), g(mvo).reshape(-1, 2)


def _assert_select(got, e, level, nctu, nrefs, what):
    idx, rid, cost, mvo = got
    assert np.array_equal(idx, e["ref_idx"]), f"{what}: ref_idx differs on {int(np.count_nonzero(idx != e['ref_idx']))} blocks"
    # entries of other levels still hold the pre-fill
    assert np.array_equal(mvo, ME.full_mv_out(level, nctu, e["mv_out"], PREFILL)), f"{what}: mv_out differs"
    if rid is not None:
        assert np.array_equal(rid, e["ref_id"]), f"{what}: ref_id differs"
        assert np.array_equal(cost.reshape(-1, nrefs), e["cost"]), f"{what}: cost_out differs"


@pytest.mark.parametrize("ref_cost", [ME.COST_DEFAULT, ME.COST_FLAT, ME.COST_REVERSED], ids=["default", "flat", "reversed"])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("depth", [8, 10])
def test_ref_select_equals_the_expectation_on_the_six_stripe_picture(depth, level, ref_cost):
    case = ME.five_ref(depth, 3)
    ids = (4, 9, 2, 7)
    e = case.expect(level, ref_cost, ref_ids=ids)
    what = f"{depth}-bit level {level} ref_cost {ref_cost}"
    _assert_select(_select_on_device(case, level, ref_cost, 4, ids), e, level, case.nctu, 4, what)
    assert len(np.unique(e["ref_idx"])) == 4 and set(np.unique(e["ref_id"])) == set(ids), what


@pytest.mark.parametrize("nrefs", [1, 2, 4, 8])
def test_ref_select_with_one_to_eight_references(nrefs):
    """8 references = the four planes twice: the first copy wins every tie.  Also with ref_id and cost_out left NULL."""
    case = ME.five_ref(8, 2)
    cost = (ME.COST_FLAT * 2)[:nrefs] if nrefs != 4 else A.ref_cost_bits(4)
    for level in (0, 2):
        e = case.expect(level, cost, nrefs=nrefs)
        what = f"{nrefs} references level {level}"
        _assert_select(_select_on_device(case, level, cost, nrefs, None), e, level, case.nctu, nrefs, what)
        _assert_select(_select_on_device(case, level, cost, nrefs, None, optional=False), e, level, case.nctu, nrefs, what + " (no optional outputs)")
        assert e["ref_idx"].max() == min(nrefs, 4) - 1, what


def _assert_outputs(st, elev, ens, edist, what):
    """levels, numSig and SSE of a stage against the expectation; the case must code something (more than a DC here and there)"""
    assert np.array_equal(st.levels.cpu().numpy(), elev), f"{what}: levels differ"
    assert np.array_equal(st.num_sig.cpu().numpy().view(np.uint32), ens), f"{what}: numSig differs"
    assert np.array_equal(st.dist.cpu().numpy().view(np.uint64), edist), f"{what}: SSE differs"
    assert (ens > 1).any() and np.count_nonzero(elev) > 500, f"{what}: a degenerate case ({np.count_nonzero(elev)} levels)"


def _chroma_refs(depth, w, h, seed, n=5):
    """[(Cb, Cr) padded flat planes] of n pictures + (stride, org): textured chroma planes of a w x h (luma) picture"""
    clip = F.synth_clip(w, h, n, depth=depth, seed=seed)
    pads = [[F.pad_chroma(clip[k][c], w, h) for c in (1, 2)] for k in range(n)]
    return [[p[0] for p in pic] for pic in pads], pads[0][0][1], pads[0][0][2]


def _luma_stage_vs_assembly(depth, level, cur, refs, stride, org, w, h, mv, ref_idx, qp, flags, what, qp_cells=None):
    """cur / refs: padded host luma planes"""
    import torch
    dev = torch.device("cuda:0")
    nctu = (w // 64) * (h // 64)
    pics = []
    for pl in [cur] + list(refs):
        inner = pl[F.MARGIN_Y:F.MARGIN_Y + h, F.MARGIN_X:F.MARGIN_X + w]
        pics.append(P.DevicePicture(np.ascontiguousarray(inner), dev))
        assert np.array_equal(pics[-1].host, pl), "DevicePicture pads like frames.pad_plane"
    st = S.InterReconRefs(nctu, w, h, depth, level, qp, dev, intra_slice=flags)
    _fill_outputs(st)
    if qp_cells is not None:
        st.qp_map = _up(np.asarray(qp_cells, np.int8).reshape(-1), dev)
    recon = torch.full_like(pics[0].t, _sentinel(depth))
    st.run(pics[0], pics[1:], recon, _up(mv.reshape(-1), dev), _up(np.asarray(ref_idx, np.int8), dev))
    torch.cuda.synchronize()
    erec, elev, ens, edist = ME.recon_luma(depth, cur, refs, stride, org, w, h, level, mv, np.clip(ref_idx, 0, len(refs) - 1), qp, flags, qp_cells, _nthreads())
    _assert_outputs(st, elev, ens, edist, what)
    _assert_plane(recon.cpu().numpy().view(cur.dtype), erec, stride, org, w, h, _sentinel(depth), what)


def _chroma_stage_vs_assembly(depth, level, w, h, mv, ref_idx, qps, flags, what, seed, qp_cells=None):
    """Both planes: the pair in one launch against the assembly, then against two single launches."""
    import torch
    dev = torch.device("cuda:0")
    nctu = (w // 64) * (h // 64)
    planes, stride, org = _chroma_refs(depth, w, h, seed)
    d_mv, d_idx = _up(mv.reshape(-1), dev), _up(np.asarray(ref_idx, np.int8), dev)
    fencs = [_dev_plane(planes[4][c], dev) for c in range(2)]
    frefs = [[_dev_plane(planes[3 - k][c], dev) for k in range(4)] for c in range(2)]
    runs = []
    for pair in (True, False):
        sts = [S.InterReconChromaRefs(nctu, w, h, depth, level, qps[c], dev, intra_slice=flags) for c in range(2)]
        recons = [torch.full_like(f, _sentinel(depth)) for f in fencs]
        for c, st in enumerate(sts):
            _fill_outputs(st)
            if qp_cells is not None:
                st.qp_map = _up(np.asarray(qp_cells[c], np.int8).reshape(-1), dev)
        if pair:
            S.InterReconChromaRefs.run_pair(sts, fencs, frefs, recons, stride, org, d_mv, d_idx)
        else:
            for c in range(2):
                sts[c].run(fencs[c], frefs[c], recons[c], stride, org, d_mv, d_idx)
        torch.cuda.synchronize()
        runs.append((sts, recons))
    for c in range(2):
        erec, elev, ens, edist = ME.recon_chroma(depth, planes[4][c], [planes[3 - k][c] for k in range(4)], stride, org, w, h, level, mv, ref_idx, qps[c], flags,
                                                 None if qp_cells is None else qp_cells[c], _nthreads())
        for (sts, recons), name in zip(runs, ("pair", "single")):
            _assert_outputs(sts[c], elev, ens, edist, f"plane {c} {name}, {what}")
            _assert_plane(recons[c].cpu().numpy().view(planes[4][c].dtype), erec, stride, org, w // 2, h // 2, _sentinel(depth), f"plane {c} {name}, {what}")


@pytest.mark.parametrize("depth,level,flags", [(8, 0, 2), (8, 1, 0), (8, 2, 2), (10, 0, 0), (10, 1, 2), (10, 2, 0), (12, 1, 2)])
def test_inter_recon_refs_equal_the_per_block_assembly(depth, level, flags):
    """The six-stripe picture with the oracle's records and the expected ref_idx (all four references chosen): luma, and Cb / Cr as a pair
    and as two launches.  flags 2: sign hiding."""
    case = ME.five_ref(depth, 3)
    e = case.expect(level, ME.COST_DEFAULT)
    assert len(np.unique(e["ref_idx"])) == 4
    mv = ME.full_mv_out(level, case.nctu, e["mv_out"], 0)
    qp = 28 + 6 * (depth - 8)
    what = f"{depth}-bit level {level} flags {flags}"
    _luma_stage_vs_assembly(depth, level, case.cur, case.refs, case.stride, case.org, case.w64, case.h64, mv, e["ref_idx"], qp, flags, what)
    _chroma_stage_vs_assembly(depth, level, case.w64, case.h64, mv, e["ref_idx"], (qp - 9, qp - 12), flags, what, 310 + depth)


@pytest.mark.parametrize("depth,level", [(8, 2), (10, 1)])
def test_inter_recon_refs_with_a_qp_map(depth, level):
    case = ME.five_ref(depth, 3)
    e = case.expect(level, ME.COST_DEFAULT)
    mv = ME.full_mv_out(level, case.nctu, e["mv_out"], 0)
    nb = len(e["ref_idx"])
    rng = np.random.default_rng([41, depth, level])
    vals = QE.map_values(depth)[2:6]
    cells = [QE.cells_of_blocks(rng.choice(vals, size=nb), case.w64, case.h64, level) for _ in range(3)]
    assert len({(int(r), int(q)) for r, q in zip(e["ref_idx"], QE.blocks_of_cells(cells[0], case.w64, case.h64, level))}) == 16
    what = f"{depth}-bit level {level} with a qp_map"
    _luma_stage_vs_assembly(depth, level, case.cur, case.refs, case.stride, case.org, case.w64, case.h64, mv, e["ref_idx"], 30, 2, what, cells[0])
    _chroma_stage_vs_assembly(depth, level, case.w64, case.h64, mv, e["ref_idx"], (30, 30), 2, what, 410 + depth, cells[1:])


@pytest.mark.parametrize("depth,level", [(8, 0), (8, 1), (10, 2)])
def test_alternating_ref_idx_with_vectors_of_every_phase(depth, level):
    """A hand-made ref_idx that changes from block to block (also out of range: clamped), with synthesised vectors of every phase: a
    kernel that reads the previous block's prefetched patch pointer fails this."""
    w, h = 256, 128
    nctu = (w // 64) * (h // 64)
    nb = nctu * (64 >> (2 * level))
    rng = np.random.default_rng([43, depth, level])
    mv = _mvs(rng, nctu)
    if level < 2:
        assert len(_phases(mv, nctu, level, 3)) == 16
    idx = (np.arange(nb) % 4).astype(np.int8)
    idx[5::16], idx[9::16] = -3, 11                     # outside [0, nrefs): clamped to 0 / 3
    clip = F.synth_clip(w, h, 5, depth=depth, seed=430 + depth)
    pads = [F.pad_plane(clip[k][0]) for k in (4, 3, 2, 1, 0)]
    stride, org = pads[0][1], pads[0][2]
    what = f"alternating ref_idx, {depth}-bit level {level}"
    _luma_stage_vs_assembly(depth, level, pads[0][0], [p[0] for p in pads[1:]], stride, org, w, h, mv, idx, 26 + 6 * (depth - 8), 2, what)
    _chroma_stage_vs_assembly(depth, level, w, h, mv, np.clip(idx, 0, 3), (21 + 6 * (depth - 8), 18 + 6 * (depth - 8)), 2, what, 440 + depth)


@pytest.mark.parametrize("depth,level", [(8, 1), (10, 2), (8, 2)])
def test_inter_recon_refs_multi_pass(depth, level):
    """The persistent 16 / 32-point luma kernels past their first resident pass, ref_idx random over 4 planes."""
    n = 8 << level
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_REFS, n, depth, False, (64 // n) ** 2)
    what = f"refs luma {n}x{n} {depth}-bit: " + _passes(nb, g, tail=level == 2)
    rng = np.random.default_rng([45, depth, level])
    nctu = (w // 64) * (h // 64)
    mv = _mvs(rng, nctu)
    idx = rng.integers(0, 4, size=nb).astype(np.int8)
    clip = F.synth_clip(w, h, 5, depth=depth, seed=450 + level)
    pads = [F.pad_plane(clip[k][0]) for k in (4, 3, 2, 1, 0)]
    _luma_stage_vs_assembly(depth, level, pads[0][0], [p[0] for p in pads[1:]], pads[0][1], pads[0][2], w, h, mv, idx, 30 + 6 * (depth - 8), 2, what)


@pytest.mark.parametrize("depth", [8, 10])
def test_inter_recon_chroma_pair_refs_multi_pass(depth):
    """The persistent 16-point chroma kernel, Cb and Cr in one launch (the grid split over the planes), past its first pass."""
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_CHROMA_REFS, 16, depth, False, 4, 2)
    what = f"refs chroma pair 16x16 {depth}-bit: " + _passes(nb, g, tail=True)
    rng = np.random.default_rng([47, depth])
    nctu = (w // 64) * (h // 64)
    mv = _mvs(rng, nctu)
    assert len(_phases(mv, nctu, 2, 7)) == 64
    idx = rng.integers(0, 4, size=nb).astype(np.int8)
    _chroma_stage_vs_assembly(depth, 2, w, h, mv, idx, (32, 29), 2, what, 470 + depth)


# ---- the step and the mini-GOP ---------------------------------------------------------------------------------------------------
W, H, R = 256, 192, 12


def _step(depth, dev, qp, subme=3, level=2, max_refs=4, sao=True, **kw):
    return S.MultiRefFramePipeline(W, H, depth, dev, max_refs=max_refs, rng=R, subme=subme, level=level, qp=qp, deblock=True, sao=sao, chroma=True,
                                   sao_apply=sao, sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P) if sao else None, want_cost=True, **kw)


def _clip5(depth, seed=81):
    """five pictures whose occluded bands (tests/bidir_expect.py) make older references the better ones for part of the picture"""
    return BE.occluded_clip(W, H, 5, depth, seed)


def _pics(clip, dev):
    return [P.DevicePicture(y, dev, u, v) for (y, u, v) in clip]


@pytest.mark.parametrize("depth,level", [(8, 2), (10, 2), (8, 1)])
def test_step_every_stage_equals_the_oracle_chain(depth, level):
    """MultiRefFramePipeline.run at 256x192 with 4 references, chroma, deblocking, SAO with the rate-distortion decision and sign hiding."""
    import torch
    dev = torch.device("cuda:0")
    qp = 30 + 12 * (depth == 10)
    clip = _clip5(depth)
    pics = _pics(clip, dev)
    pipe = _step(depth, dev, qp, level=level)
    marks = []
    pipe.run(pics[4], [pics[3 - k] for k in range(4)], mark=marks.append)
    torch.cuda.synchronize()
    assert marks == [m % r for r in range(4) for m in ("me%d", "subpel%d")] + ["ref_select", "recon", "recon_chroma", "deblock", "sao_stats", "sao_rdo",
                                                                                "sao_apply", "border"]
    hp = [BE.padded_planes(c)[0] for c in clip]
    cpu = ME.p_chain_refs(depth, hp[4], [hp[3 - k] for k in range(4)], W, H, R, 3, level, qp, sao_rdo=pipe.sao_rdo, cores=_nthreads())
    bad = BE.compare(ME.device_outputs(pipe, pics[0].host.dtype, 4), cpu)
    assert not bad, bad
    assert len(np.unique(cpu["ref_idx"])) >= 2, np.bincount(cpu["ref_idx"], minlength=4).tolist()
    assert int(cpu["num_sig"].sum()) > 0 and (cpu["bs_ver"] > 0).any() and (cpu["bs_hor"] > 0).any()
    assert set(pipe.checksum()) >= {"best0", "best3", "subpel0", "subpel3", "ref_idx", "mv_out", "levels", "recon"}
    assert [p.shape for p in pipe.final_planes()] == [p.shape for p in pics[4].planes()]


@pytest.mark.parametrize("depth", [8, 10])
def test_one_reference_is_the_p_step_and_copies_change_nothing(depth):
    """With one reference the final planes equal FramePipeline's on the same input; with four copies of that reference they equal the
    one-reference result and ref_idx is all zero."""
    import torch
    dev = torch.device("cuda:0")
    qp = 30 + 12 * (depth == 10)
    pics = _pics(_clip5(depth, 83)[:2], dev)
    fp = S.FramePipeline(W, H, depth, dev, rng=R, subme=3, level=2, qp=qp, want_surf=False, deblock=True, sao=True, chroma=True, sao_apply=True,
                         sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P))
    fp.run(pics[1], pics[0])
    pipe = _step(depth, dev, qp)
    pipe.run(pics[1], [pics[0]])
    torch.cuda.synchronize()
    one = [p.clone() for p in pipe.final_planes()]
    for g, e in zip(one, fp.final_planes()):
        assert torch.equal(g, e), "one reference: not the P step's picture"
    assert torch.equal(pipe.rc.levels, fp.rc.levels) and int(pipe.rc.num_sig.sum()) > 0
    pipe.rs.ref_idx.fill_(0x5a)
    pipe.run(pics[1], [pics[0]] * 4)
    torch.cuda.synchronize()
    assert int(pipe.rs.ref_idx.abs().max()) == 0
    for g, e in zip(pipe.final_planes(), one):
        assert torch.equal(g, e), "four copies of one reference: not the one-reference picture"


def test_step_with_chroma_satd():
    """chroma_satd=True at subme 3: every reference's records are the chroma walk's (tests/subpel_chroma_expect.py)."""
    import torch
    dev = torch.device("cuda:0")
    depth, qp = 8, 30
    clip = _clip5(depth, 85)
    pics = _pics(clip, dev)
    pipe = _step(depth, dev, qp, max_refs=3, sao=False, chroma_satd=True)
    pipe.run(pics[4], [pics[3], pics[2], pics[1]])
    torch.cuda.synchronize()
    hp = [BE.padded_planes(c)[0] for c in clip]
    cpu = ME.p_chain_refs(depth, hp[4], [hp[3], hp[2], hp[1]], W, H, R, 3, 2, qp, chroma_satd=True, sao=False, cores=_nthreads())
    bad = BE.compare(ME.device_outputs(pipe, pics[0].host.dtype, 3), cpu)
    assert not bad, bad
    luma = ME.p_chain_refs(depth, hp[4], [hp[3], hp[2], hp[1]], W, H, R, 3, 2, qp, sao=False, cores=_nthreads())
    assert not np.array_equal(luma["mv_out"], cpu["mv_out"]), "the chroma records changed nothing"


def test_step_with_qp_maps():
    import torch
    dev = torch.device("cuda:0")
    depth, qp, level = 8, 30, 2
    clip = [tuple(p) for p in QE.varied_clip(_clip5(depth, 87), depth)]
    pics = _pics(clip, dev)
    refs = [pics[3 - k] for k in range(4)]
    pipe = _step(depth, dev, qp, sao=False)
    pipe.run(pics[4], refs)
    torch.cuda.synchronize()
    uniform = pipe.checksum()
    aq = S.AdaptiveQuant(W, H, depth, dev, qg_size=16, aq_mode=2, aq_strength=1.0)
    offs, _, _, _ = aq.run(pics[4], cb=pics[4].c[0], cr=pics[4].c[1], stride_c=pics[4].stride_c, org_c=pics[4].org_c)
    maps = S.CuQpMaps(W, H, depth, level, dev, qg_size=16).run(qp + 0.3, offs)
    assert len(np.unique(maps.cu_qp_host)) >= 3
    pipe.set_qp_maps(maps)
    pipe.run(pics[4], refs)
    torch.cuda.synchronize()
    assert pipe.checksum() != uniform
    hp = [BE.padded_planes(c)[0] for c in clip]
    cpu = ME.p_chain_refs(depth, hp[4], [hp[3 - k] for k in range(4)], W, H, R, 3, level, qp, cu_qp=maps.cu_qp_host, tu_qp=maps.tu_qp_host, sao=False,
                          cores=_nthreads())
    bad = BE.compare(ME.device_outputs(pipe, pics[0].host.dtype, 4), cpu)
    assert not bad, bad
    pipe.set_qp_maps(None)
    pipe.run(pics[4], refs)
    torch.cuda.synchronize()
    assert pipe.checksum() == uniform


def test_mini_gop_with_three_p_references():
    """MiniGop(p_refs=3), gop 2, 7 pictures: every anchor equals p_chain_refs fed the previous coded anchors, newest first; with p_refs=1
    the driver is today's."""
    import torch
    from test_gpu_bpicture import _b_step
    dev = torch.device("cuda:0")
    depth, qp, gop = 8, 30, 2
    clip = BE.occluded_clip(W, H, 7, depth, 89)
    pics = _pics(clip, dev)
    b_step = _b_step(W, H, depth, dev, R, 3, 2, qp)
    p_step = _step(depth, dev, qp, max_refs=3)
    order, out = S.MiniGop(p_step, b_step, gop, p_refs=3).run(pics)
    torch.cuda.synchronize()
    assert order == [0, 2, 1, 4, 3, 6, 5] and sorted(out) == list(range(7))
    dt = pics[0].host.dtype
    shape = pics[0].host.shape
    want = {0: [p.reshape(-1) for p in BE.padded_planes(clip[0])[0]]}
    used = set()
    for a in (2, 4, 6):
        refs = [(want[k][0].reshape(shape), want[k][1], want[k][2]) for k in range(a - gop, -1, -gop)][:3]
        o = ME.p_chain_refs(depth, BE.padded_planes(clip[a])[0], refs, W, H, R, 3, 2, qp, sao_rdo=p_step.sao_rdo, cores=_nthreads())
        want[a] = [o["recon"].reshape(-1), o["recon_c0"].reshape(-1), o["recon_c1"].reshape(-1)]
        used |= set(np.unique(o["ref_idx"]).tolist())
        for name, g, e in zip(("Y", "Cb", "Cr"), out[a], want[a]):
            g = g.cpu().numpy().view(dt).reshape(-1)
            assert np.array_equal(g, e), f"anchor {a} {name}: {int(np.count_nonzero(g != e))} of {e.size} samples differ"
    assert len(used) >= 2, used

    def today(**kw):
        fp = S.FramePipeline(W, H, depth, dev, rng=R, subme=3, level=2, qp=qp, want_surf=False, deblock=True, sao=True, chroma=True, sao_apply=True,
                             sign_hide=True, sao_rdo=sao_rdo_inputs(depth, qp, HT.SLICE_P))
        return S.MiniGop(fp, b_step, gop, **kw).run(pics)
    (o1, out1), (o2, out2) = today(), today(p_refs=1)
    torch.cuda.synchronize()
    assert o1 == o2
    for k in out1:
        for g, e in zip(out2[k], out1[k]):
            assert torch.equal(g, e), f"picture {k}: p_refs=1 is not today's mini-GOP"
