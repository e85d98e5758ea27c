"""GPU parity of the lookahead preparation kernels at 12 bits and at their limits: the cases of tests/lookahead_cases.py (which
tests/test_lookahead_cases_cpu.py shows to reach every path, and on which it pins the oracle against the real classes) through
x265hip_lowres_init / _lowres_intra / _cutree_propagate / _lowres_weight_cost / _lowres_weight_apply / _aq_energy / _aq_hevc_quadrants.
The oracle is the only expectation and every comparison is bit for bit."""
import importlib

import numpy as np
import pytest

import lookahead_cases as LA

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")


def _dev():
    import torch
    return torch.device("cuda:0")


def _up(a):
    """A host array as a device tensor of the same bits (torch has no uint16 / uint32)."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(signed) if signed else a).copy()).to(_dev())


def _down(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


# ---- picture preparation + intra estimate ------------------------------------------------------------------------------------------------
def _run_picture(depth, img, penalty, label):
    """stages.Lookahead on a picture: the four planes with their borders, intraCost, intraMode and lowresCosts against the oracle."""
    import torch
    h, w = img.shape
    pic = P.DevicePicture(img, _dev())
    la = S.Lookahead(w, h, depth, _dev(), intra_penalty=penalty)
    for t in la.planes + [la.intra_cost, la.intra_mode, la.lowres_costs]:
        t.fill_(0x5a)
    la.run(pic)
    torch.cuda.synchronize()
    e = LA.prepare(depth, img, penalty)
    g = e.g
    assert (la.stride, la.org, la.wcu, la.hcu) == (g.stride, g.org, g.wcu, g.hcu)
    for i in range(4):
        got = _down(la.planes[i], e.planes[i]).reshape(g.rows, g.stride)[:, :g.width + 2 * g.mx]
        exp = e.planes[i].reshape(g.rows, g.stride)[:, :g.width + 2 * g.mx]
        assert np.array_equal(got, exp), f"{label}: lowres plane {i} differs ({np.count_nonzero(got != exp)} samples)"
    assert np.array_equal(la.intra_cost.cpu().numpy(), e.cost), f"{label}: intraCost differs in blocks {np.nonzero(la.intra_cost.cpu().numpy() != e.cost)[0][:8].tolist()}"
    got = la.intra_mode.cpu().numpy()
    assert np.array_equal(got, e.mode), f"{label}: intraMode differs: blocks {np.nonzero(got != e.mode)[0][:8].tolist()} device {got[got != e.mode][:8].tolist()} oracle {e.mode[got != e.mode][:8].tolist()}"
    assert np.array_equal(_down(la.lowres_costs, e.lc), e.lc), f"{label}: lowresCosts differs"


@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_mode_chart_every_mode_and_both_ends_of_the_scan(depth):
    for penalty in (LA.PENALTY[depth], 0):
        _run_picture(depth, LA.mode_chart(depth), penalty, f"chart d{depth} penalty {penalty}")


@pytest.mark.parametrize("depth", [10, 12])
def test_whole_pictures_flat_full_range_and_alternating(depth):
    for c in LA.PICTURE_CASES:
        if c.depth == depth:
            _run_picture(depth, LA.picture(c.kind, depth, c.width, c.height), LA.PENALTY[depth], c.id)


def _run_plane(c, penalty, label):
    """x265hip_lowres_intra on a half-resolution plane handed over directly."""
    import torch
    n = c.wcu * c.hcu
    cost = torch.full((n,), -1, dtype=torch.int32, device=_dev())
    mode = torch.full((n,), 99, dtype=torch.uint8, device=_dev())
    lc = torch.full((n,), -1, dtype=torch.int16, device=_dev())
    A.lowres_intra(c.depth, _up(c.plane), c.stride, c.org, c.wcu, c.hcu, penalty, cost, mode, lc)
    torch.cuda.synchronize()
    ecost, emode, elc = LA.oracle().lowres_intra(c.depth, c.plane, c.stride, c.org, c.wcu, c.hcu, penalty)
    got = mode.cpu().numpy()
    bad = np.nonzero(got != emode)[0][:8]
    assert np.array_equal(got, emode), f"{label}: intraMode differs: blocks {bad.tolist()} device {got[bad].tolist()} oracle {emode[bad].tolist()}"
    assert np.array_equal(cost.cpu().numpy(), ecost), f"{label}: intraCost differs"
    assert np.array_equal(_down(lc, elc), elc), f"{label}: lowresCosts differs"


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_pure_modes_win_through_the_edge_filter_clip(depth, transposed):
    for penalty in (LA.PENALTY[depth], 0):
        _run_plane(LA.clip_plane(depth, transposed), penalty, f"clip d{depth} {'transposed' if transposed else 'upright'} penalty {penalty}")


@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_symmetric_plane_ties_fall_the_same_way(depth):
    for penalty in (LA.PENALTY[depth], 0):
        _run_plane(LA.tie_plane(depth), penalty, f"ties d{depth} penalty {penalty}")


# ---- cuTree ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LA.cutree_cases(), ids=lambda c: c.id)
def test_cutree_step_funnels_borders_bipred_ends_and_tiny_grids(case):
    import torch
    c = case
    e0, e1 = LA.cutree_oracle(c)
    opt = lambda a: None if a is None else _up(a)
    d0, d1 = _up(c.r0), opt(c.r1)
    A.cutree_propagate(c.wcu, c.hcu, opt(c.prop), _up(c.intra), _up(c.lcost), _up(c.invq), _up(c.mv0), opt(c.mv1), c.fps, c.bipred, d0, d1)
    torch.cuda.synchronize()
    g0 = _down(d0, e0)
    assert np.array_equal(g0, e0), f"list-0 reference: blocks {np.nonzero(g0 != e0)[0][:8].tolist()} device {g0[g0 != e0][:8].tolist()} oracle {e0[g0 != e0][:8].tolist()}"
    if c.bframe:
        g1 = _down(d1, e1)
        assert np.array_equal(g1, e1), f"list-1 reference: blocks {np.nonzero(g1 != e1)[0][:8].tolist()} device {g1[g1 != e1][:8].tolist()} oracle {e1[g1 != e1][:8].tolist()}"


# ---- weighted reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_weight_cost_at_the_ends_of_scale_denominator_and_offset(depth):
    """Both launches of four, and launches of 1, 2 and 3 candidates into a sentinel-filled output, with a cap that never binds and with
    the picture's own intra estimate."""
    import torch
    O = LA.oracle()
    wc = LA.weight_case(depth)
    g = wc.g
    d_cur, d_ref = _up(wc.cur), _up(wc.ref[0])
    for name, cap in wc.caps.items():
        d_cap = _up(cap)
        for launch in LA.WEIGHT_LAUNCHES:
            for ncand in (4, 1, 2, 3):
                cost = torch.full((4,), -7, dtype=torch.int32, device=_dev())
                A.lowres_weight_cost(depth, d_cur, d_ref, g.stride, g.org, g.width, g.lines, d_cap, launch[:ncand], cost)
                torch.cuda.synchronize()
                got = cost.cpu().numpy()
                exp = [O.lowres_weight_cost(depth, wc.cur, wc.ref[0], g.stride, g.org, g.width, g.lines, cap, cand) for cand in launch[:ncand]]
                assert got[:ncand].view(np.uint32).tolist() == exp, f"cap {name}, candidates {launch[:ncand]}"
                assert (got[ncand:] == -7).all(), f"cap {name}: {ncand} candidates wrote past their costs"


@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_weight_apply_clips_at_zero_and_at_max(depth):
    import torch
    O = LA.oracle()
    wc = LA.weight_case(depth)
    g = wc.g
    src = [_up(p) for p in wc.ref]
    for w in LA.WEIGHTS:
        dst = [torch.full_like(s, 0x5a) for s in src]
        A.lowres_weight_apply(depth, src, dst, g.stride, g.rows, w)
        torch.cuda.synchronize()
        for i in range(4):
            exp = O.weight_plane(depth, wc.ref[i], w)
            got = _down(dst[i], exp)
            assert np.array_equal(got, exp), f"weight {w}, plane {i}: {np.count_nonzero(got != exp)} samples differ"


# ---- adaptive quantisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_aq_pass_on_flat_half_checker_and_noise_pictures(depth):
    """stages.AdaptiveQuant with chroma: block energies (sums of squares up to 256 * 4095^2, above 2^31), wp_sum / wp_ssd, the QP offsets
    and invQscaleFactor - on whole and partial last blocks, --qg-size 16 and 8, AQ modes 1 - 3."""
    for c in LA.aq_cases(depth):
        yp, stride, org, kw = LA.aq_inputs(c)
        y = LA.aq_picture(c.family, depth, c.width, c.height)[0]
        pic = P.DevicePicture(y, _dev())
        assert (pic.stride, pic.org) == (stride, org)
        aq = S.AdaptiveQuant(c.width, c.height, depth, _dev(), qg_size=c.qg, aq_mode=c.mode, aq_strength=c.strength, weightp=True)
        aq.energy.fill_(0x5a5a5a5a)
        qp, inv, wp_sum, wp_ssd = aq.run(pic, cb=_up(kw["cb"]), cr=_up(kw["cr"]), stride_c=kw["stride_c"], org_c=kw["org_c"])
        energy, eqp, einv, esum, essd = LA.oracle().aq_frame(depth, yp, stride, org, c.width, c.height, qg_size=c.qg, aq_mode=c.mode, aq_strength=c.strength,
                                                             weightp=True, **kw)
        got = _down(aq.energy, energy)
        assert np.array_equal(got, energy), f"{c.id}: block energies differ in {np.nonzero(got != energy)[0][:8].tolist()}"
        assert wp_sum == [int(v) for v in esum] and wp_ssd == [int(v) for v in essd], f"{c.id}: wp statistics differ"
        assert np.array_equal(qp, eqp) and np.array_equal(inv, einv), f"{c.id}: {np.count_nonzero(qp != eqp)} QP offsets differ"


@pytest.mark.parametrize("case", LA.HEVC_AQ_CASES, ids=lambda c: c.id)
def test_hevc_aq_pass_on_flat_pictures_and_two_sample_partitions(case):
    c = case
    O = LA.oracle()
    y = LA.aq_picture(c.family, c.depth, c.width, c.height)[0]
    pic = P.DevicePicture(y, _dev())
    aq = S.HevcAq(c.width, c.height, c.depth, _dev(), qg_size=c.qg, qp_adaptation_range=c.range, weightp=True)
    for sm in aq.sums:
        sm.fill_(-1)
    layers, inv, wp_sum, wp_ssd = aq.run(pic)
    host = pic.host.reshape(-1)
    parts, act, qp, avg, einv, esum, essd = O.aq_hevc_frame(c.depth, host, pic.stride, pic.org, c.width, c.height, qg_size=c.qg, qp_adaptation_range=c.range, weightp=True)
    at = 0
    for d in range(4):
        part = 64 >> d
        if not parts[d]:
            assert part not in layers
            continue
        sums = aq.sums[aq.parts.index(part)].cpu().numpy().view(np.uint64).reshape(-1, 4, 2)
        assert np.array_equal(sums, O.aq_hevc_quadrants(c.depth, host, pic.stride, pic.org, c.width, c.height, part)), f"layer {d}: quadrant sums differ"
        a, q, g = layers[part]
        assert np.array_equal(a, act[at:at + parts[d]]) and np.array_equal(q, qp[at:at + parts[d]]) and g == avg[d], f"layer {d}: activities / offsets differ"
        at += parts[d]
    assert np.array_equal(inv, einv)
    assert wp_sum == [int(v) for v in esum] and wp_ssd == [int(v) for v in essd], "wp statistics differ"
