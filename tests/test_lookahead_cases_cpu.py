"""The inputs of the lookahead limit tests (tests/lookahead_cases.py) checked with the oracle alone: every case the GPU module runs must
really reach the path it is listed for - every reachable intra mode chosen somewhere, both ends of the mode scan, the pure modes winning
through the clip of their edge filter, cuTree funnels, borders and bi-prediction ends, weights that clip at 0 and at max, an intra cap
that binds and one that does not, sums of squares above 2^31 - and the oracle must equal the real Lowres / LookaheadTLD classes
(oracle/_ref) on these same inputs where the classes can take them.  The cuTree step, which the real class only runs on motion fields of
its own, has a plain numpy restatement as its second reference.  These are conditions on the inputs: a case that misses one gets another
seed or other parameters, never a looser condition."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import lookahead_cases as LA

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = LA.F


def _ref(depth, symbol):
    path = os.path.join(ROOT, "oracle", "_ref", f"libx265ref{depth}.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref not built (needs the reference sources)")
    lib = ctypes.CDLL(path)
    if not hasattr(lib, symbol):
        pytest.skip(f"oracle/_ref predates {symbol}")
    return lib


def _real_preparation_equals_oracle(depth, img, label):
    """x265ref_lowres_intra (the real Lowres::init + LookaheadTLD::lowresIntraEstimate) against the oracle in the real class's geometry:
    the four planes with their borders, intraCost, intraMode, lowresCosts."""
    O = LA.oracle()
    lib = _ref(depth, "x265ref_lowres_intra")
    height, width = img.shape
    src, stride, org, _, _ = F.pad_plane(img)
    wcu, hcu = (width // 2 + 7) >> 3, (height // 2 + 7) >> 3
    lw, lh = wcu * 8, hcu * 8
    rstride = (width // 2 + 2 * F.MARGIN_X + 31) & ~31                  # Lowres::create, lowres.cpp:59-61
    rows = lh + 2 * F.MARGIN_Y
    geo = (ctypes.c_int * 5)()
    rplanes = [np.zeros(rstride * rows, dtype=img.dtype) for _ in range(4)]
    rcost, rmode, rlc = np.zeros(wcu * hcu, np.int32), np.zeros(wcu * hcu, np.uint8), np.zeros(wcu * hcu, np.uint16)
    lib.x265ref_lowres_intra.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_void_p] * 7
    assert lib.x265ref_lowres_intra(src.ctypes.data, width, height, geo, *[p.ctypes.data for p in rplanes], rcost.ctypes.data, rmode.ctypes.data, rlc.ctypes.data) == 0
    assert tuple(geo) == (lw, lh, rstride, wcu, hcu), label
    lorg = rstride * F.MARGIN_Y + F.MARGIN_X
    planes = O.lowres_init(depth, src, stride, org, rstride, lorg, rows, lw, lh, F.MARGIN_X, F.MARGIN_Y)
    for i in range(4):
        a = planes[i].reshape(rows, rstride)[:, :lw + 2 * F.MARGIN_X]
        b = rplanes[i].reshape(rows, rstride)[:, :lw + 2 * F.MARGIN_X]
        if lw + 2 * F.MARGIN_X > rstride:      # rounded-up width: the reference's right margin runs into the next row (lowres.cpp:59-66)
            a, b = a[:, :F.MARGIN_X + lw], b[:, :F.MARGIN_X + lw]
        assert np.array_equal(a, b), f"{label}: lowres plane {i} differs from Lowres::init"
    cost, mode, lc = O.lowres_intra(depth, planes[0], rstride, lorg, wcu, hcu, LA.PENALTY[depth])
    assert np.array_equal(cost, rcost) and np.array_equal(mode, rmode) and np.array_equal(lc, rlc), label


# ---- intra estimate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_mode_chart_reaches_every_mode_and_both_ends_of_the_scan(depth):
    """On the chart the oracle chooses every mode 0 .. 33 (34 cannot come out of a 5 .. 30 coarse scan followed by +-2 and +-1), so the second
    round has held the modes 2 .. 8 (a winner in {2, 3, 4} needs the coarse winner 5) and 27 .. 33 (a winner in {31, 32, 33} needs 30); at
    10 and 12 bits the noise regions saturate lowresCosts at 16383.  Penalty 0 changes the costs and nothing else."""
    p = LA.prepare(depth, LA.mode_chart(depth), LA.PENALTY[depth])
    modes = p.mode.tolist()
    census = {m: modes.count(m) for m in range(35)}
    print(depth, "modes reached:", sum(v > 0 for v in census.values()), census, "lowresCosts at 16383:", int((p.lc == 16383).sum()), "of", p.lc.size)
    assert set(modes) == set(range(34))
    assert {2, 3, 4} & set(modes) and {31, 32, 33} & set(modes)
    if depth > 8:
        assert (p.lc == 16383).any() and (p.lc < 16383).any()
    p0 = LA.prepare(depth, LA.mode_chart(depth), 0)
    assert np.array_equal(p0.mode, p.mode) and np.array_equal(p0.cost + LA.PENALTY[depth], p.cost)


@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_mode_chart_equals_the_real_classes(depth):
    _real_preparation_equals_oracle(depth, LA.mode_chart(depth), f"chart d{depth}")


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_pure_modes_win_through_the_edge_filter_clip(depth, transposed):
    """Mode 26 (transposed: 10) wins on at least 8 blocks whose unclipped edge value lies above max and on at least 8 where it lies below 0."""
    c = LA.clip_plane(depth, transposed)
    for penalty in (LA.PENALTY[depth], 0):
        cost, mode, lc = LA.oracle().lowres_intra(depth, c.plane, c.stride, c.org, c.wcu, c.hcu, penalty)
        hi, lo = LA.clip_census(c, mode, transposed)
        print(depth, "transposed" if transposed else "upright", "clip winners above max / below 0:", hi, lo, "of 36 marked blocks")
        assert hi >= 8 and lo >= 8
        marked = mode.reshape(c.hcu, c.wcu)[1::2, 1::2]
        assert (marked == (10 if transposed else 26)).sum() >= 16 and (cost.reshape(c.hcu, c.wcu)[1::2, 1::2] == penalty + 4).sum() >= 16       # predicted exactly


@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_symmetric_plane_ties_mirrored_modes(depth):
    """On a diagonal block of n + n.T the transposed block is the block itself: the oracle's answer for the transposed plane is the mirrored
    mode (36 - m for the angular ones) unless the strict-less scan order decided a tie - then both give the same, lower, mode."""
    c = LA.tie_plane(depth)
    assert np.array_equal(c.img, c.img.T)
    cost, mode, _ = LA.oracle().lowres_intra(depth, c.plane, c.stride, c.org, c.wcu, c.hcu, LA.PENALTY[depth])
    diag = mode.reshape(c.hcu, c.wcu).diagonal()
    assert len(set(diag.tolist())) > 1


@pytest.mark.parametrize("depth", [10, 12])
def test_whole_pictures_reach_the_margins_the_idle_slots_and_the_rounding(depth):
    for c in LA.PICTURE_CASES:
        if c.depth != depth:
            continue
        p = LA.prepare(depth, LA.picture(c.kind, depth, c.width, c.height), LA.PENALTY[depth])
        g = p.g
        inner = [pl.reshape(g.rows, g.stride)[g.my:g.my + c.height // 2 - 1, g.mx:g.mx + c.width // 2 - 1] for pl in p.planes]
        if (c.width, c.height) == (200, 136):
            assert 2 * g.width > c.width and 2 * g.lines > c.height and g.wcu * g.hcu == 13 * 9          # reads the source margin
        if (c.width, c.height) == (16, 16):
            assert g.wcu * g.hcu == 1
        if c.kind in ("rows", "cols", "checker"):                       # (0 + max + 1) >> 1 at every level of the nested averages: rounded up
            assert all((pl == 1 << (depth - 1)).all() for pl in inner), c.id
        if c.kind == "max":
            assert all((pl.reshape(g.rows, g.stride)[:, :g.width + 2 * g.mx] == (1 << depth) - 1).all() for pl in p.planes) and (p.cost == LA.PENALTY[depth] + 4).all() and (p.mode == 1).all(), c.id
        if c.kind == "noise" and c.width > 16:
            assert (p.lc == 16383).any() and len(set(p.mode.tolist())) > 4, c.id


@pytest.mark.parametrize("depth", [10, 12])
def test_whole_pictures_equal_the_real_classes(depth):
    for c in LA.PICTURE_CASES:
        if c.depth == depth:
            _real_preparation_equals_oracle(depth, LA.picture(c.kind, depth, c.width, c.height), c.id)


# ---- cuTree ------------------------------------------------------------------------------------------------------------------------------
def test_cutree_restatement_equals_the_oracle_and_the_cases_reach_their_paths():
    cases = {c.id: c for c in LA.cutree_cases()}
    assert len(cases) == 11
    res = {}
    for c in cases.values():
        e0, e1 = LA.cutree_oracle(c)
        n0, n1, census = LA.cutree_restatement(c)
        assert np.array_equal(e0, n0), c.id
        assert (e1 is None and n1 is None) if not c.bframe else np.array_equal(e1, n1), c.id
        # the reference's int products stay defined
        assert (c.intra.astype(np.int64) * c.invq < 2 ** 31).all() and census.amount.max() < 2 ** 21, c.id
        res[c.id] = (e0, e1, census)
    c = cases["border"]
    d0, d1 = LA.cutree_oracle(c, depth=12)                             # the depth argument does not enter
    assert np.array_equal(d0, res["border"][0]) and np.array_equal(d1, res["border"][1])

    for name in ("funnel-small", "funnel-big"):
        e0, e1, census = res[name]
        c = cases[name]
        t = 5 * c.wcu + 11
        targets0 = sorted([t, t + 1, t + c.wcu, t + c.wcu + 1])
        assert np.nonzero(e0)[0].tolist() == targets0 and np.nonzero(e1)[0].tolist() == [t], name
        assert census.sources[1][t] >= 256 and (c.mv1 % 32 == 0).all() and (c.mv1 < 0).any(), name
        print(name, "list 0:", e0[targets0].tolist(), "list 1:", int(e1[t]), "from", int(census.sources[1][t]), "sources; largest amount", int(census.amount.max()))
        if name == "funnel-small":
            assert e0.max() < 65535 and e1.max() < 65535                  # the sums themselves, below saturation
        else:
            assert 2 ** 20 <= census.amount.max() < 2 ** 21 and (e0[targets0] == 65535).all() and e1[t] == 65535

    c, (e0, e1, census) = cases["border"], res["border"]
    print("border: landed", census.landed, "dropped", census.dropped)
    assert all(census.landed[s] > 0 and census.dropped[s] > 0 for s in ("left", "right", "top", "bottom"))
    for mv in (c.mv0, c.mv1):
        assert -1 in mv and -32 in mv and {0, 1, 31} <= set((mv & 31).reshape(-1).tolist())
        cux, cuy = (mv[:, 0] >> 5) + np.arange(c.wcu * c.hcu) % c.wcu, (mv[:, 1] >> 5) + np.arange(c.wcu * c.hcu) // c.wcu
        assert {-2, -1, c.wcu - 1, c.wcu} <= set(cux.tolist()) and {-2, -1, c.hcu - 1, c.hcu} <= set(cuy.tolist())

    for weight, (same, other) in ((0, (0, 1)), (64, (1, 0))):
        c = cases[f"bipred-{weight}"]
        e = res[c.id]
        assert ((c.lcost >> 14) == 3).all()
        assert np.array_equal(e[same], (c.r0, c.r1)[same]) and (e[other] != (c.r0, c.r1)[other]).any(), c.id

    for c in cases.values():
        if c.id.startswith("tiny") and not c.bframe:
            assert c.mv1 is None and c.r1 is None and ((c.lcost >> 14) < 2).all()


# ---- weighted reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_weights_clip_at_both_ends_and_the_intra_cap_binds_on_some_blocks(depth):
    O = LA.oracle()
    wc = LA.weight_case(depth)
    g = wc.g
    mx = (1 << depth) - 1
    n = wc.ref[0].size
    at_max = lambda w: sum(int((O.weight_plane(depth, p, w) == mx).sum()) for p in wc.ref[:1])
    at_zero = lambda w: sum(int((O.weight_plane(depth, p, w) == 0).sum()) for p in wc.ref[:1])
    counts = (at_max((127, 0, 127)), at_zero((1, 7, -128)), at_max((64, 6, 127)), at_zero((64, 6, -128)))
    print(depth, "samples at max / 0 / max / 0:", counts, "of", n)
    assert counts[0] > 0.9 * n and counts[1] == n and 0.4 * n < counts[2] < 0.6 * n and 0.4 * n < counts[3] < 0.6 * n
    assert (O.weight_plane(depth, wc.ref[0], (0, 0, 0)) == 0).all()
    assert np.array_equal(O.weight_plane(depth, wc.ref[0], (64, 6, 0)), wc.ref[0])
    bound = free = 0
    for launch in LA.WEIGHT_LAUNCHES:
        for cand in launch:
            blocks = LA.weight_block_costs(wc, cand)
            never = O.lowres_weight_cost(depth, wc.cur, wc.ref[0], g.stride, g.org, g.width, g.lines, wc.caps["never"], cand)
            own = O.lowres_weight_cost(depth, wc.cur, wc.ref[0], g.stride, g.org, g.width, g.lines, wc.caps["own"], cand)
            assert never == int(blocks.sum()) and own == int(np.minimum(blocks, wc.caps["own"]).sum()), cand
            bound += int((blocks > wc.caps["own"]).sum()); free += int((blocks < wc.caps["own"]).sum())
            print(depth, cand, "uncapped", never, "capped", own)
    print(depth, "intra cap bound on", bound, "blocks, not on", free)
    assert bound > 0 and free > 0


# ---- adaptive quantisation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", LA.DEPTHS)
def test_aq_cases_reach_the_top_of_the_sums_and_stay_finite(depth):
    O = LA.oracle()
    top_sqr = top_energy = False
    for c in LA.aq_cases(depth):
        yp, stride, org, kw = LA.aq_inputs(c)
        energy, qp, inv, sm, ssd = O.aq_frame(depth, yp, stride, org, c.width, c.height, qg_size=c.qg, aq_mode=c.mode, aq_strength=c.strength, weightp=True, **kw)
        assert np.isfinite(qp).all(), c.id
        # the library's host-side half (no device work) on the oracle's energies, the frame averages divided as the reference divides them
        hq, hinv = A.aq_offsets(depth, c.qg, c.mode, c.strength, energy, A.aq_average_blocks(c.width, c.height, c.qg))
        assert np.array_equal(hq, qp) and np.array_equal(hinv, inv), c.id
        if c.family in ("zero", "max") and (c.width, c.height) == (64, 48):
            assert not energy.any() and len(set(qp.tolist())) == 1, c.id              # mode 1: log2(max(energy, 1)); modes 2, 3: identical roots
        if depth == 12 and c.qg == 16:
            blk = yp.reshape(-1, stride)[org // stride:org // stride + 16, org % stride:org % stride + 16].astype(np.int64)
            top_sqr |= c.family == "max" and int((blk * blk).sum()) == 256 * 4095 ** 2 > 2 ** 31
            top_energy |= c.family == "half" and int(energy.max()) > 2 ** 30
        if c.family == "noise":
            assert len(np.unique(inv)) > 2, c.id
    if depth == 12:
        assert top_sqr and top_energy


@pytest.mark.parametrize("depth", [8, 12])
def test_aq_cases_equal_the_real_class(depth):
    """x265ref_aq_frame (the real LookaheadTLD::calcAdaptiveQuantFrame): the pictures of whole blocks with chroma, the partial one luma
    only (the window synthesises no chroma padding)."""
    O = LA.oracle()
    lib = _ref(depth, "x265ref_aq_frame")
    lib.x265ref_aq_frame.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 5
    for c in LA.aq_cases(depth):
        chroma = (c.width, c.height) == (64, 48)
        yp, stride, org, kw = LA.aq_inputs(c, chroma=chroma)
        _, cb, cr = LA.aq_picture(c.family, depth, c.width, c.height)
        n = -(-c.width // c.qg) * -(-c.height // c.qg)
        rqp, rinv = np.zeros(4 * n + 64, np.float64), np.zeros(4 * n + 64, np.int32)
        rsum, rssd, rn = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(1, np.int32)
        assert lib.x265ref_aq_frame(yp.ctypes.data, cb.ctypes.data if chroma else None, cr.ctypes.data if chroma else None, c.width, c.height, c.qg, c.mode, c.strength, 1,
                                    rqp.ctypes.data, rinv.ctypes.data, rsum.ctypes.data, rssd.ctypes.data, rn.ctypes.data) == 0
        assert rn[0] == A.aq_average_blocks(c.width, c.height, c.qg) >= n, c.id          # the size of the real class's arrays
        energy, qp, inv, sm, ssd = O.aq_frame(depth, yp, stride, org, c.width, c.height, qg_size=c.qg, aq_mode=c.mode, aq_strength=c.strength, weightp=True, **kw)
        assert np.array_equal(sm, rsum) and np.array_equal(ssd, rssd), f"{c.id}: wp statistics {sm} {ssd} vs {rsum} {rssd}"
        assert np.array_equal(qp, rqp[:n]) and np.array_equal(inv, rinv[:n]), f"{c.id}: {np.count_nonzero(qp != rqp[:n])} QP offsets differ"


def _hevc_oracle(c):
    y = LA.aq_picture(c.family, c.depth, c.width, c.height)[0]
    yp, stride, org, _, _ = F.pad_plane(y)
    return yp, stride, org, LA.oracle().aq_hevc_frame(c.depth, yp.reshape(-1), stride, org, c.width, c.height, qg_size=c.qg, qp_adaptation_range=c.range, weightp=True)


def test_hevc_aq_cases_reach_the_clipped_partitions_and_stay_finite():
    O = LA.oracle()
    for c in LA.HEVC_AQ_CASES:
        yp, stride, org, (parts, act, qp, avg, inv, sm, ssd) = _hevc_oracle(c)
        assert np.isfinite(act).all() and np.isfinite(qp).all(), c.id
        if c.family == "max":
            assert (act == 1.0).all() and not qp.any() and (inv == 256).all(), c.id
        if c.width % 8 == 2:                                            # the last partitions are 2 samples wide / high: hw = hh = 1, one sample per quadrant
            part = 64 >> max(d for d in range(4) if parts[d])
            sums = O.aq_hevc_quadrants(c.depth, yp.reshape(-1), stride, org, c.width, c.height, part)
            last = sums[-1].astype(np.int64)
            img = LA.aq_picture(c.family, c.depth, c.width, c.height)[0].astype(np.int64)
            assert c.width % part == 2 and c.height % part == 2
            assert np.array_equal(last[:, 0], img[-2:, -2:].reshape(-1)) and np.array_equal(last[:, 1], img[-2:, -2:].reshape(-1) ** 2), c.id


@pytest.mark.parametrize("depth", [8, 12])
def test_hevc_aq_cases_equal_the_real_class(depth):
    lib = _ref(depth, "x265ref_aq_hevc_frame")
    lib.x265ref_aq_hevc_frame.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_int] + [ctypes.c_void_p] * 7
    for c in LA.HEVC_AQ_CASES:
        if c.depth != depth:
            continue
        yp, stride, org, (parts, act, qp, avg, inv, sm, ssd) = _hevc_oracle(c)
        total = int(parts.sum())
        rparts, ract, rqp, ravg = np.zeros(4, np.int32), np.zeros(total + 64, np.float64), np.zeros(total + 64, np.float64), np.zeros(4, np.float64)
        rinv, rsum, rssd = np.zeros(total + 64, np.int32), np.zeros(3, np.uint64), np.zeros(3, np.uint64)
        assert lib.x265ref_aq_hevc_frame(yp.ctypes.data, None, None, c.width, c.height, c.qg, c.range, 1, rparts.ctypes.data, ract.ctypes.data, rqp.ctypes.data,
                                         ravg.ctypes.data, rinv.ctypes.data, rsum.ctypes.data, rssd.ctypes.data) == 0
        assert np.array_equal(parts, rparts) and np.array_equal(act, ract[:total]) and np.array_equal(avg, ravg), c.id
        assert np.array_equal(qp, rqp[:total]) and np.array_equal(inv, rinv[:inv.size]), c.id
        assert np.array_equal(sm, rsum) and np.array_equal(ssd, rssd), f"{c.id}: wp statistics {sm} {ssd} vs {rsum} {rssd}"
