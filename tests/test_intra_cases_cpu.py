"""The inputs of the hostile-content tests of the I-picture stage (tests/intra_cases.py) checked with the walk of tests/intra_expect.py
alone: every case the GPU modules run must really reach what it is listed for - the clip of the edge filter of modes 10 / 26 at both
bounds, ties that the scan order decides, a rate term of 2^36, levels at both int16 limits, reconstructions at the limits of the sample
range, coded chroma.  These are conditions on the inputs: a case that misses one gets another picture, never a looser condition.  Where
oracle/_ref is built, the real reference's slots are called beside the oracle's in every walk below and must agree."""
import functools
import os

import numpy as np
import pytest

import harness
import intra_cases as IC
import intra_expect as IE
import qp_map_expect as QE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("mode", "cost", "levels", "num_sig", "dist")
CHROMA_OUTPUTS = tuple(k + "_c%d" % c for k in ("levels", "num_sig", "dist") for c in range(2))


@functools.lru_cache(maxsize=None)
def _have_reference(depth):
    return harness.load_reference(depth, ROOT) is not None


def _walk(c, seed=77):
    x = IC.expectation(c, _have_reference(c.depth), seed)
    assert x["e"]["tables"] == 1 + _have_reference(c.depth)
    return x["e"]


def _shares(e):
    return {k: float(m.mean()) for k, m in e["masks"].items()}


def _winners(e, mask=None):
    m = e["mode"] if mask is None else e["mode"][mask]
    return dict(zip(*(a.tolist() for a in np.unique(m, return_counts=True))))


def _ids(cases):
    return dict(argvalues=cases, ids=[c.id for c in cases])


@pytest.mark.parametrize("c", **_ids(IC.EDGE_CLIP_CASES))
def test_edge_clip_pictures_take_the_clip_at_both_bounds(c):
    """Levels 0 and 1, points mid and low-lambda, all depths: the winner is mode 10 or 26 and its unclipped edge filter leaves [0, max] on
    at least 3 % of the blocks, with both mode 10 and mode 26 among them and both bounds crossed.  Smallest share found: 11.2 % (level 0,
    12 bits, mid: 43 of 384 blocks, 18 of them mode 10); below 0 on at least 5.5 %, above max on at least 5.7 % of the blocks."""
    e = _walk(c)
    m, sh = e["masks"], _shares(e)
    print(c.id, {k: round(sh[k], 3) for k in ("edge_clip", "edge_clip_lo", "edge_clip_hi")}, "winners that clip", _winners(e, m["edge_clip"]))
    assert sh["edge_clip"] >= 0.03
    assert set(_winners(e, m["edge_clip"])) == {10, 26}
    assert m["edge_clip_lo"].any() and m["edge_clip_hi"].any()


@pytest.mark.parametrize("c", **_ids([c for c in IC.QP_MAX_CASES if c.kind.startswith("flat")]))
def test_flat_pictures_at_the_largest_qp_tie_on_every_block(c):
    """flat_hi / flat_lo at qp-max with lambda8 0: every block is a tie between several modes, DC - the first in scan order - wins every
    one, and nothing but the first block (predicted from 1 << (depth - 1)) is coded.  Share found: 100 % at every depth and level."""
    e = _walk(c)
    print(c.id, "ties", round(_shares(e)["cost_tie"], 3), "winners", _winners(e), "coded blocks", int((e["num_sig"] > 0).sum()))
    assert e["masks"]["cost_tie"].all() and (e["mode"] == 1).all()
    assert (e["num_sig"][1:] == 0).all() and (e["num_sig_c0"][1:] == 0).all() and (e["num_sig_c1"][1:] == 0).all()


@pytest.mark.parametrize("c", **_ids([c for c in IC.TIE_CASES if c.kind == "halves"]))
def test_halves_tie_between_most_probable_modes(c):
    """`halves` with mode bits (3, 3, 6): the three most probable modes cost the same on a flat block, so the first most probable mode
    (planar beside two DC neighbours) ties with DC and loses on scan order - tie_not_p0 on at least 3 % of the blocks of every level; with
    (6, 3, 2) the first most probable mode is the dearest and the tie is among the non-MPM modes - cost_tie on at least 3 %.  At least
    two distinct winners either way.  Smallest shares found: tie_not_p0 75.0 % (level 2; winners DC x 21, 26 x 3), cost_tie with (6, 3, 2) 95.8 % (level 2; five distinct winners)."""
    e = _walk(c)
    sh = _shares(e)
    print(c.id, {k: round(sh[k], 3) for k in ("cost_tie", "tie_not_p0")}, "winners", _winners(e))
    assert sh["cost_tie"] >= 0.03 and len(_winners(e)) >= 2
    if c.point == "mpm-ties-336":
        assert sh["tie_not_p0"] >= 0.03


@pytest.mark.parametrize("c", **_ids([c for c in IC.TIE_CASES if c.kind != "halves"]))
def test_flat_picture_with_free_mode_bits_ties(c):
    """flat_hi with lambda8 0 at the mid QP: cost_tie on at least 3 % of the blocks (found: 100 %)."""
    e = _walk(c)
    print(c.id, "ties", round(_shares(e)["cost_tie"], 3), "winners", _winners(e))
    assert _shares(e)["cost_tie"] >= 0.03


@pytest.mark.parametrize("c", **_ids(IC.QP_MIN_CASES))
def test_the_smallest_qp_saturates_the_levels(c):
    """qp 0: at 12 bits (levels 1 and 2) at least one block has a luma level at an int16 limit and both -32768 and 32767 occur; at 8 and
    10 bits the largest |level| exceeds 1000.  Found: both limits in all four 12-bit cases, level_sat on 3.1 % (edges, level 1) to 25 % of
    the blocks; 8 / 10 bits: largest |level| 1718 to 8516."""
    e = _walk(c)
    lev = e["levels"].astype(np.int64)
    print(c.id, "level_sat", round(_shares(e)["level_sat"], 3), "levels from", int(lev.min()), "to", int(lev.max()))
    if c.depth == 12:
        assert e["masks"]["level_sat"].any() and lev.min() == -32768 and lev.max() == 32767
    else:
        assert np.abs(lev).max() > 1000


@pytest.mark.parametrize("depth,level", [(d, l) for d in (8, 10, 12) for l in (0, 1, 2)])
def test_the_rate_term_reaches_two_to_the_28(depth, level):
    """edges at big-cost (lambda8 2^24, mode_bits 4096 x 3: bits * lambda8 = 2^36): every reported cost lies in [2^28, 2^31), cost - sad
    is 2^28 exactly, and the decision - by sa8d alone - has at least three distinct winners.  Found: 30 / 11 / 3 winners or more at levels
    0 / 1 / 2; the largest cost, 2^28 + 2.98 million, at 12 bits and level 2."""
    e = _walk(IC.case("edges", "big-cost", depth, level))
    sad, cost = e["cost"][:, 0].astype(np.int64), e["cost"][:, 1].astype(np.int64)
    print(f"edges-big-cost-d{depth}-l{level}", "cost from", int(cost.min()), "to", int(cost.max()), "winners", len(_winners(e)))
    assert (cost >= 1 << 28).all() and (cost < 1 << 31).all() and (cost - sad == 1 << 28).all()
    assert len(_winners(e)) >= 3


def test_a_cheap_first_mpm_beats_every_sa8d():
    """big-cost-mpm, (1, 4095, 4096): the first most probable mode pays 2^16 and the others 2^28 less 2^16 or 2^28 - more than any sa8d of
    a 16x16 block of 10-bit samples -, so it wins every block, at a cost below 2^28."""
    c = [k for k in IC.COST_CASES if k.point == "big-cost-mpm"][0]
    e = _walk(c)
    cost = e["cost"][:, 1].astype(np.int64)
    print(c.id, "cost from", int(cost.min()), "to", int(cost.max()), "winners", _winners(e))
    assert (cost - e["cost"][:, 0] == 1 << 16).all() and e["masks"]["mpm_priced"].all()


@pytest.mark.parametrize("kind", ["edges", "noise"])
@pytest.mark.parametrize("depth", [8, 10, 12])
def test_full_range_content_reconstructs_at_the_limits(depth, kind):
    """edges and noise at mid: at every level the reconstruction of at least 3 % of the blocks contains 0 or max, and chroma is coded on at
    least 3 %; at level 0 at least 8 distinct winners.  Smallest found: recon_at_limit 50.8 % (noise, level 0), chroma_coded 100 %, 29 winners."""
    for level in (0, 1, 2):
        e = _walk(IC.case(kind, "mid", depth, level))
        sh = _shares(e)
        print(f"{kind}-mid-d{depth}-l{level}", {k: round(sh[k], 3) for k in ("recon_at_limit", "chroma_coded")}, "winners", len(_winners(e)))
        assert sh["recon_at_limit"] >= 0.03 and sh["chroma_coded"] >= 0.03
        assert level or len(_winners(e)) >= 8


@pytest.mark.parametrize("c", **_ids(IC.ALL_CASES))
def test_the_walk_does_not_depend_on_the_recon_planes_before_it(c):
    """Every case the GPU tests run: two different fillings of the recon planes give the same outputs and the same picture area."""
    a, b = _walk(c), IC.expectation(c, False, 78)["e"]
    w64, h64 = IC.planes(c.depth, c.kind, c.level)[1:]
    _, _, stride, rows, _ = IE.F.padded_dims(w64, h64)
    sc = w64 // 2 + 2 * IE.F.CHROMA_MARGIN_X
    for k in OUTPUTS + (CHROMA_OUTPUTS if c.chroma else ()):
        assert np.array_equal(a[k], b[k]), k
    inner = lambda e: e["recon"].reshape(rows, stride)[IE.F.MARGIN_Y:IE.F.MARGIN_Y + h64, IE.F.MARGIN_X:IE.F.MARGIN_X + w64]
    assert np.array_equal(inner(a), inner(b)) and not np.array_equal(a["recon"], b["recon"])
    if c.chroma:
        for k in ("recon_c0", "recon_c1"):
            inner_c = lambda e: e[k].reshape(-1, sc)[IE.F.CHROMA_MARGIN_Y:IE.F.CHROMA_MARGIN_Y + h64 // 2, IE.F.CHROMA_MARGIN_X:IE.F.CHROMA_MARGIN_X + w64 // 2]
            assert np.array_equal(inner_c(a), inner_c(b)), k


@pytest.mark.parametrize("c", **_ids(IC.LUMA_ONLY_CASES))
def test_luma_does_not_read_chroma(c):
    """expect(chroma=False) - what the kernel without chroma planes is compared with - equals the luma outputs of the walk with chroma."""
    a, b = IC.expectation(c)["e"], IC.expectation(IC.case(c.kind, c.point, c.depth, c.level, c.sign_hide, c.strong, True))["e"]
    assert "levels_c0" not in a and "recon_c0" not in a
    for k in OUTPUTS + ("recon",):
        assert np.array_equal(a[k], b[k]), k
    assert int(a["num_sig"].sum()) > 0


def test_chroma_qp_is_the_stage_helper():
    import importlib
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    for depth in (8, 10, 12):
        for qp in range(52 + 6 * (depth - 8)):
            assert IC.chroma_qp(qp, depth) == S.chroma_quant_qp(qp, depth)


@pytest.mark.parametrize("depth", [8, 10])
def test_the_range_end_map_is_what_it_is_listed_for(depth):
    """The map of test_intra_picture_with_maps_at_the_range_ends: entries outside [0, max] (-128, -1, 127) in every plane; among the blocks' luma
    QPs after the clamp 0, 1, max - 1, max and two values between on at least 3 % of the blocks each; a block priced with the clamped lambda
    2^24 and one with lambda 0; and the walk on the map as given equals the walk on the map clamped beforehand."""
    level = 1
    tu, lam, values = IC.range_end_map(depth, level)
    qmax = 51 + 6 * (depth - 8)
    assert tu.dtype == np.int8 and all((tu[p] == v).any() for p in range(3) for v in (-128, -1, 127))
    assert int(lam.max()) > 1 << 24 and lam.dtype == np.uint32
    q = np.clip(QE.blocks_of_cells(tu[0], IC.WIDTH, IC.HEIGHT, level), 0, qmax)
    shares = {int(v): float((q == v).mean()) for v in np.unique(q)}
    print(f"depth {depth}:", {k: round(v, 3) for k, v in shares.items()})
    assert set(shares) == {0, 1, qmax - 1, qmax, values[4], values[5]} and min(shares.values()) >= 0.03
    pl, w64, h64 = IC.planes(depth, "edges", level)
    e = QE.walk(depth, pl, w64, h64, level, tu, lambda8_by_qp=lam, flags=3, with_reference=_have_reference(depth))
    assert (e["lambda8"] == 1 << 24).any() and (e["lambda8"] == 0).any() and int(e["lambda8"].max()) == 1 << 24
    clamped = np.clip(tu, 0, qmax).astype(np.int8)
    e2 = QE.walk(depth, pl, w64, h64, level, clamped, lambda8_by_qp=np.minimum(lam, 1 << 24), flags=3)
    for k in OUTPUTS + CHROMA_OUTPUTS + ("recon", "recon_c0", "recon_c1"):
        assert np.array_equal(e[k], e2[k]), k
