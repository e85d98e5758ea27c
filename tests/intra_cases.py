"""Deterministic inputs for the hostile-content tests of the I-picture stage (numpy and the oracle only, no torch): pictures on which the
parts of x265hip_intra_picture that textured mid-range content leaves idle have work to do - the clip of the edge filter of modes 10 / 26,
exact ties between modes, a rate term beyond 32 bits, levels at both int16 limits, reconstructions at the limits of the sample range -
and the operating points (qp, lambda8, mode_bits) that go with them.

tests/test_intra_cases_cpu.py asserts, with the walk of tests/intra_expect.py alone, that every case below really reaches what it is
listed for; tests/test_gpu_ipicture.py and tests/test_gpu_qp_steps.py feed the same cases to the kernel."""
import functools

import numpy as np

import intra_expect as IE
import qp_map_expect as QE
import subpel_cases as SC

H = IE.H

# 3 x 2 CTUs: a wave with two CTUs (wave 2 = CTUs (2, 0) and (0, 1)) and an above-right arm that comes from another CTU
WIDTH, HEIGHT = 192, 128
KINDS = ("edges", "flat_hi", "flat_lo", "halves", "edge_clip", "noise")          # the order is part of the random kinds' seeds
POINTS = ("mid", "low-lambda", "qp-max", "qp-min", "big-cost", "big-cost-mpm", "mpm-ties-336", "mpm-ties-632", "lambda-0")


def point(name, depth):
    """(qp, lambda8, mode_bits) of an operating point: qp is the luma quantiser's (CU QP + 6 (depth - 8))."""
    bd = 6 * (depth - 8)
    return {"mid": (30 + bd, 1024, (2, 3, 6)),
            "low-lambda": (22 + bd, 256, (2, 3, 6)),
            "qp-max": (51 + bd, 0, (2, 3, 6)),                         # nearly nothing is coded: reconstruction = prediction, ties everywhere
            "qp-min": (0, 64, (2, 3, 6)),                              # the largest levels the quantiser forms
            "big-cost": (30 + bd, 1 << 24, (4096, 4096, 4096)),        # every mode pays 2^28: decided by sa8d, reported cost = 2^28 + sad
            "big-cost-mpm": (30 + bd, 1 << 24, (1, 4095, 4096)),       # the first most probable mode pays 2^16, the others just below 2^28
            "mpm-ties-336": (30 + bd, 1024, (3, 3, 6)),                # the three most probable modes cost the same
            "mpm-ties-632": (30 + bd, 1024, (6, 3, 2)),                # the most probable mode is the dearest
            "lambda-0": (30 + bd, 0, (2, 3, 6))}[name]                 # the mode bits are free: every decision is by sa8d and scan order


# One seed per depth for the random kinds: the first from 41 on at which `edges` has three distinct winners among its 24 blocks of level 2 at
# big-cost and, at 12 bits and qp 0, levels at both int16 limits at levels 1 and 2 (tests/test_intra_cases_cpu.py asserts both).
SEEDS = {8: 41, 10: 44, 12: 56}


def chroma_qp(qp, depth):
    """Quant::setChromaQP (quant.cpp:233-244, 4:2:0, no offset) of a luma quantiser QP: what stages.chroma_quant_qp returns."""
    bd = 6 * (depth - 8)
    q = min(max(qp - bd, -bd), 57)
    return (QE.CHROMA_SCALE[q] if q >= 30 else q) + bd


def edge_clip_luma(depth, n, width=WIDTH, height=HEIGHT):
    """Bars n samples wide at the two ends of the range, the last column of every bar replaced by a ramp rising down the rows of a block:
    the left neighbours of a block lie below its corner by up to the whole range while its above row sits at 0, so the edge filter of
    mode 26, above[0] + ((left[y] - corner) >> 1), falls below 0 - and only its clip makes the prediction the flat column the source has,
    which is why mode 26 wins.  The right half of the picture is the pattern transposed: the same for mode 10.  The lower half is the
    complement max - sample: falling ramps beside bars at max, the filter exceeds max."""
    mx = (1 << depth) - 1
    half = width // 2

    def pattern(x, y):
        bars = np.where((x // n + y // (2 * n)) % 2 == 0, mx - (x % 3), x % 3)
        ramp = np.minimum((y % n) * (mx // 10) + mx // 8, mx)
        return np.where(x % n == n - 1, ramp, bars)
    yy, xx = np.mgrid[0:height, 0:width]
    y = np.where(xx < half, pattern(xx, yy), pattern(yy, xx - half))
    return np.where(yy < height // 2, y, mx - y).astype(IE.harness.pix_dtype(depth))


@functools.lru_cache(maxsize=None)
def build(depth, kind, level=0, width=WIDTH, height=HEIGHT):
    """(Y, Cb, Cr) of one kind at one depth (4:2:0); `level` matters for edge_clip only (its period is the block size 8 << level).  The
    result is shared between tests: read only."""
    assert kind in KINDS and width % 64 == 0 and height % 64 == 0
    mx = (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    rng = np.random.default_rng([SEEDS[depth], depth, KINDS.index(kind)])
    cw, ch = width // 2, height // 2
    if kind == "edges":
        yuv = [SC.edges_picture(rng, w, h, mx, dt) for w, h in ((width, height), (cw, ch), (cw, ch))]
    elif kind == "noise":
        yuv = [rng.integers(0, mx + 1, size=(h, w)).astype(dt) for w, h in ((width, height), (cw, ch), (cw, ch))]
        # The last CTU of luma: a sample-by-sample checkerboard between 0 and max whose phase flips from one 32x32 cell to the next - all of a
        # block's energy in one coefficient of either sign, which noise (whose coefficients stay near 0.8 of the int16 range at 12 bits) lacks.
        yy, xx = np.mgrid[0:64, 0:64]
        yuv[0][height - 64:, width - 64:] = (((xx + yy + xx // 32 + yy // 32) & 1) * mx).astype(dt)
    elif kind in ("flat_hi", "flat_lo"):
        hi = mx if kind == "flat_hi" else 0
        yuv = [np.full((height, width), hi, dt), np.full((ch, cw), mx - hi, dt), np.full((ch, cw), hi, dt)]
    elif kind == "halves":
        a, b = 200 << (depth - 8), 40 << (depth - 8)
        y = np.full((height, width), a, dt)
        y[:, width // 2:] = b
        c = np.full((ch, cw), b, dt)
        c[:, cw // 2:] = a
        yuv = [y, c, (a + b - c).astype(dt)]
    else:
        y = edge_clip_luma(depth, 8 << level, width, height)
        yuv = [y, y[::2, ::2].copy(), (mx - y[::2, ::2]).astype(dt)]
    for p in yuv:
        p.setflags(write=False)
    return tuple(yuv)


class Case(tuple):
    """(kind, point, depth, level, sign_hide, strong, chroma)"""
    kind, point, depth, level, sign_hide, strong, chroma = (property(lambda s, k=k: s[k]) for k in range(7))
    id = property(lambda s: f"{s.kind}-{s.point}-d{s.depth}-l{s.level}" + ("" if s.sign_hide else "-nosdh") + ("" if s.strong else "-weak") + ("" if s.chroma else "-luma"))
    flags = property(lambda s: H.TU_INTRA_SLICE | (H.TU_SIGN_HIDE if s.sign_hide else 0))


def case(kind, pt, depth, level, sign_hide=True, strong=True, chroma=True):
    assert kind in KINDS and pt in POINTS
    return Case((kind, pt, depth, level, sign_hide, strong, chroma))


@functools.lru_cache(maxsize=None)
def planes(depth, kind, level):
    """The padded host planes of a picture (what intra_expect.expect takes), and w64, h64: shared, read only."""
    pl, w64, h64 = IE.padded_planes(build(depth, kind, level if kind == "edge_clip" else 0))
    for p in pl:
        p.setflags(write=False)
    return pl, w64, h64


@functools.lru_cache(maxsize=None)
def expectation(c, with_reference=False, seed=77):
    """The walk's expectation of a case (shared: read only) and what it was run with: dict with yuv, w64, h64, qp, qp_c, lambda8, mode_bits,
    init (the recon planes' contents before the walk) and e (intra_expect.expect's result)."""
    pl, w64, h64 = planes(c.depth, c.kind, c.level)
    qp, lambda8, mode_bits = point(c.point, c.depth)
    qpc = chroma_qp(qp, c.depth)
    init = IE.garbage_planes(c.depth, [np.asarray(p).reshape(-1).shape for p in (pl if c.chroma else pl[:1])], seed=seed)
    e = IE.expect(c.depth, pl, w64, h64, c.level, qp, qp_c=(qpc, qpc), flags=c.flags, lambda8=lambda8, mode_bits=mode_bits, strong=c.strong, chroma=c.chroma,
                  with_reference=with_reference, recon_init=init)
    return dict(yuv=build(c.depth, c.kind, c.level if c.kind == "edge_clip" else 0), w64=w64, h64=h64, qp=qp, qp_c=(qpc, qpc), lambda8=lambda8, mode_bits=mode_bits,
                init=init, e=e)


# ---------------------------------------------------------------------------------------------------------------- the lists the tests run
DEPTHS = (8, 10, 12)

# the edge filter's clip (levels 0 and 1: modes 10 / 26 are filtered for n <= 16 only), reconstructions at the range limits, coded chroma
EDGE_CLIP_CASES = [case("edge_clip", p, d, l) for p in ("mid", "low-lambda") for d in DEPTHS for l in (0, 1)]
CLIPPING_CASES = (EDGE_CLIP_CASES
                  + [case("edges", "mid", d, l) for d in (8, 10) for l in (0, 1, 2)]
                  + [case("edges", "mid", 8, 1, sign_hide=False), case("edges", "mid", 10, 0, sign_hide=False)]
                  + [case("noise", "mid", 12, l) for l in (0, 2)]
                  + [case("edges", "mid", 8, 2, strong=False)])
# both ends of the QP range
QP_MAX_CASES = [case(k, "qp-max", d, l) for k in ("edges", "flat_hi", "flat_lo") for d in DEPTHS for l in (0, 1, 2)]
QP_MIN_CASES = ([case("edges", "qp-min", 8, 0), case("noise", "qp-min", 8, 2), case("edges", "qp-min", 10, 1), case("noise", "qp-min", 10, 0)]
                + [case(k, "qp-min", 12, l) for k in ("edges", "noise") for l in (1, 2)])
QP_END_CASES = QP_MAX_CASES + QP_MIN_CASES
# ties between modes: the winner is the first in the order DC, planar, 2 .. 34
TIE_CASES = ([case("halves", p, d, l) for p in ("mpm-ties-336", "mpm-ties-632") for d in (8, 10) for l in (0, 1, 2)]
             + [case("flat_hi", "lambda-0", 8, 1), case("flat_hi", "lambda-0", 10, 0)])
# bits * lambda8 = 2^36
COST_CASES = [case("edges", "big-cost", d, l) for d in (8, 12) for l in (0, 2)] + [case("edges", "big-cost-mpm", 10, 1)]
# the arm of the kernel without chroma planes
LUMA_ONLY_CASES = [case("edges", "mid", 8, 1, chroma=False), case("edges", "mid", 10, 2, chroma=False)]
ALL_CASES = sorted(set(CLIPPING_CASES + QP_END_CASES + TIE_CASES + COST_CASES + LUMA_ONLY_CASES))


# ---------------------------------------------------------------------------------------------------------------- the map at the range ends
def range_end_map(depth, level, width=WIDTH, height=HEIGHT):
    """(tu_qp int8 [3, h/8, w/8], lambda8_by_qp uint32 [52 + 6 (depth - 8)]) for the map test: every block's three quantiser QPs drawn from
    {0, 1, max - 1, max, two values in the middle} and from the int8 entries outside the range (-128, -1 code like 0; 127, and at 8 bits
    max + 1, like max); the lambda table has one entry above 2^24 (priced like 2^24) and 0."""
    qmax = 51 + 6 * (depth - 8)
    values = [0, 1, qmax - 1, qmax, 22 + 3 * (depth - 8), 34 + 6 * (depth - 8), -128, 127, -1] + ([qmax + 1] if qmax + 1 < 127 else [])
    nb = (width // 64) * (height // 64) * (64 >> (2 * level))
    rng = np.random.default_rng([43, depth, level])
    tu = np.stack([QE.cells_of_blocks(np.asarray(values, np.int64)[rng.permutation(np.arange(nb) % len(values))], width, height, level) for _ in range(3)])
    lam = QE.lambda8_table(depth).copy()
    lam[qmax] = (1 << 24) + 12345            # clamped to 2^24 by the kernel
    lam[1] = 0
    return tu, lam, values
