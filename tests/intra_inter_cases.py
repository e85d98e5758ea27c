"""Deterministic (reference, current) picture pairs, vectors and operating points for the intra-in-inter stages (numpy and the oracle only,
no torch).  192x128 = 3x2 CTUs: CTU (2, 0) and CTU (0, 1) share a wave, and the above-right arm of CTU (0, 1) / (1, 1) comes from another CTU.

  split      the current picture is a sub-pel-shifted copy of a noisy reference on one side of a boundary that runs through CTUs (x = 80 / 48 in the
             upper CTU row, x = 112 in the last 32 rows) and along CTU edges (y = 64, x = 128) - inter wins there, intra cannot predict noise - and
             ramps, bars and flat areas the reference does not have on the other side, where intra wins
  swapped    the same with the two sides exchanged: intra blocks left of / above inter ones
  all_new    new content everywhere
  shift      the shifted copy everywhere

tests/test_intra_inter_cpu.py asserts with the walk alone what the pictures reach; tests/test_gpu_intra_inter.py feeds the same cases to
the kernels."""
import collections
import functools

import numpy as np

import intra_cases as IC
import intra_expect as IE
import intra_inter_expect as IX
import qp_map_expect as QE

F, H = IE.F, IE.H
WIDTH, HEIGHT = 192, 128
KINDS = ("split", "swapped", "all_new", "shift")
SHIFTS = {"split": (6, -3), "swapped": (-5, 8), "all_new": (0, 0), "shift": (9, 2)}          # quarter samples: the shifted side's true vector
PAD = 16                                                                                 # samples of field beyond the picture on every side


def _field(rng, h, w, cutoff):
    """Band-limited noise of unit variance on an h x w grid: white noise with every frequency above `cutoff` cycles per sample removed."""
    f = np.fft.fft2(rng.normal(0, 1, (h, w)))
    fy, fx = np.abs(np.fft.fftfreq(h))[:, None], np.abs(np.fft.fftfreq(w))[None, :]
    f[(fy > cutoff) | (fx > cutoff)] = 0
    out = np.fft.ifft2(f).real
    return out / out.std()


def _new_content(yy, xx, block):
    """Ramps, bars and flat areas by `block` x `block` cell, in 8-bit units."""
    kind = ((xx // block) + 3 * (yy // block)) % 4
    ramp = 60 + 1.5 * (xx % block) + 2.0 * (yy % block)
    bars_v = np.where((xx // 4) % 2 == 0, 200.0, 70.0)
    bars_h = np.where((yy // 4) % 2 == 0, 40.0, 170.0)
    flat = 90.0 + 20 * (((xx // block) + (yy // block)) % 5)
    return np.select([kind == 0, kind == 1, kind == 2], [ramp, bars_v, bars_h], flat)


def new_side(kind, yy, xx):
    """Where the current picture shows content the reference lacks (luma coordinates)."""
    m = np.where(yy < 64, xx >= 80 - 32 * ((yy // 32) % 2), xx >= 128 - 16 * ((yy // 32) % 2))
    return {"split": m, "swapped": ~m, "all_new": np.ones_like(m), "shift": np.zeros_like(m)}[kind]


@functools.lru_cache(maxsize=None)
def pictures(kind, depth):
    """((Y, Cb, Cr) reference, (Y, Cb, Cr) current) of WIDTH x HEIGHT."""
    rng = np.random.default_rng([211, KINDS.index(kind)])
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    px, py = SHIFTS[kind]

    def q(a):
        return np.clip(np.rint(a * sc), 0, mx).astype(dt)
    # luma on a grid of quarter samples, chroma (4:2:0) on a grid of eighth samples: the same sub-sample shift of both
    fy = 128 + 42 * _field(rng, 4 * (HEIGHT + 2 * PAD), 4 * (WIDTH + 2 * PAD), 0.085)
    fc = [128 + 30 * _field(rng, 8 * (HEIGHT // 2 + PAD), 8 * (WIDTH // 2 + PAD), 0.04) for _ in range(2)]
    yy, xx = np.mgrid[0:HEIGHT, 0:WIDTH]
    ref_y = fy[4 * (yy + PAD), 4 * (xx + PAD)]
    cur_y = np.where(new_side(kind, yy, xx), _new_content(yy, xx, 64), fy[4 * (yy + PAD) + py, 4 * (xx + PAD) + px])
    cy, cx = np.mgrid[0:HEIGHT // 2, 0:WIDTH // 2]
    new_c = new_side(kind, 2 * cy, 2 * cx)
    ref, cur = [q(ref_y)], [q(cur_y)]
    for i in range(2):
        ref.append(q(fc[i][8 * (cy + PAD // 2), 8 * (cx + PAD // 2)]))
        cur.append(q(np.where(new_c, (100.0, 150.0)[i] + 0.25 * _new_content(2 * cy, 2 * cx, 64) * (1 - 2 * i),
                              fc[i][8 * (cy + PAD // 2) + py, 8 * (cx + PAD // 2) + px])))
    return tuple(ref), tuple(cur)


def vectors(kind, level):
    """One quarter-sample vector per block (index = ctu * blocks + z): the true shift on the shifted side, elsewhere vectors that walk
    through all 16 phases and reach up to 50 samples, into the extended border."""
    n = 8 << level
    nblk = (64 // n) ** 2
    cw = WIDTH // 64
    out = []
    for b in range((WIDTH // 64) * (HEIGHT // 64) * nblk):
        ctu, z = divmod(b, nblk)
        bx, by = IE.zorder(z)
        gx, gy = (ctu % cw) * 64 + bx * n, (ctu // cw) * 64 + by * n
        if new_side(kind, np.array(gy + n // 2), np.array(gx + n // 2)):
            far = 4 * ((b * 7) % 51) * (1 if b % 2 else -1)
            out.append((far + b % 4, -far // 2 + (b // 4) % 4))
        else:
            out.append(SHIFTS[kind])
    return out


Case = collections.namedtuple("Case", "id kind depth level point flags chroma ties maps")


def _case(kind, depth, level, point="mid", sign_hide=True, chroma=True, ties=False, maps=None):
    name = f"{kind}-d{depth}-l{level}-{point}" + ("" if sign_hide else "-nosh") + ("" if chroma else "-luma") + ("-ties" if ties else "") + (f"-{maps}" if maps else "")
    return Case(name, kind, depth, level, point, H.TU_SIGN_HIDE if sign_hide else 0, chroma, ties, maps)


# the mid QP with sign hiding on and off on the two split pictures at every level (the coverage the CPU test asserts), 10 and 12 bits
MID_CASES = [_case(k, 8, l, sign_hide=sh) for k in ("split", "swapped") for l in (0, 1, 2) for sh in (True, False)] + \
            [_case("split", 10, 1), _case("swapped", 10, 2), _case("split", 12, 1, sign_hide=False)]
WHOLE_CASES = [_case("all_new", 8, 1), _case("shift", 8, 1), _case("all_new", 10, 2), _case("shift", 10, 0)]
QP_END_CASES = [_case("split", 8, 1, "qp-min"), _case("swapped", 8, 2, "qp-max"), _case("split", 10, 0, "qp-max"), _case("swapped", 12, 1, "qp-min")]
TIE_CASES = [_case(k, 8, l, ties=True) for k in ("split", "swapped") for l in (0, 1, 2)] + [_case("swapped", 10, 1, ties=True)]
MAP_CASES = [_case("split", 8, 1, maps="map"), _case("swapped", 8, 2, maps="map-lambda"), _case("split", 10, 0, maps="map-lambda")]
LUMA_ONLY_CASES = [_case("split", 8, 1, chroma=False), _case("swapped", 10, 2, chroma=False)]
ALL_CASES = MID_CASES + WHOLE_CASES + QP_END_CASES + TIE_CASES + MAP_CASES + LUMA_ONLY_CASES


def tu_qp_map(depth, level):
    """tu_qp int8 [3, h/8, w/8] with both ends of the range, their neighbours and mid values dealt over the blocks, entries outside the
    range included (the stages clamp them)."""
    qmax = 51 + 6 * (depth - 8)
    vals = np.array([0, qmax, 1, qmax - 1, 30 + 6 * (depth - 8), 24 + 6 * (depth - 8), -3, min(qmax + 5, 127)], np.int64)
    n8 = 1 << level
    by, bx = np.mgrid[0:HEIGHT // 8, 0:WIDTH // 8]
    idx = (bx // n8) * 3 + (by // n8) * 5
    return np.stack([vals[(idx + c) % len(vals)] for c in range(3)]).astype(np.int8)


def padded(yuv):
    return IE.padded_planes(yuv)[0]


@functools.lru_cache(maxsize=None)
def inter_expectation(c):
    """The inter side of a case and everything the walk and the kernels are fed: shared, never modified."""
    ref, cur = pictures(c.kind, c.depth)
    pr, pc = padded(ref), padded(cur)
    w64, h64 = WIDTH, HEIGHT
    qp, lambda8, mode_bits = IC.point(c.point, c.depth)
    qpc = IC.chroma_qp(qp, c.depth)
    nctu = (w64 // 64) * (h64 // 64)
    mv = IX.mv_records(vectors(c.kind, c.level), c.level, nctu)
    tu_qp = tu_qp_map(c.depth, c.level) if c.maps else None
    lam_tab = QE.lambda8_table(c.depth) if c.maps == "map-lambda" else None
    table = IX.s_bitsizes(4 * 57 + 4)
    it = IX.inter_side(c.depth, pc, pr, w64, h64, c.level, mv, qp, (qpc, qpc), c.flags, chroma=c.chroma, tu_qp=tu_qp, lambda8=lambda8, lambda8_by_qp=lam_tab,
                       table=table)
    return dict(ref=ref, cur=cur, pref=pr, pcur=pc, w64=w64, h64=h64, qp=qp, qp_c=(qpc, qpc), lambda8=lambda8, mode_bits=mode_bits, mv=mv, tu_qp=tu_qp,
                lambda8_by_qp=lam_tab, table=table, inter=it)


def run_walk(c, mutation=None, inter_cost=None, with_reference=False):
    x = inter_expectation(c)
    return IX.walk(c.depth, x["pcur"], x["w64"], x["h64"], c.level, x["qp"], x["inter"], qp_c=x["qp_c"], flags=c.flags, lambda8=x["lambda8"],
                   mode_bits=x["mode_bits"], chroma=c.chroma, tu_qp=x["tu_qp"], lambda8_by_qp=x["lambda8_by_qp"], inter_cost=inter_cost,
                   cost_fn=IX.tie_pattern if (c.ties and inter_cost is None) else None, mutation=mutation, with_reference=with_reference)


@functools.lru_cache(maxsize=None)
def expectation(c):
    """inter_expectation(c) plus e = the walk's result."""
    x = dict(inter_expectation(c))
    x["e"] = run_walk(c)
    return x
