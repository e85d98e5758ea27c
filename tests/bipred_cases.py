"""Deterministic two-reference inputs for the bi-predictive and chroma stage tests (numpy and the oracle only, no torch): `edges` pictures
(tests/subpel_cases.py) whose 8-tap and 4-tap filters overshoot at both ends in BOTH lists, a current picture planted so that every outcome
of the bidirectional decision occurs at vectors anywhere in a +-57 window, and both lists' integer-stage records written directly.

tests/test_bipred_cases_cpu.py asserts, with the oracle alone, that every case below really reaches what it is listed for - and holds the
plain restatement of the prediction the clip conditions are measured on; tests/test_gpu_recon.py, test_gpu_bidir.py and test_gpu_bpicture.py
feed the same cases to the kernels."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np

import subpel_cases as SC
from subpel_cases import edges_picture, oracle, pu_list, unpack_q          # noqa: F401  (re-exported for the tests)

F = importlib.import_module("x265-yuuki-asuna_amd.frames")

KINDS = ("edges", "edges_shared", "inverse")
PLANTINGS = ("list0", "list1", "average", "zero_average", "identical", "both_exact", "tie")
LEVEL_BASE = (0, 64, 80)
RARE_PHASES = [(a, b) for a in range(8) for b in range(8) if not (a & 3) or not (b & 3) or (a & b & 1)]


def _draw_vector(rng, R, one_list=False):
    """subpel_cases' draw: the integer part uniform over the window, for a third pinned to +-R on one or both axes; the fraction in -3 .. 3
    (a fifth of the vectors are integer), pointing back into the window where the integer part is pinned.  one_list: the vector of a quadrant
    that one list predicts alone - never integer by draw and mostly fractional on both axes: the integer copies among the one-list blocks
    are planting 5's, and the share of clipped samples is counted over all of them."""
    I = rng.integers(-R, R + 1, size=2)
    if rng.random() < 1 / 3:
        axes = int(rng.integers(1, 4))
        for a in (0, 1):
            if (axes >> a) & 1:
                I[a] = R if rng.random() < 0.5 else -R
    f = np.zeros(2, np.int64) if rng.random() < 0.2 else rng.integers(-3, 4, size=2)
    if one_list:
        f = rng.integers(1, 4, size=2) * rng.choice((-1, 1), size=2) if rng.random() < 0.7 else rng.integers(-3, 4, size=2)
    return I, np.where(np.abs(I) == R, -np.sign(I) * np.abs(f), f)


def _satd8x4(d):
    """SATD of an 8-wide, 4-high difference block: the two 4 x 4 Hadamard sums, halved together."""
    H = np.array([[1, 1, 1, 1], [1, 1, -1, -1], [1, -1, -1, 1], [1, -1, 1, -1]], np.int64)
    return int(sum(np.abs(H @ d[:, k:k + 4] @ H).sum() for k in (0, 4)) >> 1)


def _plant_tie(R, depth, width, ref0, ref1, plant, locked, quad_i):
    """Planting 6 (see build_bi): turns one planting-5 quadrant into the tie quadrant, writes both references and locks reference 1's part."""
    cq, qoff = F.qpel_cost_table(R)
    cq = cq.astype(np.int64)
    level = [a for a in range(40, R - 1) if all(cq[qoff + s * 4 * a + k] == cq[qoff + 4 * a] for s in (-1, 1) for k in range(-4, 5))]
    maxv = (1 << depth) - 1
    v, e = maxv // 2, maxv // 6
    for gy, gx in zip(*np.nonzero(plant == 5)):
        y0, x0 = gy * 32, gx * 32
        for a0 in level:
            for a1 in level:
                D = int(cq[qoff + 4 * a0] + cq[qoff + 4 * a1] - 2 * cq[qoff])          # the mv cost the zero candidate saves
                for s0, s1 in ((1, -1), (-1, 1), (1, 1), (-1, -1)):
                    t0, t1 = x0 + s0 * a0, x0 + s1 * a1
                    if D % 4 or D < 12 or min(t0, t1) < 0 or max(t0, t1) > width - 32 or t0 == t1:        # t0 == t1: same sign and a0 == a1
                        continue
                    if any(plant[gy, g] == 4 for g in range(t1 // 32, (t1 + 31) // 32 + 1)):
                        continue
                    pat = np.zeros((4, 8), np.int64)
                    if D % 8 == 0:
                        pat[0, 0] = D // 8
                    else:
                        pat[0, :3], pat[0, 4] = 1, (D - 12) // 8
                    assert _satd8x4(pat) == D and v + pat.max() <= maxv
                    ref0[y0:y0 + 32, t0:t0 + 32], ref1[y0:y0 + 32, t1:t1 + 32] = v + e, v - e
                    for r in (ref0, ref1):
                        r[y0:y0 + 32, x0:x0 + 32] = v
                        r[y0:y0 + 4, x0:x0 + 8] += pat.astype(r.dtype)
                    locked[y0:y0 + 32, x0:x0 + 32] = locked[y0:y0 + 32, t1:t1 + 32] = True
                    plant[gy, gx] = 6
                    quad_i[0, gy, gx], quad_i[1, gy, gx] = (s0 * a0, 0), (s1 * a1, 0)
                    return
    raise AssertionError("no room for the tie quadrant: another seed")


@functools.lru_cache(maxsize=None)
def build_bi(depth, width, height, R, kind, seed):
    """The padded current plane `cur` and the two padded reference planes `refs` (frames.pad_plane geometry), both lists' integer-stage records
    `best` (uint64 [nctu * 85] each, cost << 32 | (my + R) * (2R + 1) + (mx + R), as subpel_cases.build packs them), the planted integer vector
    of every record per list (`imv`), the planting of every 32 x 32 quadrant (`plant`, index into PLANTINGS) and three Y / Cb / Cr pictures
    `yuv` = (list 0, current, list 1) with chroma at half size.  The result is shared between tests: read only.

    kind "edges": both references are edges_picture with independent draws; "edges_shared": reference 1 is reference 0 with half of its
    samples redrawn (more samples where both predictions overshoot the same way); "inverse": "edges" with the current picture's samples
    replaced by max - sample in every second quadrant of each of the first four plantings (|difference| up to max at every candidate: the
    width of the SATD sums; the other quadrants keep every outcome of the decision present).

    Each 32 x 32 quadrant of the current picture is one of seven plantings, the first six dealt round robin over a shuffled quadrant order:
    0 list0         list 0's fractional samples at a far vector 4 I + f (from oracle_api.phase_planes; half of them + -2 .. 2 LSB of noise); list 1's
                    records are unrelated vectors of the window - one per PU - carrying their true SAD + mv cost
    1 list1         the mirror image
    2 average       pixelavg (a + b + 1) >> 1 of both lists' fractional samples at independent far vectors that walk RARE_PHASES: only
                    the average matches
    3 zero_average  pixelavg of both references at zero displacement under unrelated non-zero records for both lists: the zero candidate wins
    4 identical     reference 1 is made a copy of reference 0 over the quadrant and the current picture copies both: both records are the zero
                    vector with cost key 0 - the zero candidate is not tried and c0 == c1
    5 both_exact    an exact copy of list 0 at an integer displacement, from a region that reference 1 holds too at another displacement: zero
                    cost keys with non-zero vectors in both lists
    6 tie           one quadrant (taken from planting 5's share): the current block is constant v, list 0 holds v + e and list 1 holds v - e at far
                    horizontal displacements chosen where the mv cost table is level (no refinement moves them, at any subme), so only their
                    average matches; both references hold v at the block's own place, plus a few raised samples in its first 8 x 8 block whose
                    SATD equals the mv cost the zero candidate saves: the 8 x 8, 16 x 16 and 32 x 32 blocks that hold them have cz == cRef
                    exactly, and the refined vectors must stay (the comparison is strict)
    The 64 x 64 PU (not part of the decision) takes its first quadrant's vectors.

    Chroma: every plane is an edges_picture of its own draw at half size and nothing is planted - every chroma block is coded against a
    mismatching prediction."""
    assert kind in KINDS and width % 64 == 0 and height % 64 == 0
    assert R + 2 + 8 <= min(F.MARGIN_X, F.MARGIN_Y)          # phase planes are specified 8 samples in from the buffer edge; drift <= 2 samples
    assert (4 * R + 8) / 8 + 2 <= min(F.CHROMA_MARGIN_X, F.CHROMA_MARGIN_Y)          # a luma component of 4R + 8 quarter samples is 29.5 chroma samples + 2 taps
    rng = np.random.default_rng([seed, depth, R, KINDS.index(kind), 2])
    maxv = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    ref0 = edges_picture(rng, width, height, maxv, dt)
    ref1 = edges_picture(rng, width, height, maxv, dt)
    if kind == "edges_shared":
        ref1 = np.where(rng.random((height, width)) < 0.5, ref0, ref1).astype(dt)
    qw, qh, cw = width // 32, height // 32, width // 64
    order = rng.permutation(qw * qh)
    plant = np.zeros(qw * qh, np.int64)
    plant[order] = np.arange(qw * qh) % 6
    nth = np.zeros(qw * qh, np.int64)                          # the quadrant's number among those of its planting
    nth[order] = np.arange(qw * qh) // 6
    plant, nth = plant.reshape(qh, qw), nth.reshape(qh, qw)

    # reference 1 first: the regions it shares with reference 0 (plantings 4 and 5), none of them written twice
    locked = np.zeros((height, width), bool)
    quad_i = np.zeros((2, qh, qw, 2), np.int64)
    quad_f = np.zeros((2, qh, qw, 2), np.int64)
    _plant_tie(R, depth, width, ref0, ref1, plant, locked, quad_i)
    for gy, gx in zip(*np.nonzero(plant == 4)):
        y0, x0 = gy * 32, gx * 32
        ref1[y0:y0 + 32, x0:x0 + 32] = ref0[y0:y0 + 32, x0:x0 + 32]
        locked[y0:y0 + 32, x0:x0 + 32] = True

    def inside(y0, x0):                                         # a non-zero displacement of the window that keeps the block inside the picture
        while True:
            I = rng.integers(-R, R + 1, size=2)
            if I.all() and 0 <= x0 + I[0] <= width - 32 and 0 <= y0 + I[1] <= height - 32:
                return I
    for gy, gx in zip(*np.nonzero(plant == 5)):
        y0, x0 = gy * 32, gx * 32
        I0 = inside(y0, x0)
        ii = np.pad(locked.cumsum(axis=0).cumsum(axis=1), ((1, 0), (1, 0)))
        free = [(ix, iy) for iy in range(max(-R, -y0), min(R, height - 32 - y0) + 1) for ix in range(max(-R, -x0), min(R, width - 32 - x0) + 1)
                if (ix or iy) and (ix, iy) != tuple(I0)
                and ii[y0 + iy + 32, x0 + ix + 32] - ii[y0 + iy, x0 + ix + 32] - ii[y0 + iy + 32, x0 + ix] + ii[y0 + iy, x0 + ix] == 0]
        assert free, "no room in reference 1 for this quadrant's second copy: another seed"
        I1 = np.array(free[int(rng.integers(len(free)))], np.int64)
        ty, tx = y0 + I1[1], x0 + I1[0]
        ref1[ty:ty + 32, tx:tx + 32] = ref0[y0 + I0[1]:y0 + I0[1] + 32, x0 + I0[0]:x0 + I0[0] + 32]
        locked[ty:ty + 32, tx:tx + 32] = True
        quad_i[0, gy, gx], quad_i[1, gy, gx] = I0, I1
    pads = [F.pad_plane(r) for r in (ref0, ref1)]
    _, stride, org, w64, h64 = pads[0]
    rbuf = [p[0] for p in pads]
    planes = []
    for rb in rbuf:
        ph = oracle().phase_planes(depth, rb.reshape(-1), stride, rb.shape[0])
        planes.append([rb] + [ph[k] for k in range(15)])          # index yf * 4 + xf

    def frac_block(l, y0, x0, q):
        pl = planes[l][int(q[1] & 3) * 4 + int(q[0] & 3)]
        sy, sx = F.MARGIN_Y + y0 + int(q[1] >> 2), F.MARGIN_X + x0 + int(q[0] >> 2)
        return pl[sy:sy + 32, sx:sx + 32].astype(np.int64)
    cur_img = np.zeros((height, width), np.int64)
    walk = 0 if width > 256 else 40
    for gy in range(qh):
        for gx in range(qw):
            y0, x0, p = gy * 32, gx * 32, int(plant[gy, gx])
            if p <= 2:
                for l in ((0,), (1,), (0, 1))[p]:
                    I, f = _draw_vector(rng, R, p < 2)
                    if p == 2:
                        # the refinement seldom ends on an integer position of one axis or on a quarter position of both: the vectors of the `average`
                        # quadrants walk those 44 of the 64 eighth-sample chroma phases (parity of the integer part x quarter 0 .. 3)
                        t = RARE_PHASES[walk % len(RARE_PHASES)]
                        walk += 1
                        for a in (0, 1):
                            I[a] += (I[a] & 1) != (t[a] >> 2)
                            I[a] -= 2 * (I[a] >= R)
                            f[a] = t[a] & 3
                    quad_i[l, gy, gx], quad_f[l, gy, gx] = I, f
                blks = [frac_block(l, y0, x0, 4 * quad_i[l, gy, gx] + quad_f[l, gy, gx]) for l in ((0,), (1,), (0, 1))[p]]
                blk = blks[0] if p < 2 else (blks[0] + blks[1] + 1) >> 1
                if p < 2 and rng.random() < 0.5:
                    blk = np.clip(blk + rng.integers(-2, 3, size=blk.shape), 0, maxv)
            elif p == 6:
                blk = np.full((32, 32), maxv // 2, np.int64)
            elif p == 3:
                blk = (frac_block(0, y0, x0, np.zeros(2, np.int64)) + frac_block(1, y0, x0, np.zeros(2, np.int64)) + 1) >> 1
            else:
                blk = frac_block(0, y0, x0, 4 * quad_i[0, gy, gx])
            if kind == "inverse" and p <= 3 and nth[gy, gx] % 2 == 1:
                blk = maxv - blk
            cur_img[y0:y0 + 32, x0:x0 + 32] = blk
    cur_img = cur_img.astype(dt)
    cbuf = F.pad_plane(cur_img)[0]

    # both lists' integer-stage records
    cost_t = F.mv_cost_table(R).astype(np.int64)
    NC = 2 * R + 1
    pus = pu_list(w64, h64)
    c64 = cur_img.astype(np.int64)
    best, imv = [], []
    for l in (0, 1):
        r64 = rbuf[l].astype(np.int64)
        b, v_of = np.zeros(len(pus), np.uint64), np.zeros((len(pus), 2), np.int32)
        for i, (ctu, lv, z, px, py, n) in enumerate(pus):
            gy, gx = py // 32, px // 32
            p = int(plant[gy, gx])
            if p == 3 or p == 1 - l:                            # unrelated: a non-zero vector of this PU's own
                v = np.zeros(2, np.int64)
                while not v.any():
                    v = _draw_vector(rng, R)[0]
            else:
                v = quad_i[l, gy, gx]
            ry, rx = F.MARGIN_Y + py + int(v[1]), F.MARGIN_X + px + int(v[0])
            s = int(np.abs(c64[py:py + n, px:px + n] - r64[ry:ry + n, rx:rx + n]).sum())
            cost = s + int(cost_t[v[0] + R] + cost_t[v[1] + R]) if s else 0
            b[i] = (cost << 32) | int((v[1] + R) * NC + v[0] + R)
            v_of[i] = v
        best.append(b)
        imv.append(v_of)

    # the three pictures of the B step: chroma of its own draws
    cw2, ch2 = width // 2, height // 2
    yuv = tuple((y,) + tuple(edges_picture(rng, cw2, ch2, maxv, dt) for _ in range(2)) for y in (ref0, cur_img, ref1))
    cbufs = [[F.pad_chroma(pic[c], w64, h64)[0] for c in (1, 2)] for pic in yuv]          # [picture][plane]
    stride_c = w64 // 2 + 2 * F.CHROMA_MARGIN_X
    org_c = F.CHROMA_MARGIN_Y * stride_c + F.CHROMA_MARGIN_X
    for a in [cbuf, cur_img, plant, quad_i, quad_f] + rbuf + best + imv + [p for pic in yuv for p in pic] + [p for pic in cbufs for p in pic]:
        a.setflags(write=False)
    return SimpleNamespace(depth=depth, R=R, kind=kind, cur=cbuf, refs=tuple(rbuf), cur_img=cur_img, ref_imgs=(ref0, ref1), stride=stride, org=org, w64=w64,
                           h64=h64, nctu=len(pus) // 85, best=tuple(best), imv=tuple(imv), plant=plant, quad_i=quad_i, quad_f=quad_f, yuv=yuv,
                           cur_c=tuple(cbufs[1]), refs_c=(tuple(cbufs[0]), tuple(cbufs[2])), stride_c=stride_c, org_c=org_c)


class BiCase(tuple):
    """(depth, width, height, R, kind, seed, subme); .build = the builder's arguments."""
    depth, width, height, R, kind, seed, subme = (property(lambda s, k=k: s[k]) for k in range(7))
    build = property(lambda s: tuple(s[:6]))
    id = property(lambda s: f"{s.kind}-d{s.depth}-{s.width}x{s.height}-R{s.R}-seed{s.seed}-subme{s.subme}")


@functools.lru_cache(maxsize=None)
def refined_bi(case):
    """The oracle's refinement of both lists' records: two int32 [nctu * 85, 2] = {cost, qx | qy << 16} (shared: read only)."""
    c = build_bi(*case.build)
    cq, qoff = F.qpel_cost_table(c.R)
    out = []
    for l in (0, 1):
        o = oracle().subpel_refine(c.depth, c.cur, c.stride, c.org, c.refs[l], c.stride, c.org, c.w64, c.h64, c.R, 0, c.nctu, c.best[l], cq, qoff, case.subme)
        o.setflags(write=False)
        out.append(o)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _phases(build):
    import bidir_expect as BE
    c = build_bi(*build)
    return tuple(BE.phases_of(c.depth, r, c.stride) for r in c.refs)


@functools.lru_cache(maxsize=None)
def decided(case, level, with_reference=False):
    """tests/bidir_expect.expect on the case's refined records (shared: read only)."""
    import bidir_expect as BE
    c = build_bi(*case.build)
    cq, qoff = F.qpel_cost_table(c.R)
    return BE.expect(c.depth, c.cur, c.stride, c.org, c.w64, c.h64, level, refined_bi(case), _phases(case.build), cq, qoff, with_reference=with_reference)


def dir_flags(case, level):
    """The prediction direction of every block of `level` the recon tests feed: the decision's own, which holds all three directions on
    every case below (a case where it did not would get another seed)."""
    d = decided(case, level)["dir"]
    assert all((d == k).any() for k in (1, 2, 3)), f"{case.id} level {level}: the decision lacks a direction"
    return d


def level_records(rec, level, nctu):
    """The records of one level, in block order: [nctu * nb, 2]."""
    nb = (64 >> (3 + level)) ** 2
    return rec.reshape(nctu, 85, 2)[:, LEVEL_BASE[level]:LEVEL_BASE[level] + nb].reshape(-1, 2)


def _bi(depth, kind, seed, subme=7, width=256, height=128):
    return BiCase((depth, width, height, 57, kind, seed, subme))


# x265hip_bidir_decide on the oracle's refined records: (case, level, phase planes?).  Every depth at every level, subme 2 and 3, interpolating and
# from phase planes; 384 x 320 = 30 CTUs: xcd_swizzle is not the identity and leaves a tail of 6.
BIDIR_CASES = [(_bi(8, "edges", 1, 3), 0, False), (_bi(8, "edges", 1, 3), 1, True), (_bi(8, "edges_shared", 1, 2), 2, False),
               (_bi(10, "edges", 1, 2), 0, True), (_bi(10, "edges_shared", 1, 3), 1, False), (_bi(10, "inverse", 1, 3), 2, True),
               (_bi(12, "inverse", 1, 3), 0, False), (_bi(12, "edges", 1, 2), 1, True), (_bi(12, "inverse", 1, 3), 2, True),
               (_bi(8, "edges", 1, 3, 384, 320), 2, True), (_bi(8, "edges", 1, 3, 384, 320), 0, False)]

# stages.InterReconBi on the refined vectors of both lists with the decision's directions: (case, level, qp, TU flags); 2 = sign hiding.  QPs are chosen
# so that the oracle codes at least 30 % of the blocks and its reconstruction clips at both ends.
RECON_BI_CASES = [(_bi(8, "edges", 2), 0, 28, 0), (_bi(8, "edges_shared", 1), 1, 30, 2), (_bi(8, "inverse", 1), 2, 40, 0),
                  (_bi(10, "edges", 1), 0, 34, 2), (_bi(10, "edges_shared", 2), 1, 40, 0), (_bi(10, "edges", 1), 2, 40, 2),
                  (_bi(12, "edges_shared", 1), 0, 40, 0), (_bi(12, "inverse", 1), 1, 70, 2), (_bi(12, "edges_shared", 1), 2, 50, 0)]

# Explicit weight tables (present, weight, offset, log2_denom) of the two lists.  Every pair has gain above 1 on the weighted paths (w0 + w1 > 2 ^ (denom + 1)
# for addWeightBi, w > 2 ^ denom for addWeightUni) and negative offsets, so both ends of both clips are met; B, C, D have wtPresent on one list only
# (D: list 1 has no table at all, so blocks of both lists take addAvg).
WEIGHTS = {"A": ((1, 80, -20, 6), (1, 70, -10, 6)), "B": ((1, 90, -40, 6), (0, 64, 0, 6)), "C": ((0, 32, 0, 5), (1, 45, -25, 5)),
           "D": ((1, 127, -60, 6), None), "E": ((1, 37, -12, 5), (1, 40, -30, 5)), "F": ((1, 3, -5, 1), (1, 3, -9, 1))}
RECON_BI_WEIGHT_CASES = [(_bi(8, "edges_shared", 1), 2, 46, "A"), (_bi(8, "inverse", 1), 0, 40, "B"), (_bi(10, "edges_shared", 1), 1, 50, "C"),
                         (_bi(10, "edges_shared", 1), 2, 50, "D"), (_bi(12, "edges", 1), 0, 60, "E"), (_bi(12, "inverse", 1), 1, 72, "F")]

# The 8 x 8-level cases of 384 x 320 (120 quadrants) are there for the phases: a 256 x 128 input has too few vectors in blocks of both lists to meet
# all 64 chroma phases (tests/test_bipred_cases_cpu.py counts them per bit depth).
# stages.InterReconChromaBi, both planes (the second at qp - 1): (case, level, qp, weights or None).  Nothing matches in chroma, so every block is coded; only
# the coarsest quantisers push the reconstruction of a picture that is mostly 0 or max already to 0 and to max where the source is neither.
RECON_CHROMA_CASES = [(_bi(8, "edges", 1, 7, 384, 320), 0, 50, None), (_bi(8, "edges_shared", 1), 1, 50, "A"), (_bi(8, "edges", 1), 2, 50, "B"),
                      (_bi(10, "edges", 1), 1, 62, None), (_bi(10, "edges_shared", 1), 2, 62, "C"), (_bi(10, "edges", 1, 7, 384, 320), 0, 62, "D"),
                      (_bi(12, "edges", 1), 2, 74, None), (_bi(12, "edges_shared", 1, 7, 384, 320), 0, 74, "E"), (_bi(12, "edges", 1), 1, 74, "F")]

# stages.InterReconChroma on list 0 alone: (case, level, qp, TU flags)
RECON_CHROMA_UNI_CASES = [(_bi(8, "edges", 1), 0, 50, 0), (_bi(8, "edges", 1), 1, 50, 2), (_bi(8, "edges", 1), 2, 50, 0),
                          (_bi(10, "edges", 1), 0, 62, 2), (_bi(10, "edges", 1), 2, 62, 0), (_bi(12, "edges", 1), 1, 74, 2), (_bi(12, "edges", 1), 2, 74, 0)]

# stages.BFramePipeline on the case's three pictures: (case, level, phase planes in the sub-pel stage?)
B_STEP_CASES = [(_bi(8, "edges", 1, 3), 2, False), (_bi(10, "edges", 1, 3), 1, True)]
