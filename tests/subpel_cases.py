"""Deterministic inputs for the sub-pel stage tests (numpy and the oracle only, no torch): pictures whose 8-tap filters overshoot at
both ends, current pictures assembled from the reference's own fractional samples, and integer-stage records written directly -
any vector of the window, zero-cost keys included - instead of taken from the device's exhaustive search.

tests/test_subpel_cases_cpu.py asserts, with the oracle alone, that every case below really reaches what it is listed for;
tests/test_gpu_subpel.py, test_gpu_recon.py and test_gpu_search.py feed the same cases to the kernels."""
import functools
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

F = importlib.import_module("x265-yuuki-asuna_amd.frames")

KINDS = ("edges", "noise", "texture", "inverse", "flat_hi", "flat_lo")
LEVEL_SIZES = (8, 16, 32, 64)


def oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def zorder_xy(z):
    return (z & 1) | ((z >> 1) & 2) | ((z >> 2) & 4), ((z >> 1) & 1) | ((z >> 2) & 2) | ((z >> 3) & 4)


def pu_list(w64, h64):
    """(ctu, level, z, px, py, n) of every record, in record order ([ctu][85], levels in z-order)."""
    out = []
    cw = w64 // 64
    for ctu in range(cw * (h64 // 64)):
        for l, n in enumerate(LEVEL_SIZES):
            for z in range((64 // n) ** 2):
                bx, by = zorder_xy(z)
                out.append((ctu, l, z, (ctu % cw) * 64 + bx * n, (ctu // cw) * 64 + by * n, n))
    return out


def edges_picture(rng, width, height, maxv, dt):
    """2 x 3-sample cells (2 wide, 3 high) at 0 or max, about 35 % of the samples replaced by uniform full-range values."""
    cells = rng.integers(0, 2, size=((height + 2) // 3, (width + 1) // 2))
    img = np.repeat(np.repeat(cells, 3, axis=0), 2, axis=1)[:height, :width] * maxv
    repl = rng.random((height, width)) < 0.35
    return np.where(repl, rng.integers(0, maxv + 1, size=(height, width)), img).astype(dt)


@functools.lru_cache(maxsize=None)
def build(depth, width, height, R, kind, seed):
    """The padded current and reference planes (frames.pad_plane geometry), the uint64 [nctu * 85] integer-stage records
    (cost << 32 | (my + R) * (2R + 1) + (mx + R)) and the integer vector per PU.  The result is shared between tests: read only.

    Every 32 x 32 quadrant of the current picture is the reference displaced by a quarter-sample vector 4 * I + f of its own (samples
    taken from oracle_api.phase_planes): I uniform over the window, for a third of the quadrants pinned to +-R on one or both axes with
    f pointing back into the window; three quadrants in ten are exact copies at an integer displacement (SAD 0 for every PU inside),
    half of the others get +-2 LSB of noise.  In every fourth CTU the four quadrants share one vector, so the 64 x 64 PU has a true
    match too, and in every eighth that match is exact: a zero-cost key at the top level.  One quadrant is an exact copy of a constant patch
    a few samples away (see below).
    kind "inverse": the current picture is max - planted sample, except in half of the exact quadrants (the zero-cost keys stay) - the
    other half become exact inverses at an integer displacement, |difference| = |max - 2 s| at the record's vector.
    kinds "flat_hi" / "flat_lo": current all max against reference all 0 / the other way round - every candidate ties on distortion."""
    assert kind in KINDS and width % 64 == 0 and height % 64 == 0
    assert R + 2 + 8 <= min(F.MARGIN_X, F.MARGIN_Y)          # phase planes are specified 8 samples in from the buffer edge; drift <= 2 samples
    rng = np.random.default_rng([seed, depth, R, KINDS.index(kind)])
    maxv = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    if kind in ("edges", "inverse"):
        ref_img = edges_picture(rng, width, height, maxv, dt)
    elif kind == "noise":
        ref_img = rng.integers(0, maxv + 1, size=(height, width)).astype(dt)
    elif kind == "texture":
        ref_img = F.synth_clip(width, height, 1, depth=depth, seed=seed)[0][0]
    else:
        ref_img = np.full((height, width), 0 if kind == "flat_hi" else maxv, dt)
    flat = kind.startswith("flat")
    # The second quadrant row's first quadrant (CTU 0, z-order quadrant 2) is an exact copy, one to three samples away on each axis, of a constant
    # patch of the reference: zero-cost keys whose every candidate is free of distortion too - only the zero-residual shortcut keeps the mv
    # cost from pulling these vectors towards the origin.
    rng_p = np.random.default_rng([seed, depth, R, KINDS.index(kind), 1])
    patch_i = rng_p.integers(1, min(R, 3) + 1, size=2) * rng_p.choice((-1, 1), size=2)
    if not flat:
        ref_img = ref_img.copy()
        ref_img[32 - 8 + patch_i[1]:32 + 40 + patch_i[1], max(0, -8 + patch_i[0]):40 + patch_i[0]] = rng_p.integers(0, maxv + 1)
    rbuf, stride, org, w64, h64 = F.pad_plane(ref_img)
    planes = None
    if not flat:
        ph = oracle().phase_planes(depth, rbuf.reshape(-1), stride, rbuf.shape[0])
        planes = [rbuf] + [ph[k] for k in range(15)]          # index yf * 4 + xf

    # one displacement per quadrant
    qw, qh, cw = w64 // 32, h64 // 32, w64 // 64
    quad_i = np.zeros((qh, qw, 2), np.int64)
    quad_f = np.zeros((qh, qw, 2), np.int64)
    cur_img = np.zeros((h64, w64), np.int64)
    for ctu in range(cw * (h64 // 64)):
        shared = None
        for k in range(4):
            gy, gx = (ctu // cw) * 2 + (k >> 1), (ctu % cw) * 2 + (k & 1)
            I = rng.integers(-R, R + 1, size=2)
            if rng.random() < 1 / 3:
                axes = int(rng.integers(1, 4))
                for a in (0, 1):
                    if (axes >> a) & 1:
                        I[a] = R if rng.random() < 0.5 else -R
            exact = rng.random() < 0.3
            f = np.zeros(2, np.int64) if exact else rng.integers(-3, 4, size=2)
            noisy = (not exact) and rng.random() < 0.5
            keep = rng.random() < 0.5                           # "inverse": this exact quadrant stays a copy
            if ctu % 4 == 1:                                    # one vector for the whole CTU
                if k == 0:
                    if ctu % 8 == 1:
                        exact, f, noisy, keep = True, np.zeros(2, np.int64), False, True
                    shared = (I, exact, f, noisy, keep)
                I, exact, f, noisy, keep = shared
            if (ctu, k) == (0, 2) and not flat:
                I, exact, f, noisy, keep = patch_i, True, np.zeros(2, np.int64), False, True
            f = np.where(np.abs(I) == R, -np.sign(I) * np.abs(f), f)
            quad_i[gy, gx], quad_f[gy, gx] = I, f
            y0, x0 = gy * 32, gx * 32
            if flat:
                cur_img[y0:y0 + 32, x0:x0 + 32] = maxv if kind == "flat_hi" else 0
                continue
            q = 4 * I + f
            pl = planes[int(q[1] & 3) * 4 + int(q[0] & 3)]
            sy, sx = F.MARGIN_Y + y0 + int(q[1] >> 2), F.MARGIN_X + x0 + int(q[0] >> 2)
            blk = pl[sy:sy + 32, sx:sx + 32].astype(np.int64)
            if noisy:
                blk = np.clip(blk + rng.integers(-2, 3, size=blk.shape), 0, maxv)
            if kind == "inverse" and not (exact and keep):
                blk = maxv - blk
            cur_img[y0:y0 + 32, x0:x0 + 32] = blk
    cur_img = cur_img.astype(dt)
    cbuf = F.pad_plane(cur_img)[0]

    # the integer stage's records
    cost_t = F.mv_cost_table(R).astype(np.int64)
    NC = 2 * R + 1
    pus = pu_list(w64, h64)
    best = np.zeros(len(pus), np.uint64)
    imv = np.zeros((len(pus), 2), np.int32)
    r64 = rbuf.astype(np.int64)
    c64 = cur_img.astype(np.int64)

    def sad(px, py, n, v):
        ry, rx = F.MARGIN_Y + py + int(v[1]), F.MARGIN_X + px + int(v[0])
        return int(np.abs(c64[py:py + n, px:px + n] - r64[ry:ry + n, rx:rx + n]).sum())
    for i, (ctu, l, z, px, py, n) in enumerate(pus):
        v = quad_i[py // 32, px // 32].copy()                  # the 64 x 64 PU takes quadrant 0's
        s = sad(px, py, n, v)
        if s and rng.random() < 0.3:
            d = np.zeros(2, np.int64)
            while not d.any():
                d = rng.integers(-1, 2, size=2)
            v = np.clip(v + d, -R, R)
            s = sad(px, py, n, v)
        cost = s + int(cost_t[v[0] + R] + cost_t[v[1] + R]) if s else 0
        best[i] = (cost << 32) | int((v[1] + R) * NC + v[0] + R)
        imv[i] = v
    for a in (cbuf, rbuf, cur_img, ref_img, best, imv):
        a.setflags(write=False)
    return SimpleNamespace(depth=depth, R=R, kind=kind, cur=cbuf, ref=rbuf, cur_img=cur_img, ref_img=ref_img, stride=stride, org=org, w64=w64, h64=h64,
                           nctu=len(pus) // 85, best=best, imv=imv, planes=planes, quad_i=quad_i, quad_f=quad_f, patch_i=patch_i)


@functools.lru_cache(maxsize=None)
def refined(case):
    """The oracle's refinement of a case's records: int32 [nctu * 85, 2] = {cost, qx | qy << 16} (shared: read only)."""
    c = build(*case.build)
    cq, qoff = F.qpel_cost_table(c.R)
    out = oracle().subpel_refine(c.depth, c.cur, c.stride, c.org, c.ref, c.stride, c.org, c.w64, c.h64, c.R, 0, c.nctu, c.best, cq, qoff, case.subme)
    out.setflags(write=False)
    return out


def unpack_q(rec):
    """(qx, qy) of the {cost, qx | qy << 16} records."""
    w = rec[:, 1].astype(np.int64)
    return ((w & 0xffff) ^ 0x8000) - 0x8000, w >> 16


class Case(tuple):
    """(depth, width, height, R, kind, seed, subme); .build = the builder's arguments."""
    depth, width, height, R, kind, seed, subme = (property(lambda s, k=k: s[k]) for k in range(7))
    build = property(lambda s: tuple(s[:6]))
    id = property(lambda s: f"{s.kind}-d{s.depth}-{s.width}x{s.height}-R{s.R}-subme{s.subme}")


def _cases():
    out = []
    seed = {8: 1, 10: 2, 12: 3}
    for d in (8, 10, 12):                                      # R = 57: the reference's default merange, and as wide as the margins (96 / 80) allow
        out += [Case((d, 256, 128, 57, "edges", seed[d], s)) for s in (0, 1, 2, 3, 5, 7)]
        out += [Case((d, 256, 128, 57, k, seed[d], s)) for k in ("noise", "texture") for s in (3, 7)]
        out += [Case((d, 256, 128, 57, "inverse", seed[d], s)) for s in (2, 7)]
    out.append(Case((10, 256, 128, 13, "edges", 4, 7)))        # other NC; 13 is the 16-bit LDS-pitch step of the search tests
    out.append(Case((8, 256, 128, 8, "edges", 8, 3)))
    out.append(Case((8, 384, 320, 57, "edges", 6, 7)))         # 30 CTUs: xcd_swizzle is not the identity and leaves a tail of 6
    return out


PLANTED_CASES = _cases()
FLAT_CASES = [Case((d, 256, 128, 57, k, 7, s)) for d in (8, 10, 12) for k, s in (("flat_hi", 7), ("flat_lo", 3))]
STRIDE_CASES = [c for c in PLANTED_CASES if c.kind == "edges" and c.R == 57 and c.subme == 7 and c.width == 256]      # rerun with fenc_stride != fref_stride
SUBPEL_CASES = PLANTED_CASES + FLAT_CASES

# stages.InterRecon on the oracle's refined vectors (subme 2): (case, level, qp), levels 0 / 1 / 2 at every depth.  Seeds and QPs are chosen so that
# the oracle codes at least 30 % of the blocks and its reconstruction clips at both ends (tests/test_subpel_cases_cpu.py asserts both).
def _recon(depth, kind, seed, level, qp):
    return Case((depth, 256, 128, 57, kind, seed, 2)), level, qp


RECON_CASES = [_recon(8, "edges", 1, 0, 30), _recon(8, "edges", 1, 1, 30), _recon(8, "inverse", 1, 2, 46), _recon(8, "inverse", 1, 0, 46),
               _recon(10, "edges", 5, 0, 22), _recon(10, "edges", 5, 1, 38), _recon(10, "edges", 5, 2, 46), _recon(10, "inverse", 1, 1, 51), _recon(10, "inverse", 1, 2, 51),
               _recon(12, "edges", 2, 0, 12), _recon(12, "edges", 2, 1, 12), _recon(12, "edges", 2, 2, 38), _recon(12, "inverse", 1, 2, 22)]
