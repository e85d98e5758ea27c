"""Deterministic inputs for the lookahead preparation tests (numpy and the oracle only, no torch): picture preparation, the intra
estimate, the cuTree step, the weighted-reference cost / application and the AQ energies at 12 bits and at the limits of their
arithmetic, and the censuses - plain numpy restatements that say which path an input takes.

Intra estimate: a chart of 36 regions, one per prediction mode, on which every reachable mode 0 .. 33 wins somewhere; stripe planes
on which the pure vertical / horizontal mode wins only through the clip of its edge filter; a transpose-symmetric plane whose
diagonal blocks tie modes m and 36 - m; flat, full-range and alternating pictures.  cuTree: funnels (hundreds of sources, one target),
targets on and just outside every picture edge, the bi-prediction weights 0 and 64, one-block and one-row grids, with a float64 +
np.add.at restatement of estimateCUPropagate as a second reference.  Weights: the ends of scale / denominator / offset on full-range
noise.  AQ: flat, half / half, checkerboard and noise pictures whose sums of squares pass 2^31.

tests/test_lookahead_cases_cpu.py asserts, with the oracle alone, that every case below reaches what it is listed for and pins the
oracle against the real classes on these inputs; tests/test_gpu_lookahead_cases.py feeds the same cases to the kernels."""
import functools
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

F = importlib.import_module("x265-yuuki-asuna_amd.frames")

DEPTHS = (8, 10, 12)
PENALTY = {8: 5, 10: 80, 12: 1280}              # 5 * (int)x265_lambda_tab[X265_LOOKAHEAD_QP] of the depth
ANGLES = (-32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32)


def oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def pixel_type(depth):
    return np.uint8 if depth == 8 else np.uint16


def _frozen(a, depth=None):
    a = np.ascontiguousarray(a if depth is None else a.astype(pixel_type(depth)))
    a.setflags(write=False)
    return a


def pad_edge(img, margin):
    """A plane of any size inside `margin` replicated samples: (flat buffer, stride, element offset of sample (0, 0))."""
    h, w = img.shape
    buf = np.pad(img, margin, mode="edge")
    return _frozen(buf.reshape(-1)), w + 2 * margin, margin * (w + 2 * margin) + margin


def lowres_geometry(width, height):
    """The geometry stages.Lookahead gives the half-resolution planes of a width x height picture (Lowres::create, the stride sized for
    the rounded width)."""
    wcu, hcu = (width // 2 + 7) >> 3, (height // 2 + 7) >> 3
    g = SimpleNamespace(wcu=wcu, hcu=hcu, width=wcu * 8, lines=hcu * 8, mx=F.MARGIN_X, my=F.MARGIN_Y)
    g.stride = (g.width + 2 * g.mx + 31) & ~31
    g.org = g.stride * g.my + g.mx
    g.rows = g.lines + 2 * g.my
    return g


# ---- intra estimate: the mode chart ------------------------------------------------------------------------------------------------------
CHART_SIZE, CHART_REGION = 192, 32
CHART_PERIODS = (23.0, 11.0, 6.3)              # of the three sinusoids, in half-resolution samples
CHART_AMPLITUDES = (0.22, 0.15, 0.10)


def mode_angle(mode):
    return ANGLES[8 + (mode - 26 if mode >= 18 else 10 - mode)]


@functools.lru_cache(maxsize=None)
def mode_chart(depth, seed=7):
    """192 x 192 full resolution, 6 x 6 regions of 32 x 32 (four 8 x 8 blocks of the half-resolution picture each): region 0 flat mid-grey,
    region 1 a bilinear ramp, region m = 2 .. 33 a smooth profile of t = u + v * angle(m) / 32 - constant along mode m's prediction
    direction, (u, v) = (x, y) for the vertical modes 18 .., (y, x) for the horizontal ones -, regions 34 and 35 full-range noise.  Of a
    region's four blocks the bottom-right one has its corner, above and left neighbours inside the region (the negative angles), the
    bottom-left one its above and above-right (the vertical modes 27 ..), the top-right one its left and below-left (the modes .. 9)."""
    mx = (1 << depth) - 1
    rng = np.random.default_rng([101, seed])
    img = np.zeros((CHART_SIZE, CHART_SIZE))
    yy, xx = np.mgrid[0:CHART_REGION, 0:CHART_REGION].astype(np.float64)
    for m in range(36):
        ry, rx = divmod(m, CHART_SIZE // CHART_REGION)
        phases = rng.uniform(0, 2 * np.pi, size=3)
        if m == 0:
            reg = np.full_like(xx, 0.5)
        elif m == 1:
            reg = 0.15 + 0.7 * (xx * (CHART_REGION - 1 - yy) + 0.4 * yy * (CHART_REGION - 1)) / (CHART_REGION - 1) ** 2
        elif m < 34:
            u, v = (xx, yy) if m >= 18 else (yy, xx)
            t = (u + v * mode_angle(m) / 32.0) / 2.0
            reg = 0.5 + sum(a * np.sin(2 * np.pi * t / p + ph) for a, p, ph in zip(CHART_AMPLITUDES, CHART_PERIODS, phases))
        else:
            reg = rng.integers(0, mx + 1, size=xx.shape) / mx
        img[ry * CHART_REGION:(ry + 1) * CHART_REGION, rx * CHART_REGION:(rx + 1) * CHART_REGION] = reg
    return _frozen(np.clip(np.rint(img * mx), 0, mx), depth)


# ---- intra estimate: planes handed over directly -----------------------------------------------------------------------------------------
PLANE_MARGIN = 16                               # the estimate reads 1 sample up / left and 8 past the right / bottom edge


def _plane_case(img, depth):
    buf, stride, org = pad_edge(_frozen(img, depth), PLANE_MARGIN)
    h, w = img.shape
    return SimpleNamespace(img=_frozen(img, depth), plane=buf, stride=stride, org=org, wcu=w // 8, hcu=h // 8, depth=depth)


@functools.lru_cache(maxsize=None)
def clip_plane(depth, transposed, seed=11):
    """96 x 96 vertical stripes with column values in [max / 4, 3 max / 4).  For the blocks (i, j), i and j odd: column x = 8 i is an extreme
    over the block and the block above it - max or 0 by ((i + j) / 2) % 2 - and the block's corner neighbour (8 i - 1, 8 j - 1) the opposite
    one, so that above[0] + ((left[r] - corner) >> 1) leaves [0, max] and only its clipped value equals the block's column 0: mode 26 predicts
    the block exactly, through the clip.  transposed: the same for mode 10."""
    mx = (1 << depth) - 1
    rng = np.random.default_rng([103, depth, seed])
    p = np.tile(rng.integers((mx + 1) // 4, 3 * (mx + 1) // 4, size=96), (96, 1))
    for j in range(1, 12, 2):
        for i in range(1, 12, 2):
            e = mx if ((i + j) // 2) % 2 == 0 else 0
            p[8 * j - 8:8 * j + 8, 8 * i] = e
            p[8 * j - 1, 8 * i - 1] = mx - e
    return _plane_case(p.T if transposed else p, depth)


def clip_census(case, modes, transposed):
    """Blocks whose winner is the pure mode (26, transposed 10) and whose unclipped edge-filter value leaves the range: (above max, below 0)."""
    p = case.img.astype(np.int64)
    if transposed:
        p = p.T
    hi = lo = 0
    m = modes.reshape(case.hcu, case.wcu)
    if transposed:
        m = m.T
    for j in range(1, 12):
        for i in range(1, 12):
            if m[j, i] != (10 if transposed else 26):
                continue
            v = p[8 * j - 1, 8 * i] + ((p[8 * j:8 * j + 8, 8 * i - 1] - p[8 * j - 1, 8 * i - 1]) >> 1)
            hi += bool((v > (1 << case.depth) - 1).any())
            lo += bool((v < 0).any())
    return hi, lo


@functools.lru_cache(maxsize=None)
def tie_plane(depth, seed=13):
    """64 x 64, n + n.T halved: the diagonal blocks and their neighbours are transpose-symmetric, so modes m and 36 - m cost the same there."""
    rng = np.random.default_rng([107, depth, seed])
    n = rng.integers(0, 1 << depth, size=(64, 64))
    return _plane_case((n + n.T) >> 1, depth)


# ---- picture preparation + intra estimate on whole pictures ------------------------------------------------------------------------------
PICTURE_KINDS = ("max", "zero", "noise", "checker", "rows", "cols")
PICTURE_SIZES = ((128, 64), (200, 136), (16, 16))        # the second reads the source margin, the third is one block (seven idle block slots)
PICTURE_CASES = [SimpleNamespace(id=f"{k}-d{d}-{w}x{h}", kind=k, depth=d, width=w, height=h) for d in (10, 12) for k in PICTURE_KINDS for (w, h) in PICTURE_SIZES]


@functools.lru_cache(maxsize=None)
def picture(kind, depth, width, height, seed=17):
    mx = (1 << depth) - 1
    yy, xx = np.mgrid[0:height, 0:width]
    if kind == "max":
        img = np.full((height, width), mx)
    elif kind == "zero":
        img = np.zeros((height, width), np.int64)
    elif kind == "noise":
        img = np.random.default_rng([109, depth, width, height, seed]).integers(0, mx + 1, size=(height, width))
    elif kind == "checker":
        img = ((xx + yy) & 1) * mx
    elif kind == "rows":
        img = (yy & 1) * mx
    elif kind == "cols":
        img = (xx & 1) * mx
    elif kind == "chart":
        return mode_chart(depth)
    else:
        raise ValueError(kind)
    return _frozen(img, depth)


def prepare(depth, img, penalty):
    """The oracle's preparation of a picture: (padded source, its stride / org, geometry, four planes, intraCost, intraMode, lowresCosts)."""
    O = oracle()
    h, w = img.shape
    src, stride, org, _, _ = F.pad_plane(img)
    g = lowres_geometry(w, h)
    planes = O.lowres_init(depth, src, stride, org, g.stride, g.org, g.rows, g.width, g.lines, g.mx, g.my)
    cost, mode, lc = O.lowres_intra(depth, planes[0], g.stride, g.org, g.wcu, g.hcu, penalty)
    return SimpleNamespace(src=src, src_stride=stride, src_org=org, g=g, planes=planes, cost=cost, mode=mode, lc=lc)


# ---- cuTree ------------------------------------------------------------------------------------------------------------------------------
def _cutree(id, wcu, hcu, intra, inter, lists, mv0, mv1, invq, prop, r0, r1, fps=1.0, bipred=32):
    n = wcu * hcu
    lcost = (np.asarray(inter, np.int64) | (np.asarray(lists, np.int64) << 14)).astype(np.uint16)
    mvs = lambda a: None if a is None else _frozen(np.asarray(a, np.int32).reshape(n, 2))
    u16 = lambda a: None if a is None else _frozen(np.asarray(a, np.uint16).reshape(n))
    return SimpleNamespace(id=id, wcu=wcu, hcu=hcu, intra=_frozen(np.asarray(intra, np.int32).reshape(n)), lcost=_frozen(lcost), mv0=mvs(mv0), mv1=mvs(mv1),
                           invq=_frozen(np.asarray(invq, np.int32).reshape(n)), prop=u16(prop), r0=u16(r0), r1=u16(r1), fps=fps, bipred=bipred, bframe=mv1 is not None)


def _funnel(id, intra_lo, intra_hi, invq, seed):
    w, h, tx, ty = 24, 12, 11, 5
    rng = np.random.default_rng([113, seed])
    n = w * h
    bx, by = np.arange(n) % w, np.arange(n) // w
    intra = rng.integers(intra_lo, intra_hi + 1, size=n)
    inter = (intra * rng.uniform(0.0, 0.3, size=n)).astype(np.int64).clip(0, 16383)
    mv0 = np.stack([(tx - bx) * 32 + rng.integers(0, 32, size=n), (ty - by) * 32 + rng.integers(0, 32, size=n)], axis=1)
    mv1 = np.stack([(tx - bx) * 32, (ty - by) * 32], axis=1)                # exact multiples of 32, the negative ones included
    return _cutree(id, w, h, intra, inter, np.full(n, 3), mv0, mv1, np.full(n, invq), None, np.zeros(n), np.zeros(n))


def _border(seed=3):
    w, h = 16, 8
    rng = np.random.default_rng([127, seed])
    n = w * h
    bx, by = np.arange(n) % w, np.arange(n) // w
    intra = rng.integers(200, 9000, size=n)
    inter = (intra * rng.uniform(0.0, 0.6, size=n)).astype(np.int64)
    # per block a target column from {-2, -1, w - 1, w} or the block's own, the same in y, fractions 0, 1, 31
    sx, sy = rng.integers(0, 5, size=n), rng.integers(0, 5, size=n)
    tx = np.where(sx == 4, bx, np.array([-2, -1, w - 1, w, 0])[sx])
    ty = np.where(sy == 4, by, np.array([-2, -1, h - 1, h, 0])[sy])

    def field():
        f = np.array([0, 1, 31])
        m = np.stack([(tx - bx) * 32 + f[rng.integers(0, 3, size=n)], (ty - by) * 32 + f[rng.integers(0, 3, size=n)]], axis=1)
        m[0], m[1], m[w] = (-1, -32), (-32, -1), (-1, 31)                     # block 0: target (-1, -1), fractions (31, 0); block (0, 1): (-1, 0), (31, 31)
        return m
    return _cutree("border", w, h, intra, inter, rng.choice([1, 2, 3], size=n), field(), field(), np.full(n, 256), rng.integers(0, 20000, size=n),
                   rng.integers(0, 20000, size=n), rng.integers(0, 20000, size=n))


def _coherent_mvs(rng, w, h):
    base = rng.integers(-40, 41, size=(h // 4 + 1, w // 4 + 1, 2))
    return np.kron(base, np.ones((4, 4, 1), np.int64))[:h, :w].reshape(w * h, 2) + rng.integers(-3, 4, size=(w * h, 2))


def _bipred_end(weight):
    w, h = 17, 9
    rng = np.random.default_rng([131, weight])
    n = w * h
    intra = rng.integers(200, 9000, size=n)
    inter = (intra * rng.uniform(0.0, 0.8, size=n)).astype(np.int64)
    return _cutree(f"bipred-{weight}", w, h, intra, inter, np.full(n, 3), _coherent_mvs(rng, w, h), _coherent_mvs(rng, w, h), rng.integers(64, 1024, size=n),
                   rng.integers(0, 40000, size=n), rng.integers(0, 30000, size=n), rng.integers(0, 30000, size=n), bipred=weight)


def _tiny(w, h, bframe):
    rng = np.random.default_rng([137, w, h, int(bframe)])
    n = w * h
    intra = rng.integers(200, 9000, size=n)
    inter = (intra * rng.uniform(0.0, 0.8, size=n)).astype(np.int64)
    mv = lambda: rng.integers(-70, 71, size=(n, 2)) * (rng.random((n, 1)) < 0.8)
    lists = rng.choice([1, 2, 3], size=n) if bframe else rng.integers(0, 2, size=n)
    return _cutree(f"tiny-{w}x{h}-{'b' if bframe else 'p'}", w, h, intra, inter, lists, mv(), mv() if bframe else None, rng.integers(64, 1024, size=n),
                   rng.integers(0, 40000, size=n), rng.integers(0, 60000, size=n), rng.integers(0, 60000, size=n) if bframe else None, fps=0.8)


@functools.lru_cache(maxsize=None)
def cutree_cases():
    return ([_funnel("funnel-small", 20, 60, 64, 1), _funnel("funnel-big", 20000, 32767, 16000, 2), _border(), _bipred_end(0), _bipred_end(64)] +
            [_tiny(w, h, b) for (w, h) in ((1, 1), (1, 7), (257, 1)) for b in (False, True)])


def cutree_oracle(c, depth=8):
    return oracle().cutree_propagate(depth, c.wcu, c.hcu, c.prop, c.intra, c.lcost, c.invq, c.mv0, c.mv1, c.fps, c.bipred, c.r0, c.r1)


def cutree_restatement(c):
    """Lookahead::estimateCUPropagate in plain numpy: the amounts in float64 with separate multiply / add / divide, then the integer
    scatter with np.add.at into 64-bit sums and one saturation at the end (every add is >= 0, so the reference's saturating adds give
    the same).  Returns (ref_cost0, ref_cost1 or None, census): the integer amounts, per list the number of sources that reach every
    target with a non-zero share, and the shares that land on / fall off each side of the picture among the sources aimed at it."""
    w, h = c.wcu, c.hcu
    n = w * h
    intra, lc = c.intra.astype(np.int64), c.lcost.astype(np.int64)
    inter = np.minimum(intra, lc & 0x3fff)
    prop = np.zeros(n) if c.prop is None else c.prop.astype(np.float64)
    amount = prop + (intra * c.invq.astype(np.int64)).astype(np.float64) * (c.fps / 256)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = amount * (intra - inter).astype(np.float64) / intra.astype(np.float64) + 0.5
    ok = (r >= 1.0) & (r < 2147483648.0)                                    # NaN (intra 0) compares false
    amt = np.where(ok, np.floor(np.where(ok, r, 0.0)), 0).astype(np.int64)
    lists = lc >> 14
    bx, by = np.arange(n) % w, np.arange(n) // w
    weights = (c.bipred, 64 - c.bipred)
    census = SimpleNamespace(amount=amt, sources=[], landed=dict.fromkeys(("left", "right", "top", "bottom"), 0),
                             dropped=dict.fromkeys(("left", "right", "top", "bottom"), 0))
    out = []
    for l, (mv, rc) in enumerate(((c.mv0, c.r0), (c.mv1, c.r1))):
        if rc is None:
            out.append(None)
            continue
        acc, srcs = np.zeros(n, np.int64), np.zeros(n, np.int64)
        use = ok & (((lists >> l) & 1) == 1)
        la = np.where(lists == 3, (amt * weights[l] + 32) >> 6, amt)
        x, y = mv[:, 0].astype(np.int64), mv[:, 1].astype(np.int64)
        still = use & (x == 0) & (y == 0)
        np.add.at(acc, np.nonzero(still)[0], la[still])
        np.add.at(srcs, np.nonzero(still & (la > 0))[0], 1)
        moved = use & ~still
        cux, cuy, fx, fy = (x >> 5) + bx, (y >> 5) + by, x & 31, y & 31
        wgt = ((32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx)
        for k in range(4):
            tx, ty = cux + (k & 1), cuy + (k >> 1)
            inside = (tx >= 0) & (ty >= 0) & (tx < w) & (ty < h)
            v = (la * wgt[k] + 512) >> 10
            hit = moved & inside
            np.add.at(acc, (ty * w + tx)[hit], v[hit])
            np.add.at(srcs, (ty * w + tx)[hit & (v > 0)], 1)
            for side, aimed, off in (("left", cux == -1, tx < 0), ("right", cux == w - 1, tx >= w), ("top", cuy == -1, ty < 0), ("bottom", cuy == h - 1, ty >= h)):
                census.landed[side] += int((hit & aimed & (v > 0)).sum())
                census.dropped[side] += int((moved & off & (v > 0)).sum())
        census.sources.append(srcs)
        out.append(np.minimum(rc.astype(np.int64) + acc, 65535).astype(np.uint16))
    return out[0], out[1], census


# ---- weighted reference ------------------------------------------------------------------------------------------------------------------
WEIGHT_LAUNCHES = ([None, (127, 0, 127), (1, 7, -128), (64, 6, 127)], [(64, 6, -128), (127, 7, 0), (0, 0, 0), (33, 5, -1)])
WEIGHTS = [c for launch in WEIGHT_LAUNCHES for c in launch if c is not None]


@functools.lru_cache(maxsize=None)
def weight_case(depth, seed=19):
    """Half-resolution planes of 64 x 48 full-range noise in the geometry stages.Lookahead gives a 128 x 96 picture: the current picture's
    plane 0 and the reference's four planes, noise over the whole buffers (the application weights margins and all), and the two intra caps -
    1 << 20 everywhere (never binds) and the current plane's own intra estimate.  Independent noise always costs more than the intra
    estimate, so every fourth block of the reference's plane 0 repeats the current picture's block: there the cap does not bind for the
    weights near the identity."""
    g = lowres_geometry(128, 96)
    rng = np.random.default_rng([139, depth, seed])
    cur, ref = [rng.integers(0, 1 << depth, size=(g.rows, g.stride)).astype(pixel_type(depth)) for _ in range(2)]
    for by in range(g.hcu):
        for bx in range(g.wcu):
            if (bx + by) % 4 == 0:
                ys, xs = slice(g.my + 8 * by, g.my + 8 * by + 8), slice(g.mx + 8 * bx, g.mx + 8 * bx + 8)
                ref[ys, xs] = cur[ys, xs]
    cur = _frozen(cur.reshape(-1))
    ref = [_frozen(ref.reshape(-1))] + [_frozen(rng.integers(0, 1 << depth, size=g.rows * g.stride).astype(pixel_type(depth))) for _ in range(3)]
    own = oracle().lowres_intra(depth, cur, g.stride, g.org, g.wcu, g.hcu, PENALTY[depth])[0]
    return SimpleNamespace(depth=depth, g=g, cur=cur, ref=ref, caps={"never": _frozen(np.full(g.wcu * g.hcu, 1 << 20, np.int32)), "own": _frozen(own)})


def weight_block_costs(wc, cand):
    """The uncapped 8 x 8 SATD of every block for one candidate: the oracle's weightCostLuma on a picture of one block."""
    O, g = oracle(), wc.g
    big = np.full(1, 1 << 30, np.int32)
    return np.array([O.lowres_weight_cost(wc.depth, wc.cur, wc.ref[0], g.stride, g.org + 8 * by * g.stride + 8 * bx, 8, 8, big, cand)
                     for by in range(g.hcu) for bx in range(g.wcu)], dtype=np.int64)


# ---- adaptive quantisation ---------------------------------------------------------------------------------------------------------------
AQ_FAMILIES = ("zero", "max", "half", "checker", "noise")
AQ_SIZES = ((64, 48), (58, 38))                 # the second: partial last blocks, luma and chroma


def _aq_plane(family, depth, width, height, half, rng):
    mx = (1 << depth) - 1
    yy, xx = np.mgrid[0:height, 0:width]
    if family == "zero":
        img = np.zeros((height, width), np.int64)
    elif family == "max":
        img = np.full((height, width), mx)
    elif family == "half":
        img = ((xx % (2 * half)) >= half) * mx
    elif family == "checker":
        img = ((xx + yy) & 1) * mx
    elif family == "noise":
        img = rng.integers(0, mx + 1, size=(height, width))
    else:
        raise ValueError(family)
    return _frozen(img, depth)


@functools.lru_cache(maxsize=None)
def aq_picture(family, depth, width, height, seed=23):
    """Y, Cb, Cr of a 4:2:0 picture; `half`: every 16 x 16 luma (8 x 8 chroma) block is 0 on its left half and max on its right one."""
    rng = np.random.default_rng([149, depth, width, height, seed])
    return (_aq_plane(family, depth, width, height, 8, rng), _aq_plane(family, depth, width // 2, height // 2, 4, rng),
            _aq_plane(family, depth, width // 2, height // 2, 4, rng))


def aq_cases(depth):
    """(family, size, qg, mode): everything at 8 and 12 bits, one pass over the families at 10."""
    if depth == 10:
        return [SimpleNamespace(id=f"{f}-d10-58x38-qg16-m{1 + i % 3}", family=f, depth=10, width=58, height=38, qg=16, mode=1 + i % 3, strength=1.0) for i, f in enumerate(AQ_FAMILIES)]
    return [SimpleNamespace(id=f"{f}-d{depth}-{w}x{h}-qg{qg}-m{m}", family=f, depth=depth, width=w, height=h, qg=qg, mode=m, strength=1.0 if m < 3 else 0.8)
            for f in AQ_FAMILIES for (w, h) in AQ_SIZES for qg in (16, 8) for m in (1, 2, 3)]


def aq_inputs(case, chroma=True):
    """(padded luma, stride, org, chroma keywords of the oracle / the stage) - luma in the frames.pad_plane geometry, chroma inside 16
    replicated samples."""
    y, cb, cr = aq_picture(case.family, case.depth, case.width, case.height)
    yp, stride, org, _, _ = F.pad_plane(y)
    kw = {}
    if chroma:
        pb, stride_c, org_c = pad_edge(cb, 16)
        kw = dict(cb=pb, cr=pad_edge(cr, 16)[0], stride_c=stride_c, org_c=org_c)
    return _frozen(yp.reshape(-1)), stride, org, kw


HEVC_AQ_CASES = [SimpleNamespace(id="flat-d8-64x48-qg16", family="max", depth=8, width=64, height=48, qg=16, range=1.0),
                 SimpleNamespace(id="noise-d8-130x66-qg64", family="noise", depth=8, width=130, height=66, qg=64, range=2.0),      # partitions clipped to 2 x 2: numPix 1
                 SimpleNamespace(id="noise-d8-130x66-qg8", family="noise", depth=8, width=130, height=66, qg=8, range=6.0),
                 SimpleNamespace(id="flat-d12-66x34-qg8", family="max", depth=12, width=66, height=34, qg=8, range=1.0),
                 SimpleNamespace(id="noise-d12-66x34-qg8", family="noise", depth=12, width=66, height=34, qg=8, range=3.0)]
