"""Deterministic pictures, vector fields and operating points for the merge stage of a P picture (numpy and the oracle only, no torch).

Sizes: 192x128 (3x2 CTUs: CTU (2, 0) and (0, 1) share a wave, B0 of CTU (0, 1) / (1, 1) comes from the above-right CTU), 64x64, 64x192 (one
CTU wide: its odd waves are empty) and 256x64.  Content: band-limited noise; the current picture is the reference displaced, block by
block, by the block's vector of the field - so the block's own vector predicts it well and every other candidate costs differently - and
one flat pair.  The fields are handed to the stage directly as searched vectors:

  uniform    one vector everywhere
  distinct   every block its own vector, all 16 phases
  rows / columns / quads   equal vectors along one direction or in 2x2 groups: each pruning pair
  knight     equal vectors along gbx + 2 gby: B0 equals A1 while B1 differs (the pair the reference does not prune)
  far_edge   +40 .. +57 samples in the last two block columns and rows, their negatives in the first (every fourth of those -72 .. -75
             samples, beyond clipMv's lower limit for the block below / right of it): inherited vectors clip
  flat       zero vectors on a flat pair: every candidate has sa8d 0

Inter costs: `real` = what x265hip_inter_sa8d_cost gives (the oracle's), `pattern` = merge cost + (-1, 0, +1)[block % 3]."""
import collections
import functools

import numpy as np

import intra_expect as IE
import intra_inter_cases as IIC
import intra_inter_expect as IX
import merge_expect as ME
import qp_map_expect as QE

F = IE.F
PAD = 80
FIELDS = ("uniform", "distinct", "rows", "columns", "quads", "knight", "far_edge", "flat")
VEC16 = [(k % 4 + 4 * ((k * 3) % 5 - 2), k // 4 + 4 * ((k * 2) % 7 - 3)) for k in range(16)]          # all 16 phases


def field_vector(field, gbx, gby, bw, bh):
    """The quarter-sample vector of block (gbx, gby) of a bw x bh grid."""
    if field == "uniform":
        return 6, -3
    if field == "flat":
        return 0, 0
    if field == "distinct":
        i = gby * bw + gbx
        return (i * 7) % 41 - 20, (i * 11) % 37 - 18
    if field == "rows":
        return VEC16[gby % 16]
    if field == "columns":
        return VEC16[gbx % 16]
    if field == "quads":
        return VEC16[((gbx // 2) * 3 + (gby // 2) * 5) % 16]
    if field == "knight":
        return VEC16[(gbx + 2 * gby) % 16]
    assert field == "far_edge"
    k = gby * 3 + gbx
    far = 4 * (40 + k % 18) + k % 4

    def near(j):
        return -(4 * (72 + j % 4) + 1) if j % 4 == 3 else -far
    qx = far if gbx >= bw - 2 else (near(gby) if gbx == 0 else 5)
    qy = far if gby >= bh - 2 else (near(gbx) if gby == 0 else -2)
    return qx, qy


def vectors(field, level, w64, h64):
    """(qx, qy) per block, index = ctu * blocks + z."""
    n = 8 << level
    bpc = 64 // n
    cw = w64 // 64
    out = []
    for b in range(cw * (h64 // 64) * bpc * bpc):
        ctu, z = divmod(b, bpc * bpc)
        bx, by = IE.zorder(z)
        out.append(field_vector(field, (ctu % cw) * bpc + bx, (ctu // cw) * bpc + by, cw * bpc, (h64 // 64) * bpc))
    return out


@functools.lru_cache(maxsize=None)
def _noise(w64, h64):
    rng = np.random.default_rng([977, w64, h64])
    return 128 + 42 * IIC._field(rng, 4 * (h64 + 2 * PAD), 4 * (w64 + 2 * PAD), 0.085)


@functools.lru_cache(maxsize=None)
def luma_pair(field, level, depth, w64, h64):
    """(reference Y, current Y) of w64 x h64."""
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    q = lambda a: np.clip(np.rint(a * sc), 0, mx).astype(dt)
    if field == "flat":
        flat = np.full((h64, w64), 128.0)
        return q(flat), q(flat)
    fy = _noise(w64, h64)
    n = 8 << level
    yy, xx = np.mgrid[0:h64, 0:w64]
    bw, bh = w64 // n, h64 // n
    vq = np.array([[field_vector(field, gbx, gby, bw, bh) for gbx in range(bw)] for gby in range(bh)])
    qx, qy = vq[yy // n, xx // n, 0], vq[yy // n, xx // n, 1]
    return q(fy[4 * (yy + PAD), 4 * (xx + PAD)]), q(fy[4 * (yy + PAD) + qy, 4 * (xx + PAD) + qx])


@functools.lru_cache(maxsize=None)
def chroma_pair(field, level, depth, w64, h64):
    """((Cb, Cr) reference, (Cb, Cr) current) of a 4:2:0 picture: smooth noise, the current planes displaced block by block by the luma
    field's vectors (a quarter luma sample is an eighth chroma sample)."""
    rng = np.random.default_rng([978, w64, h64])
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    q = lambda a: np.clip(np.rint(a * sc), 0, mx).astype(dt)
    cy, cx = np.mgrid[0:h64 // 2, 0:w64 // 2]
    nc = 4 << level
    bw, bh = w64 // (2 * nc), h64 // (2 * nc)
    vq = np.array([[field_vector(field, gbx, gby, bw, bh) for gbx in range(bw)] for gby in range(bh)])
    qx, qy = vq[cy // nc, cx // nc, 0], vq[cy // nc, cx // nc, 1]
    ref, cur = [], []
    for _ in range(2):
        f = 128 + 30 * IIC._field(rng, 8 * (h64 // 2 + PAD), 8 * (w64 // 2 + PAD), 0.04)
        ref.append(q(f[8 * (cy + PAD // 2), 8 * (cx + PAD // 2)]))
        cur.append(q(f[8 * (cy + PAD // 2) + qy, 8 * (cx + PAD // 2) + qx]))
    return tuple(ref), tuple(cur)


Case = collections.namedtuple("Case", "id field w h depth level costs max_merge lambda8 maps")


def _case(field, level, costs, max_merge, w=192, h=128, depth=8, lambda8=1024, maps=None):
    name = f"{w}x{h}-{field}-d{depth}-l{level}-{costs}-mm{max_merge}-lam{lambda8}" + (f"-{maps}" if maps else "")
    return Case(name, field, w, h, depth, level, costs, max_merge, lambda8, maps)


def _per_level(level):
    return [_case("uniform", level, "real", 3), _case("distinct", level, "pattern", 5), _case("distinct", level, "real", 2),
            _case("rows", level, "pattern", 3), _case("columns", level, "pattern", 5), _case("quads", level, "real", 3),
            _case("quads", level, "pattern", 5, lambda8=0), _case("knight", level, "pattern", 5), _case("far_edge", level, "pattern", 3),
            _case("far_edge", level, "pattern", 1), _case("far_edge", level, "real", 5), _case("flat", level, "real", 3)]


COVER_CASES = [c for level in (0, 1, 2) for c in _per_level(level)]                               # 8 bits, 192x128: what the coverage condition counts
DEEP_CASES = [_case("rows", 1, "pattern", 3, depth=10), _case("far_edge", 1, "pattern", 5, depth=10), _case("quads", 1, "real", 2, depth=10, lambda8=0),
              _case("quads", 1, "real", 3, depth=10, maps="map-lambda"), _case("knight", 1, "pattern", 5, depth=8, maps="map-lambda")]
SIZE_CASES = [_case("quads", 0, "pattern", 3, w=64, h=64), _case("distinct", 2, "pattern", 5, w=64, h=64),
              _case("rows", 1, "pattern", 3, w=64, h=192), _case("columns", 2, "pattern", 2, w=64, h=192), _case("far_edge", 0, "real", 5, w=64, h=192),
              _case("far_edge", 0, "pattern", 3, w=256, h=64), _case("quads", 2, "real", 5, w=256, h=64), _case("knight", 1, "pattern", 1, w=256, h=64)]
ALL_CASES = COVER_CASES + DEEP_CASES + SIZE_CASES


def tu_qp_map(depth, level, w64, h64):
    """tu_qp int8 [3, h/8, w/8]: both ends of the range, their neighbours, mid values and entries outside the range dealt over the blocks."""
    qmax = 51 + 6 * (depth - 8)
    vals = np.array([0, qmax, 1, qmax - 1, 30 + 6 * (depth - 8), 24 + 6 * (depth - 8), -3, min(qmax + 5, 127)], np.int64)
    n8 = 1 << level
    by, bx = np.mgrid[0:h64 // 8, 0:w64 // 8]
    idx = (bx // n8) * 3 + (by // n8) * 5
    return np.stack([vals[(idx + c) % len(vals)] for c in range(3)]).astype(np.int8)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """What the stage is fed: padded luma planes, the searched records, the operating point, the real inter costs.  Shared, never modified."""
    ref, cur = luma_pair(c.field, c.level, c.depth, c.w, c.h)
    pr, pc = F.pad_plane(ref)[0], F.pad_plane(cur)[0]
    nctu = (c.w // 64) * (c.h // 64)
    packed = [ME.pack(qx, qy) for qx, qy in vectors(c.field, c.level, c.w, c.h)]
    words = [(7 * i + 3) % 9001 for i in range(len(packed))]                                   # the searched records' cost words: passed through for inter blocks
    mv = ME.records(np.array(packed, np.int64).astype(np.int32), np.array(words, np.int32), c.level, nctu)
    qp = 30 + 6 * (c.depth - 8)
    tu_qp = tu_qp_map(c.depth, c.level, c.w, c.h) if c.maps else None
    lam_tab = QE.lambda8_table(c.depth) if c.maps else None
    real = None
    if c.costs == "real":
        real = IX.inter_side(c.depth, (pc,), (pr,), c.w, c.h, c.level, mv, qp, (qp, qp), 0, chroma=False, tu_qp=tu_qp, lambda8=c.lambda8, lambda8_by_qp=lam_tab,
                             table=IX.s_bitsizes(4 * 80 + 4))["inter_cost"]
    return dict(pref=pr, pcur=pc, mv=mv, qp=qp, tu_qp=tu_qp, lambda8_by_qp=lam_tab, real=real,
                pricer=ME.Pricer(c.depth, pc, pr, c.w, c.h, c.level))


def run_stage(c, mutation=None, inter_cost=None, max_merge=None, **temporal):
    """The expectation of a case (or of a mutation of the walk / other inter costs / another max_merge on the same inputs); temporal: the
    col / cur_delta / tmvp_mutation of ME.walk."""
    x = inputs(c)
    if inter_cost is None and c.costs == "real":
        inter_cost = x["real"][:, 1]
    return ME.stage_expectation(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level, x["mv"], max_merge or c.max_merge, c.lambda8, inter_cost=inter_cost,
                                cost_fn=ME.tie_pattern if inter_cost is None else None, tu_qp=x["tu_qp"], lambda8_by_qp=x["lambda8_by_qp"], qp=x["qp"],
                                mutation=mutation, pricer=x["pricer"], **temporal)


@functools.lru_cache(maxsize=None)
def expectation(c):
    x = dict(inputs(c))
    x["e"] = run_stage(c)
    return x
