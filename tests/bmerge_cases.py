"""Deterministic pictures, inter winners and operating points for the merge stage of a B picture (numpy and the oracle only, no torch).

Sizes: 192x128 (3x2 CTUs: CTU (2, 0) and (0, 1) share a wave, B0 of CTU (0, 1) / (1, 1) comes from the above-right CTU), 64x64, 64x192 (one
CTU wide: its odd waves are empty) and 256x64.  Content: two references of band-limited noise (independent); the current picture is, block
by block, reference 0 displaced by the block's list-0 vector, reference 1 displaced by its list-1 vector or the rounded average of both -
whichever the block's direction names, so that direction with those vectors is the cheapest by construction - and one flat triple.  The
inter winners are handed to the stage directly as (dir, list-0 vector, list-1 vector) per block; an unused list keeps its vector in the
input record, as a CU's arrays keep what was stored there.  The kinds:

  uniform      one motion everywhere, both lists
  distinct     every block its own vectors, all 16 phases in each list, directions 1 / 2 / 3 by block
  rows / columns / quads   equal motion along one direction or in 2x2 groups: each pruning pair
  knight       equal motion along gbx + 2 gby: B0 equals A1 while B1 differs (the pair the reference does not prune)
  dir_stripes  one list-0 vector and one list-1 vector in the lists a block uses, directions 1 / 3 / 2 by column: neighbours that differ in
               nothing but the direction (the direction rule of hasEqualMotion); the list a block does not use holds another vector in
               every row, which the reference never reads
  cross        directions 1 and 2 only, arranged along the diagonals so that a block's left neighbour uses list 0 and its upper one list 1
               or the reverse; content = the average: the combined candidates are the only bidirectional ones, and they predict best
  far_edge     the far_edge field of merge_cases in list 0 and, one sample nearer, in list 1, directions 1 / 2 / 3 by block: inherited
               vectors cross both clip limits in each list
  same_ref     cross with list 1 naming the same picture as list 0 and equal vectors: every combined candidate is suppressed; every fifth
               block along gbx + 2 gby is unmoved content, where the zero candidate wins and its index shows what stood in front of it
  flat         zero vectors, both lists, on a flat triple: every candidate has sa8d 0

Inter costs: `real` = the inter winner is what x265hip_b_sa8d_decide makes of the kind's records (bsa8d_expect.decide: its dir, vectors and
cost word 0), `pattern` = merge cost + (-1, 0, +1)[block % 3] with the kind's motion as the winner."""
import collections
import functools

import numpy as np

import bmerge_expect as BM
import bsa8d_expect as BX
import intra_expect as IE
import intra_inter_cases as IIC
import intra_inter_expect as IX
import merge_cases as MC
import qp_map_expect as QE

F = IE.F
PAD = MC.PAD
KINDS = ("uniform", "distinct", "rows", "columns", "quads", "knight", "dir_stripes", "cross", "far_edge", "same_ref", "flat")
VEC16 = MC.VEC16
RANGE = 80                                       # the search range the bit-size table of the `real` cases is sized for


def kind_motion(kind, gbx, gby, bw, bh):
    """(dir, (qx0, qy0), (qx1, qy1)) of block (gbx, gby) of a bw x bh grid."""
    i = gby * bw + gbx
    if kind == "uniform":
        return 3, (6, -3), (-5, 2)
    if kind == "flat":
        return 3, (0, 0), (0, 0)
    if kind == "distinct":
        return 1 + i % 3, MC.field_vector("distinct", gbx, gby, bw, bh), ((i * 5) % 43 - 21, (i * 13) % 39 - 19)
    if kind == "rows":
        return 1 + gby % 3, VEC16[gby % 16], VEC16[(gby * 7 + 3) % 16]
    if kind == "columns":
        return 1 + (gbx // 2) % 3, VEC16[gbx % 16], VEC16[(gbx * 5 + 1) % 16]
    if kind == "quads":
        g = (gbx // 2) * 3 + (gby // 2) * 5
        return 1 + g % 3, VEC16[g % 16], VEC16[(g * 3 + 2) % 16]
    if kind == "knight":
        g = gbx + 2 * gby
        return 1 + (g // 2) % 3, VEC16[g % 16], VEC16[(g + 5) % 16]
    if kind == "dir_stripes":                    # the list a block does not use holds another vector in every row: never read by the reference
        d = (1, 3, 2)[gbx % 3]
        return d, ((6, -3) if d & 1 else VEC16[(gby + 3) % 16]), ((-5, 2) if d & 2 else VEC16[gby % 16])
    if kind in ("cross", "same_ref"):
        d = 1 if (gbx - gby) % 4 in (2, 3) else 2
        return d, (6, -3), ((6, -3) if kind == "same_ref" else (-5, 2))
    assert kind == "far_edge"
    qx, qy = MC.field_vector("far_edge", gbx, gby, bw, bh)
    return 1 + i % 3, (qx, qy), (qx + (4 if qx < 0 else -4), qy + (4 if qy < 0 else -4))          # one sample nearer: inside the planes' margins like list 0


def kind_content(kind, gbx, gby, bw, bh):
    """(dir, (qx0, qy0), (qx1, qy1)) the current picture's block is built from: the block's own motion, but for cross / same_ref the average
    of both lists everywhere (what the combined candidates predict) and for same_ref every fifth block along gbx + 2 gby unmoved - there
    the zero candidate predicts best, and its index tells whether a combined candidate stood in front of it."""
    d, v0, v1 = kind_motion(kind, gbx, gby, bw, bh)
    if kind == "same_ref" and (gbx + 2 * gby) % 5 == 0:
        return 3, (0, 0), (0, 0)
    return (3 if kind in ("cross", "same_ref") else d), v0, v1


def motions(kind, level, w64, h64):
    """kind_motion per block, index = ctu * blocks + z."""
    n = 8 << level
    bpc = 64 // n
    cw = w64 // 64
    out = []
    for b in range(cw * (h64 // 64) * bpc * bpc):
        ctu, z = divmod(b, bpc * bpc)
        bx, by = IE.zorder(z)
        out.append(kind_motion(kind, (ctu % cw) * bpc + bx, (ctu // cw) * bpc + by, cw * bpc, (h64 // 64) * bpc))
    return out


@functools.lru_cache(maxsize=None)
def _noise(w64, h64, which):
    rng = np.random.default_rng([979 + which, w64, h64])
    return 128 + 42 * IIC._field(rng, 4 * (h64 + 2 * PAD), 4 * (w64 + 2 * PAD), 0.085)


@functools.lru_cache(maxsize=None)
def luma_triple(kind, level, depth, w64, h64):
    """(reference 0 Y, current Y, reference 1 Y) of w64 x h64."""
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    q = lambda a: np.clip(np.rint(a * sc), 0, mx).astype(dt)
    if kind == "flat":
        flat = q(np.full((h64, w64), 128.0))
        return flat, flat.copy(), flat.copy()
    f0 = _noise(w64, h64, 0)
    f1 = f0 if kind == "same_ref" else _noise(w64, h64, 1)
    n = 8 << level
    yy, xx = np.mgrid[0:h64, 0:w64]
    bw, bh = w64 // n, h64 // n
    km = [[kind_content(kind, gbx, gby, bw, bh) for gbx in range(bw)] for gby in range(bh)]
    d = np.array([[m[0] for m in row] for row in km])[yy // n, xx // n]
    v = [np.array([[m[1 + l] for m in row] for row in km])[yy // n, xx // n] for l in (0, 1)]
    moved = [f[4 * (yy + PAD) + v[l][..., 1], 4 * (xx + PAD) + v[l][..., 0]] for l, f in enumerate((f0, f1))]
    cur =np.where(d == 1, moved[0], np.where(d == 2, moved[1], (moved[0] + moved[1]) / 2))
    return q(f0[4 * (yy + PAD), 4 * (xx + PAD)]), q(cur), q(f1[4 * (yy + PAD), 4 * (xx + PAD)])


@functools.lru_cache(maxsize=None)
def chroma_triple(kind, level, depth, w64, h64):
    """((Cb, Cr) of reference 0, of the current picture, of reference 1) of a 4:2:0 picture: smooth noise, the current planes built like
    the luma plane from the kind's motion (a quarter luma sample is an eighth chroma sample)."""
    rng = np.random.default_rng([980, w64, h64])
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = IE.harness.pix_dtype(depth)
    q = lambda a: np.clip(np.rint(a * sc), 0, mx).astype(dt)
    cy, cx = np.mgrid[0:h64 // 2, 0:w64 // 2]
    nc = 4 << level
    bw, bh = w64 // (2 * nc), h64 // (2 * nc)
    km = [[kind_content(kind, gbx, gby, bw, bh) for gbx in range(bw)] for gby in range(bh)]
    d = np.array([[m[0] for m in row] for row in km])[cy // nc, cx // nc]
    v = [np.array([[m[1 + l] for m in row] for row in km])[cy // nc, cx // nc] for l in (0, 1)]
    planes = [[], [], []]
    for _ in range(2):
        f = [128 + 30 * IIC._field(rng, 8 * (h64 // 2 + PAD), 8 * (w64 // 2 + PAD), 0.04) for _ in (0, 1)]
        if kind == "same_ref":
            f[1] = f[0]
        moved = [f[l][8 * (cy + PAD // 2) + v[l][..., 1], 8 * (cx + PAD // 2) + v[l][..., 0]] for l in (0, 1)]
        planes[0].append(q(f[0][8 * (cy + PAD // 2), 8 * (cx + PAD // 2)]))
        planes[1].append(q(np.where(d == 1, moved[0], np.where(d == 2, moved[1], (moved[0] + moved[1]) / 2))))
        planes[2].append(q(f[1][8 * (cy + PAD // 2), 8 * (cx + PAD // 2)]))
    return tuple(tuple(p) for p in planes)


Case = collections.namedtuple("Case", "id kind w h depth level costs max_merge lambda8 maps")


def _case(kind, level, costs, max_merge, w=192, h=128, depth=8, lambda8=1024, maps=None):
    name = f"{w}x{h}-{kind}-d{depth}-l{level}-{costs}-mm{max_merge}-lam{lambda8}" + (f"-{maps}" if maps else "")
    return Case(name, kind, w, h, depth, level, costs, max_merge, lambda8, maps)


def _per_level(level):
    return [_case("uniform", level, "real", 3), _case("distinct", level, "pattern", 5), _case("distinct", level, "real", 2),
            _case("rows", level, "pattern", 3), _case("columns", level, "pattern", 5), _case("quads", level, "real", 3),
            _case("quads", level, "pattern", 5, lambda8=0), _case("knight", level, "pattern", 5), _case("dir_stripes", level, "pattern", 5),
            _case("dir_stripes", level, "real", 3), _case("cross", level, "pattern", 3), _case("cross", level, "real", 5),
            _case("far_edge", level, "pattern", 3), _case("far_edge", level, "pattern", 1), _case("far_edge", level, "real", 5),
            _case("same_ref", level, "pattern", 5), _case("flat", level, "real", 3)]


COVER_CASES = [c for level in (0, 1, 2) for c in _per_level(level)]                               # 8 bits, 192x128: what the coverage condition counts
DEEP_CASES = [_case("rows", 1, "pattern", 3, depth=10), _case("far_edge", 1, "pattern", 5, depth=10), _case("cross", 1, "real", 2, depth=10, lambda8=0),
              _case("quads", 1, "real", 3, depth=10, maps="map-lambda"), _case("dir_stripes", 1, "pattern", 5, depth=8, maps="map-lambda")]
SIZE_CASES = [_case("quads", 0, "pattern", 3, w=64, h=64), _case("distinct", 2, "pattern", 5, w=64, h=64),
              _case("cross", 1, "pattern", 3, w=64, h=192), _case("columns", 2, "pattern", 2, w=64, h=192), _case("far_edge", 0, "real", 5, w=64, h=192),
              _case("far_edge", 0, "pattern", 3, w=256, h=64), _case("same_ref", 2, "real", 5, w=256, h=64), _case("knight", 1, "pattern", 1, w=256, h=64)]
ALL_CASES = COVER_CASES + DEEP_CASES + SIZE_CASES


def ref_ids(c):
    return (0, 0) if c.kind == "same_ref" else (0, 1)


@functools.lru_cache(maxsize=None)
def inputs(c):
    """What the stage is fed: padded luma planes, the inter winner (dir_in, mv0, mv1), the operating point and, for `real` costs, the
    decision of bsa8d_expect.decide the winner was taken from.  Shared, never modified."""
    r0, cur, r1 = luma_triple(c.kind, c.level, c.depth, c.w, c.h)
    p0, pc, p1 = (F.pad_plane(p)[0] for p in (r0, cur, r1))
    nctu = (c.w // 64) * (c.h // 64)
    km = motions(c.kind, c.level, c.w, c.h)
    nb = len(km)
    pk = lambda v: np.array([BM.pack(*x) for x in v], np.int64).astype(np.int32)
    # the records' cost words: list 0 is the cheaper list where the kind's direction uses it
    w0 = np.array([40 + (7 * i) % 23 if m[0] & 1 else 400 + i % 11 for i, m in enumerate(km)], np.int32)
    w1 = np.array([45 + (5 * i) % 19 if m[0] == 2 else (90 if m[0] == 3 else 410) + i % 7 for i, m in enumerate(km)], np.int32)
    recs = [BM.records(pk([m[1] for m in km]), w0, c.level, nctu), BM.records(pk([m[2] for m in km]), w1, c.level, nctu)]
    qp = 30 + 6 * (c.depth - 8)
    tu_qp = MC.tu_qp_map(c.depth, c.level, c.w, c.h) if c.maps else None
    lam_tab = QE.lambda8_table(c.depth) if c.maps else None
    out = dict(pref=(p0, p1), pcur=pc, recs=recs, qp=qp, tu_qp=tu_qp, lambda8_by_qp=lam_tab, nctu=nctu, ref_ids=ref_ids(c),
               pricer=BM.Pricer(c.depth, pc, p0, p1, c.w, c.h, c.level))
    if c.costs == "real":
        d = BX.decide(c.depth, pc, (p0, p1), c.w, c.h, c.level, recs, lambda8=c.lambda8, table=IX.s_bitsizes(4 * RANGE + 4), qp=qp, tu_qp=tu_qp,
                      lambda8_by_qp=lam_tab, ref_ids=ref_ids(c), with_reference=False)
        out.update(decision=d, dir_in=d["dir"], mv0=BX.BE.full_mv_out(c.level, nctu, d["mv0"], 0), mv1=BX.BE.full_mv_out(c.level, nctu, d["mv1"], 0),
                   real=d["cost"][:, 0].astype(np.int64))
    else:
        out.update(decision=None, dir_in=np.array([m[0] for m in km], np.uint8), mv0=recs[0], mv1=recs[1], real=None)
    assert len(out["dir_in"]) == nb
    return out


def run_stage(c, mutation=None, inter_cost=None, max_merge=None, **temporal):
    """The expectation of a case (or of a mutation of the walk / other inter costs / another max_merge on the same inputs); temporal: the
    col / cur_deltas / tmvp_mutation of BM.walk."""
    x = inputs(c)
    if inter_cost is None and c.costs == "real":
        inter_cost = x["real"]
    return BM.stage_expectation(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level, x["dir_in"], x["mv0"], x["mv1"], max_merge or c.max_merge, c.lambda8,
                                inter_cost=inter_cost, cost_fn=BM.tie_pattern if inter_cost is None else None, tu_qp=x["tu_qp"],
                                lambda8_by_qp=x["lambda8_by_qp"], qp=x["qp"], ref_ids=x["ref_ids"], mutation=mutation, pricer=x["pricer"], **temporal)


@functools.lru_cache(maxsize=None)
def expectation(c):
    x = dict(inputs(c))
    x["e"] = run_stage(c)
    return x
