"""Deterministic (list 0, current, list 1) picture triples, records and operating points for the sa8d choice of a B picture's blocks and
for stages.Sa8dBFramePipeline (numpy and the oracle only, no torch).  192x128 = 3x2 CTUs, as in tests/intra_inter_cases.py.

The pictures are laid out in 32x32 cells, one kind per cell, four cells of every kind:
  M  plain motion (frames.synth_clip), every list matches
  A  only list 0 matches (list 1 shows other content)          B  only list 1 matches
  D  flat + noise in all three pictures: spurious vectors, the zero pair competes
  E  opposite patterns in the two references that only the coincident average cancels
  N  ramps, bars and flat areas the references lack (tests/intra_inter_cases.py's new content): intra wins with --b-intra; in every
     other row of cells list 0 shows that content under noise, so that the inter candidate intra beats is a single list there
The kinds are dealt so that every N cell has other kinds left of and above it.  tests/test_bsa8d_cpu.py asserts with the expectation
alone what the pictures reach; tests/test_gpu_bsa8d.py feeds the same cases to the kernels."""
import collections
import functools

import numpy as np

import bidir_expect as BE
import bsa8d_expect as BX
import intra_cases as IC
import intra_expect as IE
import intra_inter_cases as PC
import intra_inter_expect as IX
import qp_map_expect as QE

F, H = IE.F, IE.H
WIDTH, HEIGHT = 192, 128
RANGE, SUBME = 12, 2
CELLS = ("MANEBD",
         "NEMDNA",
         "BNDMEN",
         "EMANDB")


def cell_kind(yy, xx):
    table = np.array([[ord(c) for c in row] for row in CELLS])
    return table[(yy // 32) % 4, (xx // 32) % 6]


@functools.lru_cache(maxsize=None)
def pictures(depth, width=WIDTH, height=HEIGHT, seed=31):
    """((Y, Cb, Cr) list 0, current, list 1) of width x height."""
    clip = [[p.copy() for p in f] for f in F.synth_clip(width, height, 3, depth=depth, seed=seed)]
    other = F.synth_clip(width, height, 3, depth=depth, seed=seed + 1000)
    r = np.random.default_rng([seed, depth])
    sc, mx = 1 << (depth - 8), (1 << depth) - 1
    dt = clip[0][0].dtype

    def q(a):
        return np.clip(np.rint(a), 0, mx).astype(dt)
    for c in range(3):
        s = 1 if c == 0 else 2
        h, w = height // s, width // s
        yy, xx = np.mgrid[0:h, 0:w]
        kind = cell_kind(yy * s, xx * s)
        is_ = lambda ch: kind == ord(ch)
        clip[2][c][is_("A")] = other[2][c][is_("A")]
        clip[0][c][is_("B")] = other[0][c][is_("B")]
        if c == 0:
            for i in range(3):
                clip[i][c][is_("D")] = q(128 * sc + r.normal(0, 3.0 * sc, size=(h, w)))[is_("D")]
            # in every other row of cells list 1 shows other content instead: list 0 alone predicts the flat area, and DC beats its noise
            lone = is_("D") & ((yy // 32) % 2 == 1)
            clip[2][c][lone] = other[2][c][lone]
            e = np.rint(r.normal(0, 20.0 * sc, size=(h, w)))
            clip[0][c][is_("E")] = q(128 * sc + e)[is_("E")]
            clip[2][c][is_("E")] = q(128 * sc - e)[is_("E")]
            clip[1][c][is_("E")] = q(128 * sc + r.normal(0, 1.0 * sc, size=(h, w)))[is_("E")]
            new = sc * PC._new_content(yy, xx, 64)
            clip[1][c][is_("N")] = q(new)[is_("N")]
            # in every other row of cells list 0 shows the new content under noise: one list beats both, and intra beats that list
            near = is_("N") & ((yy // 32) % 2 == 0)
            clip[0][c][near] = q(new + r.normal(0, 8.0 * sc, size=(h, w)))[near]
        else:
            new = (100.0, 150.0)[c - 1] + 0.25 * PC._new_content(2 * yy, 2 * xx, 64) * (1 - 2 * (c - 1))
            clip[1][c][is_("N")] = q(sc * new)[is_("N")]
    return tuple(tuple(f) for f in clip)


def far_records(level, nctu, lst, seed=5):
    """Synthetic records of one list: vectors that walk through all 16 phases and reach the search range of 57 samples (into the padded
    border), zero vectors on every fifth block, costs that make either list the cheaper one - and equal costs on every seventh block."""
    nblk = 64 >> (2 * level)
    vec, cost = [], []
    for b in range(nctu * nblk):
        far = 4 * ((b * (7 + 4 * lst)) % 58) * (1 if (b + lst) % 2 else -1)
        qx, qy = far + (b + lst) % 4, -far // 2 + ((b // 4) + 2 * lst) % 4
        if b % 5 == lst:
            qx, qy = 0, 0
        if b % 10 == 3:
            qx, qy = 0, 0                                       # both lists zero: the zero pair is not tried
        if abs(qx) > 228:
            qx = 228 if qx > 0 else -228
        if b == 2:
            qx, qy = ((228, -227), (-226, 228))[lst]            # the search range itself, in both directions
        vec.append((qx, qy))
        cost.append(500 if b % 7 == 0 else 300 + ((b * (13 + 10 * lst)) % 400))
    mv = IX.mv_records(vec, level, nctu)
    lbase = (0, 64, 80)[level]
    for b, c in enumerate(cost):
        mv[(b // nblk) * 85 + lbase + b % nblk, 0] = c
    return mv


Case = collections.namedtuple("Case", "id depth level records lambda8 table_len maps width height hostile same_ref")


def _case(depth, level, records="searched", lambda8=IE.LAMBDA8, table_len=4 * 57 + 4, maps=None, width=WIDTH, height=HEIGHT, hostile=False, same_ref=False):
    name = f"d{depth}-l{level}-{records}" + ("" if lambda8 == IE.LAMBDA8 else f"-lam{lambda8}") + ("" if table_len == 232 else f"-t{table_len}") + \
           (f"-{maps}" if maps else "") + ("" if (width, height) == (WIDTH, HEIGHT) else f"-{width}x{height}") + ("-hostile" if hostile else "") + \
           ("-same" if same_ref else "")
    return Case(name, depth, level, records, lambda8, table_len, maps, width, height, hostile, same_ref)


SEARCHED_CASES = [_case(8, l) for l in (0, 1, 2)] + [_case(10, l) for l in (0, 1, 2)] + [_case(12, 1)]
FAR_CASES = [_case(8, 0, "far"), _case(8, 1, "far"), _case(8, 2, "far"), _case(10, 1, "far"), _case(10, 2, "far"), _case(12, 1, "far")]
POINT_CASES = [_case(8, 1, lambda8=0), _case(8, 2, "far", lambda8=0), _case(8, 1, maps="map-lambda"), _case(10, 0, "far", maps="map-lambda"),
               _case(8, 1, "far", table_len=100), _case(10, 2, "far", table_len=100)]
GRID_CASES = [_case(8, 1, "far", width=64, height=128), _case(8, 0, width=192, height=64), _case(8, 2, width=256, height=192)]
HOSTILE_CASES = [_case(8, 1, "far", hostile=True), _case(10, 0, "far", hostile=True), _case(12, 1, "far", hostile=True)]
TIE_CASES = [_case(8, l, "far", lambda8=0, same_ref=True) for l in (0, 1, 2)]
KERNEL_CASES = SEARCHED_CASES + FAR_CASES + POINT_CASES + GRID_CASES + HOSTILE_CASES + TIE_CASES


def hostile_lumas(depth, width, height):
    """Three luma pictures of black / white checker cells with a few grey samples: every filter sum leaves the sample range (the clips of
    the rounded pixel, of the 14-bit intermediate's addAvg and of nothing else must each land where the reference's do)."""
    mx = (1 << depth) - 1
    yy, xx = np.mgrid[0:height, 0:width]
    out = []
    for k in range(3):
        p = np.where(((xx + k) // (1 + k) + (yy // (2 + k))) % 2 == 0, mx, 0)
        p = np.where((xx * 7 + yy * 3 + k) % 11 == 0, mx // 2, p)
        out.append(p.astype(IE.harness.pix_dtype(depth)))
    return out


@functools.lru_cache(maxsize=None)
def kernel_expectation(c):
    """Everything the kernel is fed for a case and the decision expected of it: shared, never modified."""
    if c.hostile:
        ys = hostile_lumas(c.depth, c.width, c.height)
    else:
        pics = pictures(c.depth, c.width, c.height)
        ys = [p[0] for p in pics]
    if c.same_ref:
        ys[2] = ys[0]
    pl = [F.pad_plane(y) for y in ys]
    cur, stride, org, w64, h64 = pl[1]
    refs = (pl[0][0], pl[2][0])
    nctu = (w64 // 64) * (h64 // 64)
    if c.records == "far":
        recs = [far_records(c.level, nctu, 0), far_records(c.level, nctu, 0 if c.same_ref else 1)]
    else:
        recs = [BE.oracle_records(c.depth, cur, r, stride, org, w64, h64, RANGE, SUBME) for r in refs]
    qp = 30 + 6 * (c.depth - 8)
    tu_qp = np.tile(PC.tu_qp_map(c.depth, c.level), (1, 2, 2))[:, :h64 // 8, :w64 // 8].copy() if c.maps else None
    lam_tab = QE.lambda8_table(c.depth) if c.maps == "map-lambda" else None
    table = IX.s_bitsizes(c.table_len)
    e = BX.decide(c.depth, cur, refs, w64, h64, c.level, recs, lambda8=c.lambda8, table=table, qp=qp, tu_qp=tu_qp, lambda8_by_qp=lam_tab, with_reference=False)
    return dict(ys=ys, cur=cur, refs=refs, stride=stride, org=org, w64=w64, h64=h64, nctu=nctu, recs=recs, qp=qp, tu_qp=tu_qp, lambda8_by_qp=lam_tab,
                table=table, e=e)


def run_decide(c, mutation=None, with_reference=False):
    x = kernel_expectation(c)
    return BX.decide(c.depth, x["cur"], x["refs"], x["w64"], x["h64"], c.level, x["recs"], lambda8=c.lambda8, table=x["table"], qp=x["qp"],
                     tu_qp=x["tu_qp"], lambda8_by_qp=x["lambda8_by_qp"], mutation=mutation, with_reference=with_reference)


@functools.lru_cache(maxsize=None)
def bidir_decision(c):
    """What bidir_expect.expect (x265hip_bidir_decide's expectation) gives for the same records."""
    x = kernel_expectation(c)
    cq, qoff = F.qpel_cost_table(57 if c.records == "far" else RANGE, 4.0)
    phases = [BE.phases_of(c.depth, r, x["stride"]) for r in x["refs"]]
    return BE.expect(c.depth, x["cur"], x["stride"], x["org"], x["w64"], x["h64"], c.level, x["recs"], phases, cq, qoff, with_reference=False)


@functools.lru_cache(maxsize=None)
def intra_expectation(level, depth=8, ties=False):
    """The b_intra part on the searched records: the bi-predictive coding of the decision and the intra walk on top of it."""
    c = _case(depth, level)
    x = kernel_expectation(c)
    pics = pictures(depth)
    pad = [PC.padded(p) for p in pics]
    qp, lambda8, mode_bits = IC.point("mid", depth)
    qpc = IC.chroma_qp(qp, depth)
    it = BX.inter_coding(depth, pad[1], (pad[0], pad[2]), x["w64"], x["h64"], level, x["e"], qp, (qpc, qpc), H.TU_SIGN_HIDE)
    w = IX.walk(depth, pad[1], x["w64"], x["h64"], level, qp, it, qp_c=(qpc, qpc), flags=H.TU_SIGN_HIDE, lambda8=lambda8, mode_bits=mode_bits,
                cost_fn=IX.tie_pattern if ties else None)
    return dict(x, pad=pad, qp_i=qp, qp_c=(qpc, qpc), lambda8=lambda8, mode_bits=mode_bits, inter=it, walk=w, masks=BX.intra_masks(x["e"], w, x["w64"], level))
