"""Deterministic inputs for the loop-filter tests (numpy and the oracle only, no torch): deblocking and SAO at the limits of their
arithmetic and at both ends of the QP range, and the censuses - plain numpy restatements that count how often each path is taken.

SAO: pictures whose differences source - deblocked are +-(2^depth - 1) over whole runs, wavefronts and CTUs (the packed
accumulators of the statistics kernel at their last bit), statistics and lambdas at QP 0 and 51 for the decision walk, parameter
sets with the largest offsets and the last band positions for the application.  Deblocking: block steps scaled by tc(qp) with noise
scaled by beta(qp) at QP 0 .. 51 over base 0, mid-grey and max, ramps for the strong filter's 2 tc clip, QP maps whose means round,
chroma QP offsets of +-12.

tests/test_loopfilter_cases_cpu.py asserts, with the oracle alone, that every case below reaches what it is listed for and pins the
oracle against the real classes on these inputs; tests/test_gpu_loopfilter_cases.py feeds the same cases to the kernels."""
import functools
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")

DEPTHS = (8, 10, 12)
FAMILIES = ("flat", "flatneg", "rows", "rowsneg", "cols", "checker", "mixed")
LUMA_SIZES = ((128, 128), (70, 66))            # 2 x 2 CTUs: every combination of startX / startY and of the skipped right / bottom strips
CHROMA_SIZES = ((64, 64), (35, 33))            # the same on the 32 x 32 footprint (four samples per lane)
CHROMA_MARGIN = 48


def oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def pixel_type(depth):
    return np.uint8 if depth == 8 else np.uint16


def sao_lim(depth):
    """OFFSET_THRESH - 1: the largest offset the decision can choose and the bitstream can carry."""
    return (1 << min(depth - 5, 5)) - 1


def pad_any(img, margin):
    """A plane of any size inside `margin` zero samples: (flat buffer, stride, element offset of sample (0, 0))."""
    h, w = img.shape
    buf = np.zeros((h + 2 * margin, w + 2 * margin), dtype=img.dtype)
    buf[margin:margin + h, margin:margin + w] = img
    return np.ascontiguousarray(buf).reshape(-1), w + 2 * margin, margin * (w + 2 * margin) + margin


def inner(buf, stride, org, width, height):
    """The picture area of a flat padded plane."""
    return buf.reshape(-1, stride)[org // stride:org // stride + height, org % stride:org % stride + width]


# ---- SAO pictures ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sao_picture(family, depth, width, height, seed=1, tile=64):
    """(source, deblocked) of one plane; read only.  mx = 2^depth - 1:
    flat / flatneg: every difference +mx / -mx, every edge class 0, one band;  rows / rowsneg / cols: deblocked = y & 1 (x & 1), so
    the edge types across the stripes put whole runs into the classes 1 and 4 with differences mx, mx - 1;  checker: differences of
    +-mx next to each other;  mixed: seeded, source in {0, mx}, deblocked in {0, 1, mx - 1, mx} per sample;  zero: deblocked ==
    source;  identical: every CTU (`tile`) the same mixed tile, so the merge candidates tie with the CTU's own choice."""
    mx = (1 << depth) - 1
    yy, xx = np.mgrid[0:height, 0:width]
    rng = np.random.default_rng([71, depth, width, height, seed])

    def mixed(h, w):
        return rng.integers(0, 2, size=(h, w)) * mx, np.array([0, 1, mx - 1, mx])[rng.integers(0, 4, size=(h, w))]

    if family == "flat":
        src, rec = np.full((height, width), mx), np.zeros((height, width), np.int64)
    elif family == "flatneg":
        src, rec = np.zeros((height, width), np.int64), np.full((height, width), mx)
    elif family == "rows":
        src, rec = np.full((height, width), mx), yy & 1
    elif family == "rowsneg":
        src, rec = np.zeros((height, width), np.int64), mx - (yy & 1)
    elif family == "cols":
        src, rec = np.full((height, width), mx), xx & 1
    elif family == "checker":
        rec = ((xx + yy) & 1) * mx
        src = mx - rec
    elif family == "mixed":
        src, rec = mixed(height, width)
    elif family == "zero":
        rec = mixed(height, width)[1]
        src = rec
    elif family == "identical":
        s, r = mixed(tile, tile)
        reps = ((height + tile - 1) // tile, (width + tile - 1) // tile)
        src, rec = np.tile(s, reps)[:height, :width], np.tile(r, reps)[:height, :width]
    else:
        raise ValueError(family)
    dt = pixel_type(depth)
    src, rec = np.ascontiguousarray(src.astype(dt)), np.ascontiguousarray(rec.astype(dt))
    src.setflags(write=False); rec.setflags(write=False)
    return src, rec


SAO_STAT_CASES = [SimpleNamespace(id=f"{fam}-d{d}-{fp}-{w}x{h}", family=fam, depth=d, width=w, height=h, ctu=ctu, plane_offset=po)
                  for d in DEPTHS for fp, sizes, ctu, po in (("luma", LUMA_SIZES, (64, 64), 0), ("chroma", CHROMA_SIZES, (32, 32), 2))
                  for (w, h) in sizes for fam in FAMILIES]


@functools.lru_cache(maxsize=None)
def _sao_plane_cached(family, depth, width, height, ctu0, seed):
    src, rec = sao_picture(family, depth, width, height, seed, tile=ctu0)
    if ctu0 == 64:
        sp, stride, org, _, _ = F.pad_plane(src)
        rp = F.pad_plane(rec)[0]
        sp, rp = sp.reshape(-1), rp.reshape(-1)
    else:
        sp, stride, org = pad_any(src, CHROMA_MARGIN)
        rp = pad_any(rec, CHROMA_MARGIN)[0]
    sp.setflags(write=False); rp.setflags(write=False)
    return SimpleNamespace(src=src, rec=rec, src_plane=sp, rec_plane=rp, stride=stride, org=org)


def sao_plane(case, seed=1):
    """The padded planes of a statistics / application case: luma footprints in the frames.pad_plane geometry, the 32 x 32 footprint
    inside a zero margin.  Shared between tests: read only."""
    return _sao_plane_cached(case.family, case.depth, case.width, case.height, case.ctu[0], seed)


_EO_TABLE = np.array([1, 2, 0, 3, 4])
_EO_STEP = ((0, 1), (1, 0), (1, 1), (1, -1))          # (dy, dx) of the second neighbour; the first one lies opposite


def sao_classes(rec):
    """Edge class 0 .. 4 of every sample for the four edge types (int [4, h, w]; the picture's outermost samples are classified against a
    replicated border and never counted) and its band."""
    r = np.pad(rec.astype(np.int64), 1, mode="edge")
    h, w = rec.shape
    c = r[1:-1, 1:-1]
    out = np.zeros((4, h, w), np.int64)
    for t, (dy, dx) in enumerate(_EO_STEP):
        a = r[1 - dy:1 - dy + h, 1 - dx:1 - dx + w]
        b = r[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        out[t] = _EO_TABLE[np.sign(c - a) + np.sign(c - b) + 2]
    return out


def sao_counted(width, height, ctu, plane_offset, lx, ty):
    """bool [5, ch, cw]: the samples of the CTU at (lx, ty) that calcSaoStatsCTU counts for EO_0 .. EO_3 and BO (sao.cpp:806-915)."""
    rx, by = min(lx + ctu[0], width), min(ty + ctu[1], height)
    cw, ch = rx - lx, by - ty
    at_right, at_bottom = rx == width, by == height
    skip_r, skip_b = 5 - plane_offset, 4 - plane_offset
    y, x = np.mgrid[0:ch, 0:cw]
    start_x, end_x = int(lx == 0), (cw - 1 if at_right else cw - skip_r)
    start_y, end_y = int(ty == 0), (ch - 1 if at_bottom else ch - skip_b)
    all_x = x < (cw if at_right else cw - skip_r)
    ex, ey = (x >= start_x) & (x < end_x), (y >= start_y) & (y < end_y)
    return np.stack([ex & (y < ch - skip_b), all_x & ey, ex & ey, ex & ey, all_x & (y < (ch if at_bottom else ch - skip_b))])


def sao_census(depth, src, rec, ctu, plane_offset):
    """count / offsetOrg [nctu, 5, 32] from a per-sample classification, and how far the packed accumulators of the statistics kernel are
    filled: a lane owns `spl` consecutive samples of a CTU row (16, or 4 on a footprint up to 32 x 32), the 8-bit route adds runs of
    `run` = min(spl, 8) samples into 4 + 12-bit fields of the classes 1 .. 4 (class 0 = totals - those) and reduces the 1024 samples of a
    wavefront (16 rows x 64 columns) in one word.  All figures are for differences of exactly +mx, the largest biased sum."""
    height, width = rec.shape
    mx = (1 << depth) - 1
    d = src.astype(np.int64) - rec.astype(np.int64)
    eo = sao_classes(rec)
    band = rec.astype(np.int64) >> (depth - 5)
    cws, chs = (width + ctu[0] - 1) // ctu[0], (height + ctu[1] - 1) // ctu[1]
    count, org = np.zeros((cws * chs, 5, 32), np.int32), np.zeros((cws * chs, 5, 32), np.int32)
    spl = 16 if ctu[0] > 32 else 4
    run = min(spl, 8)
    m = SimpleNamespace(full_run_class14=0, full_run_class0=0, full_wave=0, full_lane=0, run=run, spl=spl)
    for addr in range(cws * chs):
        lx, ty = (addr % cws) * ctu[0], (addr // cws) * ctu[1]
        counted = sao_counted(width, height, ctu, plane_offset, lx, ty)
        ch, cw = counted.shape[1:]
        dd = d[ty:ty + ch, lx:lx + cw]
        for t in range(5):
            cls = band[ty:ty + ch, lx:lx + cw] if t == 4 else eo[t, ty:ty + ch, lx:lx + cw]
            sel = counted[t]
            count[addr, t] = np.bincount(cls[sel], minlength=32)
            org[addr, t] = np.bincount(cls[sel], weights=dd[sel], minlength=32).astype(np.int64)
            if t == 4:
                continue
            top = sel & (dd == mx)                                 # counted samples with the largest biased difference
            for k in range(5):
                hit = np.zeros((ctu[1], ctu[0]), bool)
                hit[:ch, :cw] = top & (cls == k)
                runs = hit.reshape(ctu[1], ctu[0] // run, run).all(axis=2).sum()
                if k:
                    m.full_run_class14 += int(runs)
                else:
                    m.full_run_class0 += int(runs)
                m.full_lane += int(hit.reshape(ctu[1], ctu[0] // spl, spl).all(axis=2).sum())
                if ctu[0] == 64:
                    m.full_wave += int(hit.reshape(4, 16, 64).all(axis=(1, 2)).sum())
    return count, org, m


# ---- SAO decision ------------------------------------------------------------------------------------------------------------------------
DECISION_PICTURES = FAMILIES + ("zero", "identical")
PARTNER = {"flat": "flatneg", "flatneg": "flat", "rows": "rowsneg", "rowsneg": "rows", "cols": "rows", "checker": "checker", "mixed": "mixed",
            "zero": "zero", "identical": "identical"}


@functools.lru_cache(maxsize=None)
def decision_picture(family, depth, width=128, height=128):
    """Y, Cb, Cr (source, deblocked) of a 4:2:0 picture in the PicYuv layout (frames.pad_plane / pad_chroma): Cb is of the luma's family,
    Cr of its counterpart, so the two chroma planes - which share a type - pull in different directions."""
    fams = (family, family, PARTNER[family])
    pics = [sao_picture(fams[c], depth, width >> (c > 0), height >> (c > 0), seed=2 + c, tile=64 >> (c > 0)) for c in range(3)]
    sp, stride, org, w64, h64 = F.pad_plane(pics[0][0])
    src, rec = [sp], [F.pad_plane(pics[0][1])[0]]
    for c in (1, 2):
        b, stride_c, org_c = F.pad_chroma(pics[c][0], w64, h64)
        src.append(b); rec.append(F.pad_chroma(pics[c][1], w64, h64)[0])
    for a in src + rec:
        a.setflags(write=False)
    return SimpleNamespace(src=src, rec=rec, stride=stride, org=org, stride_c=stride_c, org_c=org_c, width=width, height=height, w64=w64, h64=h64,
                           depth=depth, ctus_w=w64 // 64, ctus_h=h64 // 64)


@functools.lru_cache(maxsize=None)
def decision_stats(family, depth):
    """The oracle's statistics of the three planes of decision_picture: (counts, offset_orgs), lists of int32 [nctu, 5, 32]."""
    O = oracle()
    p = decision_picture(family, depth)
    c0, o0 = O.sao_stats(depth, p.src[0], p.rec[0], p.stride, p.org, p.width, p.height)
    counts, orgs = [c0], [o0]
    for c in (1, 2):
        cc, oo = O.sao_stats(depth, p.src[c], p.rec[c], p.stride_c, p.org_c, p.width // 2, p.height // 2, ctu=(32, 32), plane_offset=2)
        counts.append(cc); orgs.append(oo)
    return counts, orgs


@functools.lru_cache(maxsize=None)
def raw_stats(depth, nctu, seed):
    """Statistics written directly: counts in [0, 4096] with 30 % zeros, |offsetOrg| <= count * mx - what a picture can produce, so that the
    int products of the decision stay inside int - with offsetOrg = +-count * mx exactly in one class in eight."""
    rng = np.random.default_rng([73, depth, nctu, seed])
    mx = (1 << depth) - 1
    counts, orgs = [], []
    for _ in range(3):
        n = rng.integers(0, 4097, size=(nctu, 5, 32))
        n[rng.random(n.shape) < 0.3] = 0
        e = np.rint(n * mx * rng.uniform(-1, 1, size=n.shape) * rng.choice([1.0, 0.05, 0.002], size=n.shape)).astype(np.int64)
        full = rng.random(n.shape) < 0.125
        e = np.where(full, n * mx * rng.choice([-1, 1], size=n.shape), e)
        for (a, t, k), sign in (((0, 4, 3), 1), ((0, 1, 1), 1), ((0, 1, 4), -1), ((nctu - 1, 4, 30), -1), ((nctu - 1, 2, 2), 1), ((nctu - 1, 2, 3), -1)):
            n[a, t, k], e[a, t, k] = 4096, sign * 4096 * mx               # a whole CTU in one class at the largest difference
        n[:, :4, 5:] = 0
        e[:, :4, 5:] = 0
        assert (np.abs(e) <= n * mx).all()
        counts.append(n.astype(np.int32)); orgs.append(e.astype(np.int32))
    return counts, orgs


@functools.lru_cache(maxsize=None)
def tables():
    return HT.load()


def decision_cases(depth):
    """Every decision picture at QP 0 and 51, three planes and luma only, the slice types B / P / I in turn; one mixed picture whose CTUs
    alternate between the lambdas of QP 0 and QP 51; raw statistics on 2 x 2 and 1 x 6 CTU grids."""
    out, i = [], 0
    for fam in DECISION_PICTURES:
        for qp in (0, 51):
            for planes in (3, 1):
                out.append(SimpleNamespace(id=f"{fam}-d{depth}-qp{qp}-p{planes}", kind="picture", family=fam, depth=depth, qp=qp, ctu_qp=None, planes=planes,
                                           slice_type=i % 3, ctus_w=2, ctus_h=2))
                i += 1
    out.append(SimpleNamespace(id=f"mixed-d{depth}-alternating", kind="picture", family="mixed", depth=depth, qp=26, ctu_qp=(0, 51, 51, 0), planes=3,
                               slice_type=1, ctus_w=2, ctus_h=2))
    for (cw, ch), qp, st, planes in (((2, 2), 0, 0, 3), ((2, 2), 51, 2, 3), ((6, 1), 0, 1, 3), ((6, 1), 51, 0, 1), ((1, 6), 30, 2, 3), ((1, 6), 51, 1, 3)):
        out.append(SimpleNamespace(id=f"raw-d{depth}-{cw}x{ch}-qp{qp}-p{planes}", kind="raw", family=None, depth=depth, qp=qp, ctu_qp=None, planes=planes,
                                   slice_type=st, ctus_w=cw, ctus_h=ch))
    return out


def decision_inputs(case):
    """(counts, offset_orgs, lambda_ctu int64 [nctu, 2], ctx_merge, ctx_type, sao_flag) of a decision case, statistics from the oracle."""
    nctu = case.ctus_w * case.ctus_h
    counts, orgs = decision_stats(case.family, case.depth) if case.kind == "picture" else raw_stats(case.depth, nctu, case.qp)
    qps = case.ctu_qp if case.ctu_qp is not None else (case.qp,) * nctu
    lam = np.array([HT.sao_lambdas(tables(), int(q), csp400=case.planes == 1) for q in qps], dtype=np.int64)
    ctx_m, ctx_t = HT.sao_contexts(case.slice_type, case.qp)
    return counts[:case.planes], orgs[:case.planes], lam, ctx_m, ctx_t, (1, 1 if case.planes == 3 else 0)


def decide(case):
    """The oracle's decision of a case: (params per plane, numNoSao)."""
    counts, orgs, lam, ctx_m, ctx_t, flag = decision_inputs(case)
    return oracle().sao_rdo(case.depth, counts, orgs, case.ctus_w, case.ctus_h, lam, ctx_m, ctx_t, tables()["entropy_bits"], sao_flag=flag)


# ---- SAO application ---------------------------------------------------------------------------------------------------------------------
APPLY_FAMILIES = ("flat", "flatneg", "checker", "mixed")
SAO_APPLY_CASES = [c for c in SAO_STAT_CASES if c.family in APPLY_FAMILIES]


def apply_param_sets(depth, ctus_w, ctus_h):
    """Per-CTU parameter sets int32 [nctu, 7] with offsets of +-lim only: every edge type with either sign in every class, the band
    positions 0, 28 and 31 (the window wraps to the bands 31, 0, 1, 2), and merge-left CTUs that carry their left neighbour's values."""
    lim, nctu = sao_lim(depth), ctus_w * ctus_h
    sets = []
    for k in range(4):
        p = np.zeros((nctu, 7), np.int32)
        for a in range(nctu):
            p[a, 0] = (a + k) % 4
            p[a, 2:6] = np.roll([lim, lim, -lim, -lim], a + k)
        sets.append(p)
    for k, sign in ((0, 1), (1, -1), (2, 1)):
        p = np.zeros((nctu, 7), np.int32)
        for a in range(nctu):
            p[a, 0] = 4
            p[a, 1] = (0, 28, 31)[(a + k) % 3]
            p[a, 2:6] = sign * np.array([lim, -lim, lim, -lim]) if a % 2 else sign * lim
        sets.append(p)
    for p in sets[1::2]:
        for a in range(nctu):
            if a % ctus_w:
                p[a] = p[a - 1]
                p[a, 6] = 1
    return sets


def apply_census(depth, rec, out, params, ctu):
    """A numpy restatement of the application (`out` = the oracle's picture, compared by the caller with the first value returned): the
    offset picture, the samples that an offset pushed past 0 / past mx, and the changed samples per edge type and class (int [4, 5])."""
    mx = (1 << depth) - 1
    h, w = rec.shape
    cws = (w + ctu[0] - 1) // ctu[0]
    eo = sao_classes(rec)
    band = rec.astype(np.int64) >> (depth - 5)
    yy, xx = np.mgrid[0:h, 0:w]
    inside_x, inside_y = (xx > 0) & (xx < w - 1), (yy > 0) & (yy < h - 1)
    raw = rec.astype(np.int64)
    changed = np.zeros((4, 5), np.int64)
    for a in range(params.shape[0]):
        ys, xs = slice((a // cws) * ctu[1], (a // cws + 1) * ctu[1]), slice((a % cws) * ctu[0], (a % cws + 1) * ctu[0])
        t = int(params[a, 0])
        if t < 0:
            continue
        if t == 4:
            idx = (band[ys, xs] - int(params[a, 1])) & 31
            off = np.where(idx < 4, params[a, 2:6][np.minimum(idx, 3)], 0)
        else:
            dy, dx = _EO_STEP[t]
            ok = (inside_x[ys, xs] if dx else True) & (inside_y[ys, xs] if dy else True)
            off = np.where(ok, np.concatenate([[0], params[a, 2:6]])[eo[t][ys, xs]], 0)
            for k in range(5):
                changed[t, k] += int(((eo[t][ys, xs] == k) & (out[ys, xs] != rec[ys, xs])).sum())
        raw[ys, xs] += off
    return np.clip(raw, 0, mx).astype(rec.dtype), int((raw < 0).sum()), int((raw > mx).sum()), changed


# ---- deblocking --------------------------------------------------------------------------------------------------------------------------
BETA_TABLE = np.array([0] * 16 + list(range(6, 19)) + list(range(20, 66, 2)))
TC_TABLE = np.array([0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24])
CHROMA_SCALE = np.array(list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37] + list(range(38, 52)) + [51] * 12)
assert BETA_TABLE.size == 52 and TC_TABLE.size == 54 and CHROMA_SCALE.size == 70
DB_W, DB_H = 128, 64
DB_QPS = (0, 15, 16, 17, 18, 30, 51)
LUMA_COUNTERS = ("beta_skip", "strong", "normal", "line_skip", "tc_clip", "p1_on", "p1_off", "tc2_clip", "clip_0", "clip_max", "tc0_pass", "strong_clip")
CHROMA_COUNTERS = ("clip_0", "clip_max", "tc_clip", "index_negative", "index_table", "index_63")


def bs_maps(variant, width, height, seed=0):
    """(bs_ver [h / 4, w / 8], bs_hor [h / 8, w / 4]) flat uint8, the picture's first column / row 0: all 1, all 2 or random {0, 1, 2}."""
    rng = np.random.default_rng([79, seed, width])
    shapes = ((height // 4, width // 8), (height // 8, width // 4))
    if variant == "random":
        bv, bh = [rng.integers(0, 3, size=s).astype(np.uint8) for s in shapes]
    else:
        bv, bh = [np.full(s, int(variant), np.uint8) for s in shapes]
    bv[:, 0] = 0
    bh[0, :] = 0
    return bv.reshape(-1), bh.reshape(-1)


def qp_map_extremes(width, height, seed=0):
    """int8 [h / 8, w / 8]: 0 next to 51 (mean 26 after rounding 25.5 up), 50 next to 51 (51), and 15 / 16 / 17 / 18 neighbours around the
    first non-zero beta and tc."""
    rng = np.random.default_rng([83, seed])
    vals = np.array([0, 51, 50, 51, 16, 17, 15, 18, 51, 0, 30, 51])
    m = vals[(np.arange(width // 8)[None, :] + 5 * np.arange(height // 8)[:, None]) % vals.size]
    m = np.where(rng.random(m.shape) < 0.2, rng.integers(0, 52, size=m.shape), m)
    return np.ascontiguousarray(m.astype(np.int8))


@functools.lru_cache(maxsize=None)
def deblock_picture(kind, depth, qp, base, seed=0):
    """128 x 64 luma, read only.  steps: a DC level per 8 x 8 block drawn from +-12 tc(qp) plus per-block noise of amplitude 0, 1, beta / 16,
    beta / 6 or beta / 2, over base 0 / mid / max (clipped into range);  ramps: per block slope * |x - k| (or |y - k|) with slopes of up to
    3 << (depth - 8) - smooth on both sides of an edge, which the strong filter then moves by more than 2 tc."""
    rng = np.random.default_rng([89, depth, qp, seed, {"zero": 0, "mid": 1, "max": 2}[base]])
    shift, mx = depth - 8, (1 << depth) - 1
    b0 = {"zero": 0, "mid": 1 << (depth - 1), "max": mx}[base]
    bh, bw = DB_H // 8, DB_W // 8
    if kind == "steps":
        tc = max(int(TC_TABLE[min(qp + 2, 53)]), 1) << shift
        beta = max(int(BETA_TABLE[qp]), 6) << shift
        dc = rng.integers(-12 * tc, 12 * tc + 1, size=(bh, bw))
        amp = np.array([0, 1, beta // 16, beta // 6, beta // 2])[rng.integers(0, 5, size=(bh, bw))]
        noise = np.rint(rng.uniform(-1, 1, size=(DB_H, DB_W)) * np.kron(amp, np.ones((8, 8)))).astype(np.int64)
        img = b0 + np.kron(dc, np.ones((8, 8), np.int64)) + noise
    else:
        slope = rng.integers(-3, 4, size=(bh, bw)) << shift
        k = rng.integers(0, 8, size=(bh, bw))
        along_y = rng.random((bh, bw)) < 0.5
        yy, xx = np.mgrid[0:DB_H, 0:DB_W]
        kk, ss, ay = [np.kron(a, np.ones((8, 8), np.int64)) for a in (k, slope, along_y.astype(np.int64))]
        img = b0 + ss * np.abs(np.where(ay, yy & 7, xx & 7) - kk) + (rng.integers(-1, 2, size=(bh, bw)) << shift).repeat(8, axis=0).repeat(8, axis=1)
    img = np.ascontiguousarray(np.clip(img, 0, mx).astype(pixel_type(depth)))
    img.setflags(write=False)
    return img


def luma_cases(depth):
    """(picture kind, base, qp, Bs variant, beta offset / 2, tc offset / 2, with QP map)."""
    out = []
    for qp in DB_QPS:
        for base in ("zero", "mid", "max"):
            for bs in ("1", "2", "random"):
                out.append(SimpleNamespace(kind="steps", base=base, qp=qp, bs=bs, bo=0, to=0, qmap=False))
    for qp in (30, 38):
        for bs in ("1", "2"):
            out.append(SimpleNamespace(kind="ramps", base="mid", qp=qp, bs=bs, bo=6, to=-6, qmap=False))
    for qp, bo, to in ((51, -6, 6), (0, 6, -6)):
        for bs in ("1", "2", "random"):
            out.append(SimpleNamespace(kind="steps", base="mid", qp=qp, bs=bs, bo=bo, to=to, qmap=False))
    for base in ("zero", "mid", "max"):
        out.append(SimpleNamespace(kind="steps", base=base, qp=30, bs="random", bo=0, to=0, qmap=True))
    for c in out:
        c.depth = depth
        c.id = f"{c.kind}-d{depth}-{c.base}-qp{c.qp}-bs{c.bs}-o{c.bo}{c.to:+d}" + ("-map" if c.qmap else "")
    return out


def luma_inputs(case):
    """(padded plane 2-D, stride, org, bs_ver, bs_hor, qp map or None) of a luma case; the plane is shared: read only."""
    img = deblock_picture(case.kind, case.depth, case.qp, case.base)
    plane, stride, org, _, _ = F.pad_plane(img)
    bv, bh = bs_maps(case.bs, DB_W, DB_H, seed=case.qp)
    return plane, stride, org, bv, bh, (qp_map_extremes(DB_W, DB_H) if case.qmap else None)


def _edge_pass(img, bs, qpu, depth, bo, to, cnt):
    """edgeFilterLuma for every vertical edge of img (int64 [h, w], in place); bs / qpu [h / 4, w / 8] per unit of 4 rows.  The units of one
    direction touch disjoint samples (3 on each side of an edge, edges 8 apart, reads reach 4), so they are filtered together."""
    h, w = img.shape
    shift, mx = depth - 8, (1 << depth) - 1
    T = img[:, 4:w - 4].reshape(h // 4, 4, w // 8 - 1, 8).transpose(0, 2, 1, 3).copy()          # [unit, edge, line, tap]: taps -4 .. 3 around the edge
    b, q = bs[:, 1:].astype(np.int64), qpu[:, 1:].astype(np.int64)
    m = [T[..., t] for t in range(8)]
    beta = BETA_TABLE[np.clip(q + bo, 0, 51)] << shift
    dp = np.abs(m[1] - 2 * m[2] + m[3])
    dq = np.abs(m[4] - 2 * m[5] + m[6])
    d0, d3 = dp[..., 0] + dq[..., 0], dp[..., 3] + dq[..., 3]
    on = b > 0
    go = on & (d0 + d3 < beta)
    cnt["beta_skip"] += int((on & ~go).sum())
    tc = TC_TABLE[np.clip(q + 2 * (b - 1) + to, 0, 53)] << shift
    cnt["tc0_pass"] += int((go & (tc == 0)).sum())
    sl = (np.abs(m[0] - m[3]) + np.abs(m[7] - m[4]) < (beta >> 3)[..., None]) & (np.abs(m[3] - m[4]) < ((tc * 5 + 1) >> 1)[..., None])
    strong = go & (2 * d0 < (beta >> 2)) & (2 * d3 < (beta >> 2)) & sl[..., 0] & sl[..., 3]
    normal = go & ~strong
    cnt["strong"] += int(strong.sum()); cnt["normal"] += int(normal.sum())
    new = [x.copy() for x in m]
    # strong filter: every tap moves by at most 2 tc
    t2 = (2 * tc)[..., None]
    S = strong[..., None] & np.ones(4, bool)
    tgt = {1: (2 * m[0] + 3 * m[1] + m[2] + m[3] + m[4] + 4) >> 3, 2: (m[1] + m[2] + m[3] + m[4] + 2) >> 2, 3: (m[1] + 2 * m[2] + 2 * m[3] + 2 * m[4] + m[5] + 4) >> 3,
           4: (m[2] + 2 * m[3] + 2 * m[4] + 2 * m[5] + m[6] + 4) >> 3, 5: (m[3] + m[4] + m[5] + m[6] + 2) >> 2, 6: (m[3] + m[4] + m[5] + 3 * m[6] + 2 * m[7] + 4) >> 3}
    for t, v in tgt.items():
        dlt = v - m[t]
        cl = np.clip(dlt, -t2, t2)
        cnt["strong_clip"] += int((S & (cl != dlt)).sum())
        new[t] = np.where(S, m[t] + cl, new[t])
    # normal filter
    side = (beta + (beta >> 1)) >> 3
    mp = (dp[..., 0] + dp[..., 3] < side)[..., None]
    mq = (dq[..., 0] + dq[..., 3] < side)[..., None]
    tcl, tc2 = tc[..., None], (tc >> 1)[..., None]
    delta = (9 * (m[4] - m[3]) - 3 * (m[5] - m[2]) + 8) >> 4
    N = normal[..., None] & np.ones(4, bool)
    line = N & (np.abs(delta) < 10 * tcl)
    cnt["line_skip"] += int((N & ~line).sum())
    dc = np.clip(delta, -tcl, tcl)
    cnt["tc_clip"] += int((line & (dc != delta)).sum())
    cnt["p1_on"] += int((line & mp).sum() + (line & mq).sum())
    cnt["p1_off"] += int((line & ~mp).sum() + (line & ~mq).sum())
    d1p = (((m[1] + m[3] + 1) >> 1) - m[2] + dc) >> 1
    d1q = (((m[6] + m[4] + 1) >> 1) - m[5] - dc) >> 1
    c1p, c1q = np.clip(d1p, -tc2, tc2), np.clip(d1q, -tc2, tc2)
    cnt["tc2_clip"] += int((line & mp & (c1p != d1p)).sum() + (line & mq & (c1q != d1q)).sum())
    for t, v, sel in ((3, m[3] + dc, line), (4, m[4] - dc, line), (2, m[2] + c1p, line & mp), (5, m[5] + c1q, line & mq)):
        cnt["clip_0"] += int((sel & (v < 0)).sum()); cnt["clip_max"] += int((sel & (v > mx)).sum())
        new[t] = np.where(sel, np.clip(v, 0, mx), new[t])
    img[:, 4:w - 4] = np.stack(new, axis=-1).transpose(0, 2, 1, 3).reshape(h, w - 8)


def unit_qps(qp, qmap, width, height):
    """QP of every unit of the vertical pass [h / 4, w / 8] and, transposed, of the horizontal pass [w / 4, h / 8]: the rounded mean of the two
    sides' 8 x 8 blocks."""
    if qmap is None:
        return np.full((height // 4, width // 8), qp), np.full((width // 4, height // 8), qp)
    qm = np.asarray(qmap, np.int64).reshape(height // 8, width // 8)

    def mean_left(a):
        out = np.zeros_like(a)
        out[:, 1:] = (a[:, :-1] + a[:, 1:] + 1) >> 1
        return out
    return mean_left(qm).repeat(2, axis=0), mean_left(qm.T.copy()).repeat(2, axis=0)


def luma_census(depth, img, bv, bh, qp, qmap=None, bo=0, to=0):
    """A numpy restatement of Deblock::edgeFilterLuma over a picture (deblock.cpp:317-415; vertical edges, then horizontal ones): the filtered
    picture and, per direction, how many units / lines / samples took each path (LUMA_COUNTERS)."""
    h, w = img.shape
    work = img.astype(np.int64)
    qv, qh = unit_qps(qp, qmap, w, h)
    counts = [dict.fromkeys(LUMA_COUNTERS, 0) for _ in range(2)]
    _edge_pass(work, bv.reshape(h // 4, w // 8), qv, depth, 2 * bo, 2 * to, counts[0])
    wt = np.ascontiguousarray(work.T)
    _edge_pass(wt, np.ascontiguousarray(bh.reshape(h // 8, w // 4).T), qh, depth, 2 * bo, 2 * to, counts[1])
    return np.ascontiguousarray(wt.T).astype(img.dtype), counts


CHROMA_QPS = ((0, -12, 12), (51, 12, -12), (29, 0, 1), (30, 0, -1), (18, -12, 12))


@functools.lru_cache(maxsize=None)
def chroma_picture(depth, base, seed):
    """Cb, Cr of a 128 x 64 4:2:0 picture: a step per 8 x 8 chroma block of up to +-6 << (depth - 8) over base 0 / max, read only.  Half the
    blocks carry per-sample noise of the same amplitude: between flat blocks the filter moves both sides towards each other and cannot
    leave the range, a sample at 0 next to an edge whose second neighbour is not can."""
    rng = np.random.default_rng([97, depth, seed, base == "max"])
    mx = (1 << depth) - 1
    out = []
    for c in range(2):
        steps = rng.integers(-6, 7, size=(DB_H // 16, DB_W // 16)) << (depth - 8)
        noisy = np.kron(rng.integers(0, 2, size=steps.shape), np.ones((8, 8), np.int64))
        noise = noisy * (rng.integers(-6, 7, size=(DB_H // 2, DB_W // 2)) << (depth - 8))
        img = np.clip((mx if base == "max" else 0) + np.kron(steps, np.ones((8, 8), np.int64)) + noise, 0, mx).astype(pixel_type(depth))
        img.setflags(write=False)
        out.append(np.ascontiguousarray(img))
    return out


def chroma_cases(depth):
    out = []
    for i, (qp, cb, cr) in enumerate(CHROMA_QPS):
        for base in ("zero", "max"):
            for qmap in (False, True):
                out.append(SimpleNamespace(id=f"chroma-d{depth}-{base}-qp{qp}-cb{cb}-cr{cr}" + ("-map" if qmap else ""), depth=depth, base=base, qp=qp, cb=cb, cr=cr,
                                           qmap=qmap, seed=i))
    return out


def chroma_inputs(case):
    """(cb, cr flat padded planes, stride, org, bs_ver, bs_hor - Bs 2 on every edge -, qp map or None); the planes are shared: read only."""
    cb, cr = chroma_picture(case.depth, case.base, case.seed)
    pb, stride, org = pad_any(cb, 16)
    pr = pad_any(cr, 16)[0]
    bv, bh = bs_maps("2", DB_W, DB_H)
    return pb, pr, stride, org, bv, bh, (qp_map_extremes(DB_W, DB_H, seed=1) if case.qmap else None)


def _chroma_pass(pl, bs, qpu, depth, offset, to, cnt):
    """edgeFilterChroma for every vertical edge on the 8-sample grid of a chroma plane (int64 [ch, cw], in place); bs / qpu [ch / 4, cw / 8]."""
    ch, cw = pl.shape
    mx = (1 << depth) - 1
    T8 = pl[:, 4:cw - 4].reshape(ch // 4, 4, cw // 8 - 1, 8).transpose(0, 2, 1, 3).copy()        # [unit, edge, line, tap]: taps -4 .. 3 around the edge
    T = T8[..., 2:6]
    on =(bs[:, 1:] > 1)[..., None] & np.ones(4, bool)
    q = qpu[:, 1:].astype(np.int64) + offset
    cnt["index_negative"] += int((on[..., 0] & (q + 2 + to < 0)).sum())
    cnt["index_table"] += int((on[..., 0] & (q >= 30)).sum())
    cnt["index_63"] += int((on[..., 0] & (q == 63)).sum())
    q = np.where(q >= 30, CHROMA_SCALE[np.clip(q, 0, 69)], q)
    tc = (TC_TABLE[np.clip(q + 2 + to, 0, 53)] << (depth - 8))[..., None]
    m2, m3, m4, m5 = [T[..., t] for t in range(4)]
    raw = ((m4 - m3) * 4 + m2 - m5 + 4) >> 3
    delta = np.clip(raw, -tc, tc)
    cnt["tc_clip"] += int((on & (delta != raw)).sum())
    n3, n4 = m3 + delta, m4 - delta
    cnt["clip_0"] += int((on & ((n3 < 0) | (n4 < 0))).sum()); cnt["clip_max"] += int((on & ((n3 > mx) | (n4 > mx))).sum())
    new3, new4 = np.where(on, np.clip(n3, 0, mx), m3), np.where(on, np.clip(n4, 0, mx), m4)
    T8[..., 3], T8[..., 4] = new3, new4
    pl[:, 4:cw - 4] = T8.transpose(0, 2, 1, 3).reshape(ch, cw - 8)


def chroma_census(depth, cb, cr, bv, bh, qp, qmap=None, cb_off=0, cr_off=0, to=0):
    """A numpy restatement of Deblock::edgeFilterChroma for 4:2:0 (deblock.cpp:417-497): the filtered planes and the counters
    (CHROMA_COUNTERS) summed over both planes and directions.  cb / cr: unpadded [h / 2, w / 2]."""
    ch, cw = cb.shape
    h, w = 2 * ch, 2 * cw
    qv, qh = unit_qps(qp, qmap, w, h)                           # luma units; a chroma unit of 4 lines takes the luma unit it starts at
    bvs, bhs = bv.reshape(h // 4, w // 8)[::2, ::2], bh.reshape(h // 8, w // 4)[::2, ::2].T
    cnt = dict.fromkeys(CHROMA_COUNTERS, 0)
    out = []
    for pl, off in ((cb, cb_off), (cr, cr_off)):
        work = pl.astype(np.int64)
        _chroma_pass(work, bvs, qv[::2, ::2], depth, off, 2 * to, cnt)
        wt = np.ascontiguousarray(work.T)
        _chroma_pass(wt, bhs, qh[::2, ::2], depth, off, 2 * to, cnt)
        out.append(np.ascontiguousarray(wt.T).astype(pl.dtype))
    return out[0], out[1], cnt
