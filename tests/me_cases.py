"""Deterministic inputs for the exhaustive-search tests (numpy and the oracle only, no torch): pictures, mv-cost tables and operating points that
drive the cost term of `sad + cost_x[mvx] + cost_y[mvy]` through every bit the kernels' row-local 32-bit keys give it, with x and y tables that differ.

Pictures (128x64 = 2 CTUs unless an operating point says otherwise, padded by frames.pad_plane: +-80 stays inside the margins with zero centres):
  flat_max / flat_max_r   source all 0 against reference all 2^depth - 1, and the reverse: every SAD at its maximum, every candidate ties on SAD - the
                          cost alone decides, every accumulator and key is full
  flat_equal              both pictures at one value: every SAD is 0
  noise                   uniform random samples in both pictures
  ramp                    the reference a two-dimensional ramp of 3 x + 2 y (folded every 160 to stay steep at 8 bits), the source the same padded ramp
                          displaced by a vector inside the window: SAD grows smoothly with distance, large costs move the winner to an interior compromise
  corner_pp / _mm / _pm   noise, the source the padded reference displaced by (+R, +R), (-R, -R), (+R, -R): SAD 0 in the last real column next to the
                          pad columns of the last column group, or at raster index 0
Tables (uint16 [2 R + 1], x and y different in every kind but the first two, where the kind itself says they are equal):
  cap      frames.mv_cost_table(R, 2000): the reference formula's own saturation at 32767 (1436 at the centre, 34 capped entries at +-57)
  u16max   65535 everywhere: the sum is 131070, raster order alone decides
  asym     21000 + 5 |d - ax| (+ 2 right of ax) and 43000 + 11 |d - ay| (+ 1 left of ay): different at -d and +d, different slopes, unique minima away
           from the centre and from each other - on flat content the winner is exactly (argmin cost_x, argmin cost_y)
  high     65535 - 13 p(d) and 65535 - 17 q(d), p and q permutations: distinct, the low bits decide while the high bits are all set
  step     0 inside a small off-centre rectangle, 65535 outside

tests/test_me_cases_cpu.py shows with the oracle alone that these cases tell a wrong cost handling from the right one at every PU level;
tests/test_gpu_me_cases.py runs them through x265hip_me_fullsearch on every kernel its launch table can select."""
import functools
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np

F = importlib.import_module("x265-yuuki-asuna_amd.frames")

DEPTHS = (8, 10, 12)
LEVEL_SIZE = (8, 16, 32, 64)
LEVEL_BASE = (0, 64, 80, 84)
LEVEL_PUS = (64, 16, 4, 1)
CAP_LAMBDA = 2000.0
PAD_TOTAL = (1 << 20, 1 << 23, 1 << 23, 1 << 23)      # the cost the fast paths give a pad column of the last column group, per level


def oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def pixel_type(depth):
    return np.uint8 if depth == 8 else np.uint16


def _frozen(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else a.astype(dtype))
    a.setflags(write=False)
    return a


def sad_max(depth, level):
    return ((1 << depth) - 1) * LEVEL_SIZE[level] ** 2


def total_max(depth, level):
    """The largest real sad + cost_x + cost_y of a level: two tables of 65535."""
    return sad_max(depth, level) + 2 * 65535


# ---- pictures ------------------------------------------------------------------------------------------------------------------------------
CONTENTS = ("flat_max", "flat_max_r", "flat_equal", "noise", "ramp", "corner_pp", "corner_mm", "corner_pm")
CORNER = {"corner_pp": (1, 1), "corner_mm": (-1, -1), "corner_pm": (1, -1)}


def _displaced(ref, dx, dy):
    """source(x, y) = what the padded reference plane holds at (x + dx, y + dy): SAD 0 at that displacement for every PU, the picture's edges included."""
    h, w = ref.shape
    buf, stride, _, _, _ = F.pad_plane(ref)
    p = buf.reshape(-1, stride)
    return p[F.MARGIN_Y + dy:F.MARGIN_Y + dy + h, F.MARGIN_X + dx:F.MARGIN_X + dx + w]


RAMP_HALF_PERIOD = 160.0


def ramp_vector(rng):
    return rng // 2, -(rng // 3)


@functools.lru_cache(maxsize=None)
def pictures(depth, content, width, height, rng):
    """(source, reference) luma of a case, read-only."""
    mx, t = (1 << depth) - 1, pixel_type(depth)
    r = np.random.default_rng([211, depth, width, height])
    if content in ("flat_max", "flat_max_r"):
        a, b = np.zeros((height, width)), np.full((height, width), mx)
        src, ref = (a, b) if content == "flat_max" else (b, a)
    elif content == "flat_equal":
        src = ref = np.full((height, width), mx - 5)
    elif content == "noise":
        src, ref = r.integers(0, mx + 1, (height, width)), r.integers(0, mx + 1, (height, width))
    elif content == "ramp":
        yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
        tt = (3 * xx + 2 * yy) / RAMP_HALF_PERIOD          # folded every RAMP_HALF_PERIOD: steep enough at 8 bits that a 64x64 SAD outweighs a capped cost
        ref = np.rint(mx * (0.05 + 0.9 * np.abs(tt - 2 * np.floor(tt / 2 + 0.5)))).astype(t)
        src = _displaced(ref, *ramp_vector(rng))
    else:
        sx, sy = CORNER[content]
        ref = r.integers(0, mx + 1, (height, width)).astype(t)
        src = _displaced(ref, sx * rng, sy * rng)
    return _frozen(src, t), _frozen(ref, t)


# ---- tables --------------------------------------------------------------------------------------------------------------------------------
TABLES = ("cap", "u16max", "asym", "high", "step")


def asym_minima(rng):
    """(index of cost_x's minimum, index of cost_y's): off the centre index `rng`, on opposite sides of it."""
    return rng + max(rng // 3, 1), rng - rng // 2 - 1


def step_window(rng):
    """(x0, x1, y0, y1): the index rectangle [x0, x1) x [y0, y1) where the step tables are 0."""
    ax, ay = asym_minima(rng)
    return ax - 1, ax + 2, ay, ay + 2


@functools.lru_cache(maxsize=None)
def tables(kind, rng):
    """(cost_x, cost_y), uint16 [2 rng + 1], read-only."""
    n = 2 * rng + 1
    i = np.arange(n)
    if kind == "cap":
        cx = cy = F.mv_cost_table(rng, CAP_LAMBDA)
    elif kind == "u16max":
        cx = cy = np.full(n, 65535)
    elif kind == "asym":
        ax, ay = asym_minima(rng)
        cx = 21000 + 5 * np.abs(i - ax) + 2 * (i > ax)
        cy = 43000 + 11 * np.abs(i - ay) + (i < ay)
    elif kind == "high":
        r = np.random.default_rng([223, rng])
        cx, cy = 65535 - 13 * r.permutation(n), 65535 - 17 * r.permutation(n)
    elif kind == "step":
        x0, x1, y0, y1 = step_window(rng)
        cx, cy = np.where((i >= x0) & (i < x1), 0, 65535), np.where((i >= y0) & (i < y1), 0, 65535)
    else:
        raise KeyError(kind)
    assert cx.min() >= 0 and cx.max() <= 65535 and cy.min() >= 0 and cy.max() <= 65535
    return _frozen(cx, np.uint16), _frozen(cy, np.uint16)


# ---- the oracle's answers ------------------------------------------------------------------------------------------------------------------
def _padded(depth, content, width, height, rng):
    src, ref = pictures(depth, content, width, height, rng)
    return F.pad_plane(src), F.pad_plane(ref)


@functools.lru_cache(maxsize=None)
def expected_best(depth, content, width, height, rng, table):
    """The oracle's minima, uint64 [ctu * 85], zero centres: computed once per (pictures, tables), shared by every operating point."""
    (cb, cs, co, w64, h64), (rb, rs, ro, _, _) = _padded(depth, content, width, height, rng)
    cx, cy = tables(table, rng)
    _, best = oracle().me_fullsearch(depth, cb, cs, co, rb, rs, ro, w64, h64, rng, 0, (w64 // 64) * (h64 // 64), cx, cy, want_surf=False, want_best=True)
    best.setflags(write=False)
    return best


@functools.lru_cache(maxsize=6)
def expected_surf(depth, content, width, height, rng):
    """The oracle's SAD surfaces, int32 [ctu][mvy][mvx / 4][85][4], zero centres."""
    (cb, cs, co, w64, h64), (rb, rs, ro, _, _) = _padded(depth, content, width, height, rng)
    z = np.zeros(2 * rng + 1, np.uint16)
    surf, _ = oracle().me_fullsearch(depth, cb, cs, co, rb, rs, ro, w64, h64, rng, 0, (w64 // 64) * (h64 // 64), z, z, want_surf=True, want_best=False)
    surf.setflags(write=False)
    return surf


def centres_of(nctu, seed=5):
    return np.random.default_rng([227, seed]).integers(-20, 21, size=(nctu, 2)).astype(np.int16)


def expected_centred(depth, content, width, height, rng, table, centres):
    """(surf, best) with the window of CTU c centred on centres[c]: every CTU searched on its own by the oracle, as a one-CTU picture."""
    (cb, cs, co, w64, h64), (rb, rs, ro, _, _) = _padded(depth, content, width, height, rng)
    cx, cy = tables(table, rng)
    cw = w64 // 64
    surfs, bests = [], []
    for c in range(cw * (h64 // 64)):
        o = co + (c // cw) * 64 * cs + (c % cw) * 64
        s, b = oracle().me_fullsearch(depth, cb, cs, o, rb, rs, o + int(centres[c, 1]) * rs + int(centres[c, 0]), 64, 64, rng, 0, 1, cx, cy)
        surfs.append(s); bests.append(b)
    return np.concatenate(surfs), np.concatenate(bests)


def valid(surf, nctu, rng):
    """[ctu, mvy, mvx, 85] view of an int32 surface with the pad columns of the last group dropped."""
    nc = 2 * rng + 1
    ng = (nc + 3) // 4
    return surf.reshape(nctu, nc, ng, 85, 4).transpose(0, 1, 2, 4, 3).reshape(nctu, nc, ng * 4, 85)[:, :, :nc, :]


# ---- minima in numpy, right and wrong ------------------------------------------------------------------------------------------------------
def _swap(cx, cy): return cy, cx
def _x_far(cx, cy): return cx[::-1], cy
def _y_far(cx, cy): return cx, cy[::-1]
def _x_15(cx, cy): return cx & 0x7fff, cy
def _y_15(cx, cy): return cx, cy & 0x7fff


TABLE_MUTATIONS = {"tables swapped": _swap, "cost_x read from the far end": _x_far, "cost_y read from the far end": _y_far,
                   "cost_x masked to 15 bits": _x_15, "cost_y masked to 15 bits": _y_15}


def minima(surf, nctu, rng, cx, cy, level, saturate=False, bits=None, pad=False, last=False):
    """uint64 [ctu, PUs of the level] = min over the window of (sad + cost_x[mvx] + cost_y[mvy]) << 32 | raster index from the oracle's surface, in 64-bit
    arithmetic.  The wrong ways: saturate - cost_x + cost_y clamped to 65535; bits - the total cut to its low `bits` bits; pad - a candidate of total
    PAD_TOTAL[level] takes part (the pad column of the last column group, raster index 2 rng + 1 = row 0's); last - ties go to the largest raster index."""
    nc = 2 * rng + 1
    b, n = LEVEL_BASE[level], LEVEL_PUS[level]
    sad = valid(surf, nctu, rng)[..., b:b + n].astype(np.int64)
    mvc = cx.astype(np.int64)[None, :] + cy.astype(np.int64)[:, None]
    if saturate:
        mvc = np.minimum(mvc, 65535)
    tot = sad + mvc[None, :, :, None]
    if bits is not None:
        tot &= (1 << bits) - 1
    idx = np.arange(nc * nc, dtype=np.int64).reshape(1, nc, nc, 1)
    key = (tot << 32) | (nc * nc - 1 - idx if last else idx)
    m = key.reshape(nctu, nc * nc, n).min(axis=1)
    if last:
        m = (m & ~np.int64(0xffffffff)) | (nc * nc - 1 - (m & 0xffffffff))
    if pad:
        m = np.minimum(m, (np.int64(PAD_TOTAL[level]) << 32) | nc)
    return m.astype(np.uint64)


# ---- operating points ----------------------------------------------------------------------------------------------------------------------
# route: what x265hip_me_minima_kernel_name must answer under the switches (the family and LDS pitch the launch table picks); kernel: the kernel the
# launch of this output form runs, read from launch_me.  out: best / surf / both.  packed: False (int32 surfaces), True, "t", "b".
Q2 = "me_ctu_q2_kernel<256,13566>"
GEN8, GEN16 = "me_ctu_kernel<u8,best>", "me_ctu_kernel<u16,best>"


def _op(name, depth, ranges, route, kernel=None, env=None, out="best", packed=False, centres=False, size=(128, 64)):
    return SimpleNamespace(name=name, depth=depth, ranges=ranges, route=route, kernel=kernel or route, env=env or {}, out=out, packed=packed,
                           centres=centres, size=size)


OPS = (
    # 8 bits, 256-byte pitch (+-58 is the widest window it holds)
    _op("q2_split", 8, (17, 57, 58), Q2),                                                              # small pictures: 8 column groups per workgroup
    _op("q2_whole", 8, (8, 57), Q2, env={"X265HIP_ME_SPLIT_GROUPS": "0"}),
    _op("q_v0", 8, (8, 58), "me_ctu_q_kernel<best>", env={"X265HIP_ME_BEST_VARIANT": "0"}),
    _op("q_v1", 8, (17, 57), "me_ctu_q_kernel<best>", env={"X265HIP_ME_BEST_VARIANT": "1"}),
    _op("q_fused", 8, (8, 57), Q2, kernel="me_ctu_q_kernel<surf,best>", out="both"),
    _op("q_fused_packed", 8, (17,), Q2, kernel="me_ctu_q_kernel<surf,best,packed>", out="both", packed=True),
    # 8 bits, the record-per-lane kernel: +-63 is the last window whose raster index fits 14 bits
    _op("cand", 8, (8, 63, 64, 80), "me_ctu_c_kernel (record per lane)", env={"X265HIP_ME_KERNEL": "cand"}),
    _op("cand_t", 8, (17,), None, kernel="me_ctu_c_kernel<surf,best,PACKED_T>", out="both", packed="t"),
    _op("cand_b", 8, (57,), None, kernel="me_ctu_c_kernel<surf,best,PACKED_B>", out="both", packed="b"),
    # 8 bits beyond the 256-byte pitch: the generic kernel at 512
    _op("gen8", 8, (59, 80), GEN8),
    _op("gen8_both", 8, (59,), GEN8, kernel="me_ctu_kernel<u8,surf,best>", out="both"),
    # 10 bits: +-12 is the last window at the 256-byte pitch, +-76 at the 512-byte one
    _op("w2", 10, (8, 12, 13, 57, 76), "me_ctu_w2_kernel"),
    _op("w", 10, (8, 13, 75), "me_ctu_w_kernel<best>", env={"X265HIP_ME_W2": "0"}),
    _op("w_fused", 10, (16,), "me_ctu_w2_kernel", kernel="me_ctu_w_kernel<surf,best>", out="both"),
    # 12 bits: the generic kernel, both pitches, the three output forms, windows centred per CTU
    _op("gen16", 12, (8, 14, 32, 57, 76), GEN16),
    _op("gen16_both", 12, (8, 32), GEN16, kernel="me_ctu_kernel<u16,surf,best>", out="both"),
    _op("gen16_surf", 12, (14,), GEN16, kernel="me_ctu_kernel<u16,surf>", out="surf"),
    _op("gen16_centres", 12, (14,), GEN16, kernel="me_ctu_kernel<u16,surf,best>", out="both", centres=True, size=(192, 128)),
)

# every kernel meets these five; an operating point's first range adds two more and one that rotates, its other ranges take three in all
MANDATORY = (("flat_max", "u16max"), ("flat_max_r", "high"), ("flat_max", "asym"), ("corner_pp", "cap"), ("ramp", "cap"))
FIRST_RANGE = (("noise", "step"), ("flat_equal", "asym"))
ROTATING = (("noise", "high"), ("flat_max_r", "cap"), ("flat_equal", "u16max"), ("corner_mm", "asym"), ("flat_max", "step"), ("ramp", "high"), ("corner_pm", "step"),
            ("noise", "asym"))
CORNERS = ("corner_mm", "corner_pm", "corner_pp")


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """Every case tests/test_gpu_me_cases.py runs: (id, op, rng, content, table)."""
    out, rot = [], 0
    for op in OPS:
        for j, rng in enumerate(op.ranges):
            if op.out == "surf":
                combos = (("flat_max", "u16max"), ("noise", "step"))          # no minima: the tables do not matter
            elif j == 0:
                combos = MANDATORY + FIRST_RANGE + (ROTATING[rot % len(ROTATING)],)
            else:
                combos = (("flat_max" if rot & 1 else "flat_max_r", "high"), (CORNERS[rot % 3], "cap"), ROTATING[rot % len(ROTATING)])
            rot += 1
            for content, table in combos:
                out.append(SimpleNamespace(id=f"{op.name}-d{op.depth}-r{rng}-{content}-{table}", op=op, rng=rng, content=content, table=table))
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def data_key(case):
    return (case.op.depth, case.content, case.op.size[0], case.op.size[1], case.rng, case.table)


# The first range beyond the widest window each fast path stages: the generic kernel answers (8 bits: +-59, among OPS), or the entry refuses.  16-bit samples:
# the window row of +-77 needs a 1024-byte LDS pitch and 220 rows of it pass the 160 KiB a workgroup may use, so +-77 is refused at 10 and at 12 bits.
REFUSED = ((10, 77, "best"), (10, 77, "both"), (12, 77, "best"), (12, 77, "surf"))
