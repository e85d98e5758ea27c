"""Operating points for the merge walk with the AMVP arm (numpy and the oracle only, no torch).

A case is a case of tests/merge_cases.py - its pictures, searched field, max_merge - plus a collocated field of tests/tmvp_cases.py
(`none`, `truth_rb`, `far`, or no field at all: no temporal MVP), the POC distances, the length of the bit-size table and how the inter
candidate's sa8d is chosen:

  real      what x265hip_inter_sa8d_cost gives (the oracle's sa8d of the searched vector)
  pattern   the sa8d that puts the inter COST at merge cost + (-1, 0, +1)[block % 3] (merge_expect.tie_pattern); the model derives it
            during its own walk and the array is handed to the device
  inter     merge cost - 1 everywhere: every block keeps its searched vector, so the neighbours' final motion is the searched field

Two kinds are added to merge_cases' fields by wrapping its field_vector:

  midway    (5, -3) + T[(gbx - gby) % 8] * (8, 4) with the triangle T = 0, -1, -2, -1, 0, 1, 2, 1: where gbx - gby is a multiple of four the
            block's vector lies midway between its left and its above neighbours' (A0 / B0 at -+2 steps, A1 / B1 at -+1), so the bits against
            the two predictors tie and selectMVP's SADs decide - in either direction, by the content
  clip_pair x = -(1040 | 1200) - (k % 5) by the parity of gbx + gby, y = 4 * (gby % 2): every vector lies beyond clipMv's lower limit at
            every block of a picture 192 wide, so two predictors that differ in x clip to one vector: the SADs tie and index 0 stays.  The
            left / above neighbours lie in the other group, 156 to 164 quarter samples away, where the truncated bit counts mostly tie.
            (Only the clipped vectors are ever predicted; the kind has no `real` costs.)"""
import collections
import functools

import intra_inter_expect as IX
import merge_cases as MC
import merge_expect as ME
import tmvp_cases as TC
import tmvp_expect as TX
import amvp_expect as AX

TRIANGLE = (0, -1, -2, -1, 0, 1, 2, 1)
_field_vector = MC.field_vector


def _wrapped_field_vector(field, gbx, gby, bw, bh):
    if field == "midway":
        t = TRIANGLE[(gbx - gby) % 8]
        return 5 + 8 * t, -3 + 4 * t
    if field == "clip_pair":
        k = gby * 7 + gbx * 3
        return -(1040 if (gbx + gby) % 2 == 0 else 1200) - k % 5, 4 * (gby % 2)
    return _field_vector(field, gbx, gby, bw, bh)


MC.field_vector = _wrapped_field_vector

ACase = collections.namedtuple("ACase", "id base col cur_delta col_delta costs table_len")


def _a(field, level, costs, max_merge, col=None, deltas=(4, 4), table_len=AX.TABLE_LEN, **kw):
    base = MC._case(field, level, "real" if costs == "real" else "pattern", max_merge, **kw)
    name = f"{base.w}x{base.h}-{field}-d{base.depth}-l{level}-{costs}-mm{max_merge}-lam{base.lambda8}-{col or 'notmvp'}-d{deltas[0]}_{deltas[1]}"
    return ACase(name + (f"-tab{table_len}" if table_len != AX.TABLE_LEN else ""), base, col, deltas[0], deltas[1], costs, table_len)


def _per_level(level):
    return [_a("uniform", level, "real", 3), _a("distinct", level, "pattern", 5, "truth_rb", (2, 4)), _a("distinct", level, "real", 2, "none"),
            _a("rows", level, "pattern", 3, "far", (4, 2)), _a("columns", level, "inter", 3, "truth_rb", (4, 4)), _a("quads", level, "real", 3, "truth_rb", (6, -7)),
            _a("quads", level, "pattern", 5, lambda8=0), _a("knight", level, "inter", 2, "none"), _a("far_edge", level, "pattern", 3, "far", (4, 4)),
            _a("midway", level, "inter", 3), _a("midway", level, "pattern", 3, "none"), _a("midway", level, "real", 2, "truth_rb", (4, 4)),
            _a("clip_pair", level, "inter", 3), _a("clip_pair", level, "pattern", 2, "none"), _a("flat", level, "real", 3),
            _a("distinct", level, "real", 3, lambda8=4096), _a("distinct", level, "pattern", 3, table_len=24)]


COVER_CASES = [c for level in (0, 1, 2) for c in _per_level(level)]                              # 8 bits, 192x128: what the coverage condition counts
OTHER_CASES = [_a("midway", 1, "pattern", 3, "truth_rb", (2, 4), depth=10), _a("quads", 0, "pattern", 3, "truth_rb", (4, 4), w=64, h=64),
               _a("midway", 2, "inter", 3, w=64, h=64), _a("rows", 1, "pattern", 3, "far", (4, 2), w=64, h=192), _a("midway", 0, "pattern", 2, w=64, h=192)]
ALL_CASES = COVER_CASES + OTHER_CASES
BASE_BITS = IX.BASE_BITS


@functools.lru_cache(maxsize=None)
def table(length):
    return IX.s_bitsizes(length)


@functools.lru_cache(maxsize=None)
def source(ac):
    """The case's ColSource, or None without temporal MVP.  Shared, never modified."""
    if ac.col is None:
        return None
    c = ac.base
    n = 8 << c.level
    bw, bh = c.w // n, c.h // n
    return TC.col_source(ac.col, c.level, c.w, c.h, lambda gbx, gby: MC.field_vector(c.field, gbx, gby, bw, bh), TX.scale_factor(ac.cur_delta, ac.col_delta),
                         ac.col_delta)


@functools.lru_cache(maxsize=None)
def sad_pricer(c):
    x = MC.inputs(c)
    return AX.SadPricer(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level)


def inter_always(b, merge_cost):
    return merge_cost - 1


def run_stage(ac, mutation=None, inter_sa8d=None):
    """The expectation of a case, of a mutation of the AMVP arm on it, or with another sa8d array."""
    c = ac.base
    x = MC.inputs(c)
    cost_fn = None
    if inter_sa8d is None:
        if ac.costs == "real":
            inter_sa8d = x["real"][:, 0]
        else:
            cost_fn = ME.tie_pattern if ac.costs == "pattern" else inter_always
    return AX.stage_expectation(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level, x["mv"], c.max_merge, c.lambda8, table(ac.table_len), BASE_BITS,
                                inter_sa8d=inter_sa8d, cost_fn=cost_fn, qp=x["qp"], mutation=mutation, pricer=x["pricer"], sad_pricer=sad_pricer(c),
                                col=source(ac), cur_delta=ac.cur_delta if ac.col is not None else None)


@functools.lru_cache(maxsize=None)
def expectation(ac):
    x = dict(MC.inputs(ac.base))
    x["e"] = run_stage(ac)
    x["col"] = source(ac)
    return x
