"""Collocated fields and operating points for the merge stages with the temporal candidate (numpy and the oracle only, no torch).

A case is a case of tests/merge_cases.py (P) or tests/bmerge_cases.py (B) - its pictures, searched field / inter winners, inter costs,
max_merge - plus a collocated field handed to the stage directly (not derived from a coded picture) and the POC distances.  The fields,
one (vector, distance) per 8x8 cell of the collocated picture (tmvp_expect.ColSource); every inter cell has the distance col_delta:

  none          every cell intra: no temporal candidate anywhere - the walks of merge_expect / bmerge_expect
  truth_rb      the unit a block's bottom-right try reads carries the vector the current picture was displaced by in that block, divided
                out by the scale (the first block in coding order where several read one unit); other units their own block's vector
  truth_centre  the same for the unit the centre reads, with the units the bottom-right tries read intra where the grid allows it: unit
                rows with odd uy at levels 0 / 1, units with even ux and uy at level 2
  checker       intra / inter units alternating, the inter ones with their own block's vector
  equal_a1      the unit a block's bottom-right try reads carries the searched vector of the block's LEFT neighbour (what that neighbour
                ends up with unless it merged elsewhere), divided out by the scale
  truth_unit    unit (ux, uy) carries unit_vector(ux, uy) divided out by the scale, for the B kind `tmvp_split` below
  far           vectors of +-(20000 + k, 9000 + k) quarter samples: past both clipMv limits as they are, to +-32767 under a scale of 512;
                unit 5 of every CTU holds (-32768, 32767)

In every field the three cells of a unit that are not its upper-left one hold the unit's vector + (4, 8): the device never sees them
(TMVP_UNIT_MASK); the `no_unit_mask` mutation does.

POC distances (cur_delta, col_delta): (4, 4) identity, (2, 4) scale 128, (4, 2) scale 512, (5, 7) scale 183, (6, -7) scale -219 with a
negative divisor (where C's truncating division and Python's floor differ); for B (cur_delta0, cur_delta1) = (2, -2) and (1, -3)
against a col_delta of 4: scales 128 / -128 and 64 / -192.

The B kind `tmvp_split` (192x128 only) is added to bmerge_cases' kinds by wrapping its kind_motion / kind_content: no existing kind lets a
combined candidate built from the temporal one predict best, because each has an exact spatial or spatial-combined candidate in front of
it.  Here the content of every block is bidirectional - list 0 displaced by unit_vector() of the unit the block's temporal lookup reads,
list 1 by (-5, 2) - while the inter winner uses list 1 only: the spatial candidates are {2, (-5, 2)}, the temporal one has the right list-0
vector and a wrong list-1 vector, and the pair (temporal list 0, spatial list 1) is the block's own motion."""
import collections
import functools

import numpy as np

import bmerge_cases as BC
import merge_cases as MC
import merge_expect as ME
import tmvp_expect as TX

FIELDS = ("none", "truth_rb", "truth_centre", "checker", "equal_a1", "truth_unit", "far")


def unit_vector(ux, uy):
    return (ux * 7 + uy * 3) % 41 - 20, (ux * 11 + uy * 5) % 37 - 18


def _split_motion(gbx, gby, bw, bh):
    n = 192 // bw
    assert bh * n == 128, "tmvp_split is a 192x128 kind"
    _, rb, centre = TX.positions({8: 0, 16: 1, 32: 2}[n], 192, 128, gbx * n, gby * n)
    x, y = rb or centre
    return unit_vector(x >> 4, y >> 4), (-5, 2)


_kind_motion, _kind_content = BC.kind_motion, BC.kind_content


def _wrapped_motion(kind, gbx, gby, bw, bh):
    if kind == "tmvp_split":
        return (2,) + _split_motion(gbx, gby, bw, bh)
    return _kind_motion(kind, gbx, gby, bw, bh)


def _wrapped_content(kind, gbx, gby, bw, bh):
    if kind == "tmvp_split":
        return (3,) + _split_motion(gbx, gby, bw, bh)
    return _kind_content(kind, gbx, gby, bw, bh)


BC.kind_motion, BC.kind_content = _wrapped_motion, _wrapped_content


def _inverse(v, scale):
    """A vector that scales to v, or as near as the scale allows.  Among the components that scale to it exactly, one whose product is
    negative and ends in 128 is preferred: there scaleMv's rounding term `+ (scale * v < 0)` decides the result."""
    if scale is None:
        return v

    def component(c):
        r = int(np.clip(np.rint(c * 256.0 / scale), -32768, 32767))
        exact = [x for x in range(max(r - 2, -32768), min(r + 2, 32767) + 1) if TX.scale_component(x, scale) == c]
        sharp = [x for x in exact if TX.scale_component(x, scale, "no_negative_rounding") != c]
        return (sharp or exact or [r])[0]
    return tuple(component(c) for c in v)


def col_source(field, level, w64, h64, vector_of, scale, col_delta):
    """The ColSource of a field.  vector_of(gbx, gby) -> the (qx, qy) the current picture's block (gbx, gby) of the level's grid is displaced
    by (what its search finds); scale: the scale factor the walk will apply (None = identity)."""
    n = 8 << level
    bw, bh = w64 // n, h64 // n
    src = TX.ColSource(w64, h64)
    if field == "none":
        return src
    own = lambda x, y: _inverse(vector_of(min(x // n, bw - 1), min(y // n, bh - 1)), scale)
    unit = {}                                                   # (ux, uy) of the picture -> (qx, qy) or None (intra)
    for uy in range(h64 // 16):
        for ux in range(w64 // 16):
            unit[(ux, uy)] = own(16 * ux, 16 * uy)
    blocks = [(gbx, gby) for gby in range(bh) for gbx in range(bw)]
    if field in ("truth_rb", "equal_a1"):
        taken = set()
        for gbx, gby in blocks:
            _, rb, _ = TX.positions(level, w64, h64, gbx * n, gby * n)
            if rb is not None and (rb[0] >> 4, rb[1] >> 4) not in taken:
                taken.add((rb[0] >> 4, rb[1] >> 4))
                unit[(rb[0] >> 4, rb[1] >> 4)] = _inverse(vector_of(max(gbx - 1, 0) if field == "equal_a1" else gbx, gby), scale)
    elif field == "truth_centre":
        taken = set()
        for gbx, gby in blocks:
            _, _, c = TX.positions(level, w64, h64, gbx * n, gby * n)
            if (c[0] >> 4, c[1] >> 4) not in taken:
                taken.add((c[0] >> 4, c[1] >> 4))
                unit[(c[0] >> 4, c[1] >> 4)] = _inverse(vector_of(gbx, gby), scale)
        for (ux, uy) in unit:
            if (ux % 2 == 0 and uy % 2 == 0) if level == 2 else uy % 2 == 1:
                unit[(ux, uy)] = None
    elif field == "checker":
        for (ux, uy) in unit:
            if (ux + uy) % 2:
                unit[(ux, uy)] = None
    elif field == "truth_unit":
        for (ux, uy) in unit:
            unit[(ux, uy)] = _inverse(unit_vector(ux, uy), scale)
    elif field == "far":
        for (ux, uy) in unit:
            k = ux * 5 + uy * 3
            sx, sy = (1, -1)[(ux + uy) % 2], (1, -1)[(ux // 2 + uy) % 2]
            unit[(ux, uy)] = (-32768, 32767) if (ux % 4, uy % 4) == (1, 1) else (sx * (20000 + k), sy * (9000 + k))
    else:
        raise AssertionError(field)
    for (ux, uy), v in unit.items():
        if v is None:
            continue
        for dy in (0, 1):
            for dx in (0, 1):
                q = v if (dx, dy) == (0, 0) else (int(np.clip(v[0] + 4, -32768, 32767)), int(np.clip(v[1] + 8, -32768, 32767)))
                src.mv[2 * uy + dy, 2 * ux + dx] = ME.pack(*q)
                src.delta[2 * uy + dy, 2 * ux + dx] = col_delta
    return src


PCase = collections.namedtuple("PCase", "id base field cur_delta col_delta")
BCase = collections.namedtuple("BCase", "id base field cur_deltas col_delta")


def _p(field, level, costs, max_merge, col, deltas, **kw):
    base = MC._case(field, level, costs, max_merge, **kw)
    return PCase(f"{base.id}-{col}-d{deltas[0]}_{deltas[1]}", base, col, deltas[0], deltas[1])


def _b(kind, level, costs, max_merge, col, cur_deltas, col_delta=4, **kw):
    base = BC._case(kind, level, costs, max_merge, **kw)
    return BCase(f"{base.id}-{col}-d{cur_deltas[0]}_{cur_deltas[1]}_{col_delta}", base, col, tuple(cur_deltas), col_delta)


def _p_level(level):
    return [_p("uniform", level, "real", 3, "truth_rb", (4, 4)), _p("distinct", level, "pattern", 5, "truth_rb", (2, 4)),
            _p("distinct", level, "real", 2, "truth_centre", (4, 2)), _p("quads", level, "pattern", 3, "checker", (5, 7)),
            _p("quads", level, "real", 3, "equal_a1", (4, 4)), _p("knight", level, "pattern", 5, "truth_centre", (4, 4)),
            _p("uniform", level, "pattern", 1, "truth_rb", (4, 4)), _p("distinct", level, "pattern", 2, "far", (4, 2)),
            _p("knight", level, "pattern", 3, "far", (4, 4)), _p("quads", level, "pattern", 2, "truth_rb", (6, -7)),
            _p("uniform", level, "pattern", 2, "equal_a1", (2, 4)), _p("knight", level, "pattern", 3, "far", (6, -7)),
            _p("distinct", level, "pattern", 5, "none", (4, 4))]


def _b_level(level):
    return [_b("uniform", level, "real", 3, "truth_rb", (2, -2)), _b("distinct", level, "pattern", 5, "truth_rb", (1, -3)),
            _b("cross", level, "pattern", 3, "truth_centre", (2, -2)), _b("cross", level, "real", 5, "checker", (1, -3)),
            _b("dir_stripes", level, "pattern", 5, "truth_rb", (2, -2)), _b("quads", level, "pattern", 2, "far", (2, -2)),
            _b("rows", level, "pattern", 3, "equal_a1", (2, -2)), _b("same_ref", level, "pattern", 5, "truth_rb", (2, -2)),
            _b("uniform", level, "pattern", 1, "truth_rb", (2, -2)), _b("tmvp_split", level, "pattern", 3, "truth_unit", (2, -2)),
            _b("distinct", level, "pattern", 5, "none", (2, -2))]


P_COVER = [c for level in (0, 1, 2) for c in _p_level(level)]                                     # 8 bits, 192x128: what the coverage condition counts
B_COVER = [c for level in (0, 1, 2) for c in _b_level(level)]
P_OTHER = [_p("quads", 1, "pattern", 3, "truth_rb", (2, 4), depth=10), _p("knight", 1, "pattern", 5, "far", (4, 2), depth=10),
           _p("quads", 0, "pattern", 3, "truth_rb", (4, 4), w=64, h=64), _p("rows", 1, "pattern", 3, "checker", (5, 7), w=64, h=192)]
B_OTHER = [_b("rows", 1, "pattern", 3, "truth_rb", (2, -2), depth=10), _b("quads", 0, "pattern", 3, "truth_centre", (1, -3), w=64, h=64),
           _b("cross", 1, "pattern", 3, "checker", (2, -2), w=64, h=192)]


def _vector_of(tc):
    c = tc.base
    n = 8 << c.level
    bw, bh = c.w // n, c.h // n
    if isinstance(tc, PCase):
        return lambda gbx, gby: MC.field_vector(c.field, gbx, gby, bw, bh)
    return lambda gbx, gby: BC.kind_motion(c.kind, gbx, gby, bw, bh)[1]


@functools.lru_cache(maxsize=None)
def source(tc):
    """The case's ColSource.  Shared, never modified."""
    c = tc.base
    cur = tc.cur_delta if isinstance(tc, PCase) else tc.cur_deltas[0]
    return col_source(tc.field, c.level, c.w, c.h, _vector_of(tc), TX.scale_factor(cur, tc.col_delta), tc.col_delta)


def inputs(tc):
    return (MC if isinstance(tc, PCase) else BC).inputs(tc.base)


def run_stage(tc, tmvp_mutation=None, col="case"):
    """The expectation of a case, of a mutation of the walk's temporal part on it, or (col=None) of the walk without a collocated field."""
    src = source(tc) if col == "case" else col
    if isinstance(tc, PCase):
        return MC.run_stage(tc.base, col=src, cur_delta=tc.cur_delta, tmvp_mutation=tmvp_mutation)
    return BC.run_stage(tc.base, col=src, cur_deltas=tc.cur_deltas, tmvp_mutation=tmvp_mutation)


@functools.lru_cache(maxsize=None)
def expectation(tc):
    x = dict(inputs(tc))
    x["e"] = run_stage(tc)
    x["col"] = source(tc)
    return x
