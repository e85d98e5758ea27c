"""The inputs of the exhaustive-search cost tests (tests/me_cases.py) checked with the oracle alone: the cases must TELL.  For every way of handling the
mv cost wrongly that a narrow key or a 16-bit operand invites - the tables swapped, a table read from the far end, a table kept in 15 bits, the sum of the two
saturated at 65535, the total cut to too few bits, a pad column of the last column group let into the minimum, ties resolved to the last candidate - the 64-bit
minima computed in numpy from the oracle's SAD surfaces must differ from the true ones in at least one case that tests/test_gpu_me_cases.py runs at that depth,
at every PU level the mistake can reach.  The totals the kernels' width comments rest on are asserted as exact numbers in the oracle's own output.
These are conditions on the inputs: a case list that misses one gets other cases, never a looser condition."""
import numpy as np
import pytest

import me_cases as MC

LEVELS = range(4)


def _subset(depth):
    """The GPU module's cases of a depth with small windows (the oracle's surfaces stay small), one per (pictures, tables)."""
    seen = {}
    for c in MC.gpu_cases():
        if c.op.depth == depth and c.rng <= 17 and not c.op.centres and c.op.out != "surf":
            seen.setdefault(MC.data_key(c), c)
    return list(seen.values())


def _nctu(c):
    return (c.op.size[0] // 64) * (c.op.size[1] // 64)


def _surf(c):
    return MC.expected_surf(c.op.depth, c.content, *c.op.size, c.rng)


def _true(c, level):
    b, n = MC.LEVEL_BASE[level], MC.LEVEL_PUS[level]
    return MC.expected_best(*MC.data_key(c)).reshape(-1, 85)[:, b:b + n]


def _caught(depth, level, wrong):
    """The ids of the cases whose minima of `level` the wrong computation changes; wrong(case, surf, nctu, cx, cy) -> uint64 [ctu, PUs]."""
    hit = []
    for c in _subset(depth):
        cx, cy = MC.tables(c.table, c.rng)
        if not np.array_equal(wrong(c, _surf(c), _nctu(c), cx, cy), _true(c, level)):
            hit.append(c.id)
    return hit


def test_the_case_list_is_the_size_asked_for_and_every_kernel_meets_the_mandatory_pairs():
    cases = MC.gpu_cases()
    assert 150 <= len(cases) + len(MC.REFUSED) <= 250, len(cases)
    for op in MC.OPS:
        if op.out == "surf":
            continue
        have = {(c.content, c.table) for c in cases if c.op is op}
        assert set(MC.MANDATORY) <= have, op.name
    for kind in MC.TABLES:
        if kind in ("cap", "u16max"):
            continue
        for rng in (1, 8, 17, 57, 80):
            cx, cy = MC.tables(kind, rng)
            assert not np.array_equal(cx, cy) and not np.array_equal(cx, cx[::-1]) and not np.array_equal(cy, cy[::-1]), (kind, rng)
    cx, _ = MC.tables("cap", 57)
    assert int(cx[57]) == 1436 and int(np.count_nonzero(cx == 32767)) == 34 and int(cx.max()) == 32767
    for rng in (8, 57, 80):
        cx, cy = MC.tables("high", rng)
        assert len(set(cx.tolist())) == 2 * rng + 1 == len(set(cy.tolist())) and int(min(cx.min(), cy.min())) > 65535 - 4096
        cx, cy = MC.tables("asym", rng)
        ax, ay = MC.asym_minima(rng)
        assert ax != rng != ay != ax and np.count_nonzero(cx == cx.min()) == 1 == np.count_nonzero(cy == cy.min()) and (int(cx.argmin()), int(cy.argmin())) == (ax, ay)
        d = np.arange(1, rng + 1)
        assert np.all(cx[rng - d] != cx[rng + d]) and np.all(cy[rng - d] != cy[rng + d])


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_numpy_minima_are_the_oracles(depth):
    """The plain 64-bit restatement the mutations are applied to: without a mutation it gives the oracle's minima, on every case."""
    cases = _subset(depth)
    assert len(cases) >= 8
    for c in cases:
        cx, cy = MC.tables(c.table, c.rng)
        for level in LEVELS:
            assert np.array_equal(MC.minima(_surf(c), _nctu(c), c.rng, cx, cy, level), _true(c, level)), (c.id, level)


@pytest.mark.parametrize("depth", MC.DEPTHS)
@pytest.mark.parametrize("name", list(MC.TABLE_MUTATIONS))
def test_a_wrong_table_changes_minima_at_every_level(name, depth):
    f = MC.TABLE_MUTATIONS[name]
    for level in LEVELS:
        assert _caught(depth, level, lambda c, s, n, cx, cy: MC.minima(s, n, c.rng, *f(cx, cy), level)), f"{name}: no {depth}-bit case tells at level {level}"


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_a_saturated_cost_sum_and_ties_to_the_last_candidate_change_minima_at_every_level(depth):
    for level in LEVELS:
        assert _caught(depth, level, lambda c, s, n, cx, cy: MC.minima(s, n, c.rng, cx, cy, level, saturate=True)), f"saturated sum: level {level}"
        assert _caught(depth, level, lambda c, s, n, cx, cy: MC.minima(s, n, c.rng, cx, cy, level, last=True)), f"last tie: level {level}"


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_a_total_cut_to_too_few_bits_changes_minima(depth):
    """Every width from 16 bits to one below what the level's largest real total needs."""
    for level in LEVELS:
        need = int(MC.total_max(depth, level)).bit_length()
        assert need > 16
        for bits in range(16, need):
            assert _caught(depth, level, lambda c, s, n, cx, cy: MC.minima(s, n, c.rng, cx, cy, level, bits=bits)), f"{bits} bits: no {depth}-bit case tells at level {level}"


def test_widths_needed_per_level():
    """What the key layouts must hold: cost << 10 leaves 22 bits (8x8), cost << 8 leaves 24 (upper levels, and every level of the record-per-lane kernel), the
    record-per-lane kernel's one-word reduction of the 8x8 / 16x16 levels 18."""
    need = {(d, l): int(MC.total_max(d, l)).bit_length() for d in MC.DEPTHS for l in LEVELS}
    assert [need[8, l] for l in LEVELS] == [18, 18, 19, 21]
    assert [need[10, l] for l in LEVELS] == [18, 19, 21, 23]
    assert [need[12, l] for l in LEVELS] == [19, 21, 23, 25]            # the 64x64 level of 12-bit samples does not fit cost << 8: the generic kernel's 64-bit keys
    assert MC.total_max(8, 1) == 196350 < 0x3ffff                      # 65280 + 2 * 65535 under the 18-bit clamp of pad / idle lanes


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_a_pad_column_in_the_minimum_changes_minima_where_a_real_total_reaches_it(depth):
    """A pad column carries 2^20 (8x8 keys) or 2^23 (upper levels) in place of cost_x.  No real total of 8- or 10-bit samples reaches that - which is what
    lets the fast paths keep the pad columns in their minima - and the 64x64 level of 12-bit samples does: there the cases tell."""
    for level in LEVELS:
        if MC.total_max(depth, level) < MC.PAD_TOTAL[level]:
            assert (depth, level) != (12, 3)
            continue
        assert (depth, level) == (12, 3)
        assert _caught(depth, level, lambda c, s, n, cx, cy: MC.minima(s, n, c.rng, cx, cy, level, pad=True)), "pad column: no 12-bit case tells at 64x64"


LIMITS = {8: (16320, 65280, 1044480, 147390, 1175550), 10: (65472, 261888, 4190208, 196542, 4321278), 12: (262080, 1048320, 16773120, 393150, 16904190)}


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_flat_max_with_u16max_gives_the_limit_totals_in_the_oracles_output(depth):
    """(8x8 SAD, 16x16 SAD, 64x64 SAD, 8x8 total, 64x64 total) at their maxima, exactly; every minimum sits at raster index 0."""
    s8, s16, s64, t8, t64 = LIMITS[depth]
    assert (s16 == 65280) == (depth == 8)                              # the packed-u16 limit of the 8-bit accumulators
    assert (1 << 22) < LIMITS[10][4] < (1 << 23) and LIMITS[12][4] > (1 << 24)
    cases = [c for c in _subset(depth) if (c.content, c.table) == ("flat_max", "u16max")]
    assert cases
    for c in cases:
        v = MC.valid(_surf(c), _nctu(c), c.rng)
        assert v[..., 0:64].min() == v[..., 0:64].max() == s8 and v[..., 64:80].min() == v[..., 64:80].max() == s16 and v[..., 84].min() == v[..., 84].max() == s64
        best = MC.expected_best(*MC.data_key(c)).reshape(-1, 85)
        assert np.all(best[:, 0:64] == np.uint64(t8 << 32)) and np.all(best[:, 84] == np.uint64(t64 << 32)), c.id
        assert np.all(best[:, 64:80] == np.uint64((s16 + 131070) << 32))


@pytest.mark.parametrize("depth", MC.DEPTHS)
def test_contents_do_what_they_are_listed_for(depth):
    """flat content with asym tables: the winner is (argmin cost_x, argmin cost_y) at every level; corner content: the 64x64 PU (whose noise SAD
    dwarfs two capped costs) wins at the displaced corner, with SAD 0; ramp content with capped tables: some 64x64 winner is an interior compromise - neither the
    displacement (SAD 0) nor the cheapest vector; step tables on noise: every 8x8 winner lies inside the free rectangle."""
    seen = set()
    for c in _subset(depth):
        best = MC.expected_best(*MC.data_key(c)).reshape(-1, 85)
        nc = 2 * c.rng + 1
        idx = (best & np.uint64(0xffffffff)).astype(np.int64)
        cx, cy = MC.tables(c.table, c.rng)
        if c.content.startswith("flat") and c.table == "asym":
            ax, ay = MC.asym_minima(c.rng)
            assert np.all(idx == ay * nc + ax), c.id
            seen.add("flat")
        if c.content in MC.CORNER and c.table == "cap":
            sx, sy = MC.CORNER[c.content]
            at = (c.rng + sy * c.rng) * nc + c.rng + sx * c.rng
            assert np.all(idx[:, 84] == at) and np.all(best[:, 84] >> np.uint64(32) == int(cx[at % nc]) + int(cy[at // nc])), c.id
            assert at % nc in (0, nc - 1) and (at == 0 or at % nc == nc - 1)
            seen.add("corner")
        if c.content == "ramp" and c.table == "cap":
            dx, dy = MC.ramp_vector(c.rng)
            there, centre = (c.rng + dy) * nc + c.rng + dx, c.rng * nc + c.rng
            if np.any((idx[:, 80:] != there) & (idx[:, 80:] != centre)):
                seen.add("ramp")
        if c.content == "noise" and c.table == "step":
            x0, x1, y0, y1 = MC.step_window(c.rng)
            i8 = idx[:, :64]
            if MC.sad_max(depth, 0) < 65535:          # an 8x8 SAD cannot buy its way out of the rectangle
                assert np.all((i8 % nc >= x0) & (i8 % nc < x1) & (i8 // nc >= y0) & (i8 // nc < y1)), c.id
            seen.add("step")
    assert seen == {"flat", "corner", "ramp", "step"}, seen
