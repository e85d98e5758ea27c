"""CPU-only checks of the merge stage of a P picture (x265hip_merge_decide): declaration, export, record layout and argument validation of
the entry, and the expectation the GPU tests compare against (tests/merge_expect.py): hand-worked candidate lists written out from the
statements of cudata.cpp, the limits of the walk, what the cases of tests/merge_cases.py reach (the coverage condition), that every
mutation of the walk - what a wrong kernel would compute - changes the expectation of a counted number of cases, and, where oracle/_ref is
built, the clipped predictions against the reference's own Predict::motionCompensation."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import missing_reference_build

import merge_cases as C
import merge_expect as ME

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
EINVAL, ENODEV = -2, -1
KEYS = ("merge", "merge_idx", "mv_out", "mv_pred", "cost", "best")


def test_the_entry_is_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_merge_decide\(const x265hip_merge_decide_params\* p, void\* stream\);", hdr)
    assert "x265hip_merge_decide" in A.exported_symbols() and hasattr(A.lib(), "x265hip_merge_decide")
    assert callable(A.merge_decide)
    rec = A.MergeDecideParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_merge_decide_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_merge_decide_params, {f}));' for f, _ in rec._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, val = line.split()
        want = ctypes.sizeof(rec) if name == "." else getattr(rec, name).offset
        assert int(val) == want, f"x265hip_merge_decide_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(rec._fields_) + 1 == 23


def _params():
    p = A.MergeDecideParams()
    p.depth, p.width, p.height, p.level, p.qp, p.lambda8, p.max_merge = 8, 128, 64, 2, 30, 1024, 3
    p.fenc, p.fenc_stride, p.fref, p.fref_stride = 0x10000, 320, 0x20000, 320
    p.mv, p.inter_cost, p.inter_cost_stride = 0x30000, 0x40000, 2
    p.merge, p.merge_idx, p.mv_out, p.mv_pred, p.cost, p.best = 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000
    return p


def test_merge_decide_validates_before_touching_a_device():
    import torch
    f = A.lib().x265hip_merge_decide
    f.argtypes = [ctypes.POINTER(A.MergeDecideParams), ctypes.c_void_p]
    assert f(None, None) == EINVAL

    def bad(**kw):
        p = _params()
        for k, v in kw.items():
            setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for req in ("fenc", "fref", "mv", "inter_cost", "merge", "merge_idx", "mv_out", "mv_pred", "cost"):
        assert bad(**{req: None}) == EINVAL, req
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64), ("fenc_stride", 127), ("fref_stride", 64)):
        assert bad(**{k: v}) == EINVAL, k
    for k, v in (("lambda8", -1), ("lambda8", (1 << 24) + 1), ("qp", 52), ("qp", -1), ("inter_cost_stride", 0), ("inter_cost_stride", -2)):
        assert bad(**{k: v}) == EINVAL, (k, v)
    for mm in (0, 6, -1):
        assert bad(max_merge=mm) == EINVAL
    assert b"max_merge" in A.lib().x265hip_last_error()
    assert bad(mv_out=0x30000) == EINVAL and bad(mv_pred=0x30000) == EINVAL and bad(mv_out=0x80000) == EINVAL          # mv_out == mv_pred
    assert b"alias" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        assert bad() == ENODEV and bad(best=None, max_merge=1) == ENODEV and bad(max_merge=5, depth=12, qp=75, level=0, lambda8=1 << 24, inter_cost_stride=1) == ENODEV


def test_hand_worked_candidate_lists():
    """One list per rule, written out from the statements of getInterMergeCandidates (cudata.cpp:1495-1593, 1676-1710)."""
    a, b, c, d, e = (ME.pack(*v) for v in ((4, 0), (0, 8), (-12, 3), (7, 7), (-1, -1)))
    L = lambda nb, mm, mut=None: [m for m, _ in ME.candidate_list(nb, mm, mut)[0]]
    origins = lambda nb, mm: [o for _, o in ME.candidate_list(nb, mm)[0]]
    flags = lambda nb, mm: {k for k, v in ME.candidate_list(nb, mm)[1].items() if v}
    none = dict(A1=None, B1=None, B0=None, A0=None, B2=None)
    # no neighbour: the zero candidates
    assert L(none, 3) == [0, 0, 0] and origins(none, 2) == ["zero", "zero"]
    # the order A1, B1, B0, A0; B2 is not looked at once four are in the list (:1573)
    full = dict(A1=a, B1=b, B0=c, A0=d, B2=e)
    assert L(full, 5) == [a, b, c, d, 0] and flags(full, 5) == {"B2_dropped_at_four"}
    assert L(full, 5, "b2_regardless_of_count") == [a, b, c, d, e]
    # B2 enters while fewer than four are in the list
    assert L(dict(full, A0=None), 5) == [a, b, c, e, 0] and origins(dict(full, A0=None), 5)[3] == "B2"
    # returned once count == max_merge (:1508, :1530, :1549, :1568)
    assert L(full, 1) == [a] and L(full, 2) == [a, b] and L(full, 3) == [a, b, c] and L(full, 4) == [a, b, c, d]
    assert flags(full, 2) == {"cut_at_max"} and flags(dict(none, A1=a), 1) == set()
    # B1 against A1 (:1521)
    assert L(dict(full, B1=a), 5) == [a, c, d, e, 0] and "pruned_B1" in flags(dict(full, B1=a), 5)
    # B0 against B1 only (:1540): a B0 equal to A1 stays, and is priced with its own index
    assert L(dict(full, B0=b), 5) == [a, b, d, e, 0] and "pruned_B0" in flags(dict(full, B0=b), 5)
    assert L(dict(full, B0=a), 5) == [a, b, a, d, 0] and "B0_equals_A1_kept" in flags(dict(full, B0=a), 5)
    assert L(dict(full, B0=a), 5, "prune_every_pair") == [a, b, d, e, 0]
    # a B0 equal to a B1 that is not available is not pruned
    assert L(dict(full, B1=None, B0=a), 5) == [a, a, d, e, 0]
    # A0 against A1 only (:1559): an A0 equal to B1 or B0 stays
    assert L(dict(full, A0=a), 5) == [a, b, c, e, 0] and "pruned_A0" in flags(dict(full, A0=a), 5)
    assert L(dict(full, A0=b), 5) == [a, b, c, b, 0] and L(dict(full, A0=c), 5) == [a, b, c, c, 0]
    # B2 against A1 and against B1 (:1580-1581), not against B0 / A0
    three = dict(full, A0=None)
    assert L(dict(three, B2=a), 5) == [a, b, c, 0, 0] and L(dict(three, B2=b), 5) == [a, b, c, 0, 0] and L(dict(three, B2=c), 5) == [a, b, c, c, 0]
    assert "pruned_B2" in flags(dict(three, B2=b), 5)
    # a zero vector among the neighbours is a candidate like any other, and the fill repeats it
    assert L(dict(none, A1=0, B1=a), 4) == [0, a, 0, 0]


def test_clip_and_index_bits_are_the_reference_statements():
    # clipMv (cudata.cpp:1915-1928) for a 192 x 128 picture
    assert ME.clip_mv(ME.pack(400, -400), 160, 0, 192, 128) == ME.pack((192 + 8 - 160 - 1) << 2, -((64 + 8 + 0 - 1) << 2))
    assert ME.clip_mv(ME.pack(-400, 400), 0, 96, 192, 128) == ME.pack(-((64 + 8 - 1) << 2), (128 + 8 - 96 - 1) << 2)
    assert ME.clip_mv(ME.pack(156, -284), 160, 0, 192, 128) == ME.pack(156, -284)                 # the limits themselves are kept
    assert ME.unpack(ME.pack(-301, 231)) == (-301, 231)
    # getTUBits (search.h:246-249)
    assert [ME.tu_bits(i, 5) for i in range(5)] == [1, 2, 3, 4, 4] and [ME.tu_bits(i, 3) for i in range(3)] == [1, 2, 2]
    assert ME.tu_bits(0, 1) == 0 and ME.tu_bits(1, 2) == 1 and ME.tu_bits(2, 3, "tu_bits_without_saving") == 3


# a mask that cannot reach 3 % of a level's blocks for a reason of geometry: (mask, level) -> (the largest possible share, the reason)
GEOMETRY = {
    ("B0_from_above_right_ctu", 0): (2 / 384, "only the block at the upper right corner of a CTU has its B0 in the above-right CTU, and only CTUs (0, 1) and (1, 1) of "
                                              "192x128 have one: 2 of 384 blocks; 64x64, 64x192 and 256x64 have no such CTU"),
    ("B0_from_above_right_ctu", 1): (2 / 96, "as at level 0: 2 of 96 blocks"),
}


@pytest.mark.parametrize("level", [0, 1, 2])
def test_the_cases_reach_every_outcome(level):
    """The coverage condition: at each level every mask holds for at least 3 % of the blocks of at least one case - or, where geometry
    bounds it below that, reaches the bound GEOMETRY names."""
    best = {k: (0.0, None) for k in ME.MASKS}
    for c in C.COVER_CASES:
        if c.level == level:
            for k, m in C.expectation(c)["e"]["masks"].items():
                if float(m.mean()) > best[k][0]:
                    best[k] = (float(m.mean()), c.id)
    for k, (share, cid) in best.items():
        print(level, k, round(share, 4), cid)
    print("smallest share at level", level, min((s, k) for k, (s, _) in best.items() if (k, level) not in GEOMETRY))
    for k, (share, cid) in best.items():
        if (k, level) in GEOMETRY:
            bound, reason = GEOMETRY[(k, level)]
            assert bound < 0.03 and abs(share - bound) < 1e-9, (k, level, share, reason)
        else:
            assert share >= 0.03, (level, k, share)


# cases of COVER_CASES (36) whose expectation a mutation changes: the numbers of DESIGN.md section 19
MUTATION_COUNTS = {"le_against_inter": 21, "le_among_candidates": 12, "prune_every_pair": 5, "b2_regardless_of_count": 6, "searched_not_final": 24, "no_clip": 9,
                   "clip_stored": 9, "available_by_position": 23, "tu_bits_without_saving": 18}


def test_mutations_of_the_walk_change_the_counted_cases():
    """Each mutation changes the expectation of exactly MUTATION_COUNTS cases - at least one each; `<=` against the inter cost changes
    exactly the pattern cases."""
    assert set(MUTATION_COUNTS) == set(ME.MUTATIONS)
    for mut in ME.MUTATIONS:
        hit = []
        for c in C.COVER_CASES:
            want, got = C.expectation(c)["e"], C.run_stage(c, mutation=mut)
            if any(not np.array_equal(want[k], got[k]) for k in KEYS):
                hit.append(c.id)
        print(mut, len(hit), "of", len(C.COVER_CASES), hit)
        assert hit and len(hit) == MUTATION_COUNTS[mut], (mut, len(hit))
        if mut == "le_against_inter":
            assert hit == [c.id for c in C.COVER_CASES if c.costs == "pattern"]


@pytest.mark.parametrize("c", [C.COVER_CASES[1], C.COVER_CASES[12 + 8], C.COVER_CASES[24 + 5]], ids=lambda c: c.id)
def test_limits_of_the_walk(c):
    """max_merge = 1 with an inter cost nothing beats: every block merges with index 0.  An inter cost of 0: nothing merges, and mv_out and
    mv_pred are the searched records word for word - so the TU stages are handed what FramePipeline hands them (only the records are
    checked: the coding of equal records is the same call)."""
    x = C.inputs(c)
    nctu = (c.w // 64) * (c.h // 64)
    sl = ME.level_slots(c.level, nctu)
    n = len(sl)
    hi = C.run_stage(c, inter_cost=np.full(n, 0x7fffffff, np.int64), max_merge=1)
    assert hi["merge"].all() and not hi["merge_idx"].any() and np.array_equal(hi["best"], hi["cost"])
    assert np.array_equal(hi["mv_out"][:, 0], hi["cost"][:, 1])
    lo = C.run_stage(c, inter_cost=np.zeros(n, np.int64))
    assert not lo["merge"].any() and not lo["merge_idx"].any() and (lo["best"] == np.array([-1, 0])).all()
    assert np.array_equal(lo["mv_pred"], x["mv"][sl]) and np.array_equal(lo["mv_out"], x["mv"][sl])
    assert np.array_equal(ME.records(lo["mv_pred"][:, 1], lo["mv_pred"][:, 0], c.level, nctu), x["mv"])
    assert not ME.skip_flags(lo["merge"], np.zeros(n, np.int32)).any() and ME.skip_flags(hi["merge"], np.arange(n) % 2).tolist() == [1, 0] * (n // 2)


def test_lambda_zero_ties_go_to_the_lowest_index():
    """At lambda8 = 0 the index is free: among candidates of equal sa8d the first wins (strict <, analysis.cpp:2833)."""
    c = next(c for c in C.COVER_CASES if c.lambda8 == 0 and c.level == 1)
    x = C.expectation(c)
    e = x["e"]
    assert e["masks"]["tie_lowest_index"].any()
    assert (e["cost"][:, 0] == e["cost"][:, 1]).all()
    flat = C.expectation(next(c for c in C.COVER_CASES if c.field == "flat" and c.level == 0))["e"]
    assert flat["merge"].all() and not flat["merge_idx"].any() and (flat["cost"][:, 0] == 0).all()


REF_CASES = [c for c in C.COVER_CASES if c.field == "far_edge" and c.costs == "pattern" and c.max_merge == 3] + [c for c in C.DEEP_CASES if c.field == "far_edge"]


@pytest.mark.parametrize("c", REF_CASES, ids=lambda c: c.id)
def test_clipped_predictions_equal_the_reference_motion_compensation(c):
    """clipMv against compiled reference code: the UNCLIPPED mv_out records of a far_edge case go to x265ref_motion_compensation (the real
    Predict::motionCompensation per 2Nx2N CU, which clips with CUData::clipMv, predict.cpp:92); its luma prediction must equal the
    oracle's prediction of the mv_pred records on every merged block - clipped here - and on every block that kept a searched vector
    inside clipMv's range (the stage codes a searched vector untouched; the reference would clip it too).  Levels 0 - 2 at 8 bits, level 1
    at 10; vectors beyond both limits are among the merged blocks'."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", f"libx265ref{c.depth}.so")
    if not os.path.exists(path):
        missing_reference_build()
    lib = ctypes.CDLL(path)
    if not hasattr(lib, "x265ref_motion_compensation"):
        pytest.skip("oracle/_ref predates x265ref_motion_compensation")
    x = C.expectation(c)
    e = x["e"]
    nctu = (c.w // 64) * (c.h // 64)
    n = 8 << c.level
    full = lambda recs: ME.records(recs[:, 1], recs[:, 0], c.level, nctu)
    want = ME.reference_prediction(lib, x["pref"], c.w, c.h, c.level, full(e["mv_out"]))
    got = ME.oracle_prediction(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level, full(e["mv_pred"]))
    pr = x["pricer"]
    low = high = compared = 0
    for b in range(len(e["merge"])):
        gx, gy = pr.position(b)
        v = int(e["vec_out"][b])
        cl = ME.clip_mv(v, gx, gy, c.w, c.h)
        if e["merge"][b]:
            assert cl == int(e["vec_pred"][b])
            (qx, qy), (cx, cy) = ME.unpack(v), ME.unpack(cl)
            low += cx > qx or cy > qy
            high += cx < qx or cy < qy
        elif cl != v:
            continue
        compared += 1
        assert np.array_equal(got[gy:gy + n, gx:gx + n], want[gy:gy + n, gx:gx + n]), (b, ME.unpack(v), ME.unpack(cl))
    print(c.id, "blocks compared", compared, "of", len(e["merge"]), "merged beyond the upper limit", high, "beyond the lower limit", low)
    assert high > 0 and compared >= len(e["merge"]) // 2
    assert low > 0 or c.level == 2, "a merged block beyond clipMv's lower limit"
