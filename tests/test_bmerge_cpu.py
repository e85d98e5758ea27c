"""CPU-only checks of the merge stage of a B picture (x265hip_b_merge_decide): declaration, export, record layout and argument validation
of the entry, and the expectation the GPU tests compare against (tests/bmerge_expect.py): hand-worked candidate lists written out from the
statements of cudata.cpp, the limits of the walk, what the cases of tests/bmerge_cases.py reach (the coverage condition), that every
mutation of the walk - what a wrong kernel would compute - changes the expectation of a counted number of cases, and, where oracle/_ref is
built, the clipped two-list predictions against the reference's own Predict::motionCompensation."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
from conftest import missing_reference_build

import bmerge_cases as C
import bmerge_expect as BM

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
EINVAL, ENODEV = -2, -1
KEYS = BM.OUTPUTS
RECORDS = ("mv0", "mv1", "mv0_out", "mv1_out", "mv0_pred", "mv1_pred")


def test_the_entry_is_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_b_merge_decide\(const x265hip_b_merge_decide_params\* p, void\* stream\);", hdr)
    assert "x265hip_b_merge_decide" in A.exported_symbols() and hasattr(A.lib(), "x265hip_b_merge_decide")
    assert callable(A.b_merge_decide)
    rec = A.BMergeDecideParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_b_merge_decide_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_b_merge_decide_params, {f}));' for f, _ in rec._fields_]
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
        assert int(val) == want, f"x265hip_b_merge_decide_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(rec._fields_) + 1 == 33


def _params():
    p = A.BMergeDecideParams()
    p.depth, p.width, p.height, p.level, p.qp, p.lambda8, p.max_merge, p.ref_id0, p.ref_id1 = 8, 128, 64, 2, 30, 1024, 3, 0, 1
    p.fenc, p.fenc_stride, p.fref0, p.fref1, p.fref_stride = 0x10000, 320, 0x20000, 0x28000, 320
    p.dir_in, p.mv0, p.mv1, p.inter_cost, p.inter_cost_stride = 0x30000, 0x40000, 0x50000, 0x60000, 4
    p.merge, p.merge_idx, p.dir, p.ref0, p.ref1 = 0x70000, 0x71000, 0x72000, 0x73000, 0x74000
    p.mv0_out, p.mv1_out, p.mv0_pred, p.mv1_pred, p.cost, p.best = 0x80000, 0x90000, 0xa0000, 0xb0000, 0xc0000, 0xd0000
    return p


def test_b_merge_decide_validates_before_touching_a_device():
    import torch
    f = A.lib().x265hip_b_merge_decide
    f.argtypes = [ctypes.POINTER(A.BMergeDecideParams), ctypes.c_void_p]
    assert f(None, None) == EINVAL

    def bad(**kw):
        p = _params()
        for k, v in kw.items():
            setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for req in ("fenc", "fref0", "fref1", "dir_in", "mv0", "mv1", "inter_cost", "merge", "merge_idx", "dir", "mv0_out", "mv1_out", "mv0_pred", "mv1_pred", "cost"):
        assert bad(**{req: None}) == EINVAL, req
        assert b"NULL" in A.lib().x265hip_last_error()
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
    base = _params()
    for out in RECORDS[2:]:                                   # every output record array against every input and every other output
        for other in RECORDS:
            if other != out:
                assert bad(**{out: getattr(base, other)}) == EINVAL, (out, other)
                assert b"alias" in A.lib().x265hip_last_error()
    assert bad(dir=0x30000) == EINVAL and b"alias" in A.lib().x265hip_last_error()                      # dir == dir_in
    if not torch.cuda.is_available():
        assert bad() == ENODEV and bad(best=None, ref0=None, ref1=None, max_merge=1) == ENODEV and bad(mv1=0x40000, ref_id1=0) == ENODEV
        assert bad(max_merge=5, depth=12, qp=75, level=0, lambda8=1 << 24, inter_cost_stride=1) == ENODEV


def test_hand_worked_candidate_lists():
    """One list per rule, written out from the statements of getInterMergeCandidates (cudata.cpp:1495-1593, 1652-1709) and hasEqualMotion
    (:1439-1455).  u, v, w, x: packed vectors; M(d, v0, v1): a neighbour's motion."""
    u, v, w, x, y = (BM.pack(*q) for q in ((4, 0), (0, 8), (-12, 3), (7, 7), (-1, -1)))
    M = BM.motion
    L = lambda nb, mm, same=False, mut=None: [m[:3] for m, _ in BM.candidate_list(nb, mm, same, mut)[0]]
    origins = lambda nb, mm, same=False: [o for _, o in BM.candidate_list(nb, mm, same)[0]]
    flags = lambda nb, mm, same=False: {k for k, f in BM.candidate_list(nb, mm, same)[1].items() if f}
    none = dict(A1=None, B1=None, B0=None, A0=None, B2=None)
    Z = (3, 0, 0)
    # all-zero fill at an unavailable corner: no neighbour, every entry {3, (0,0), (0,0)} (:1687-1698)
    assert L(none, 3) == [Z, Z, Z] and origins(none, 2) == ["zero", "zero"] and L(none, 2, mut="uni_zero_fill") == [(1, 0, 0)] * 2
    # one neighbour: count 1, cutoff 0, no combined candidate - not even from a bidirectional neighbour
    assert L(dict(none, A1=M(3, u, v)), 3) == [(3, u, v), Z, Z]
    # an unused list's vector is never read: stored as 0 whatever the neighbour's arrays hold
    assert L(dict(none, A1=M(1, u, x)), 1) == [(1, u, 0)] and L(dict(none, B1=M(2, x, v)), 1) == [(2, 0, v)]
    # hasEqualMotion: equal directions and equal vectors of the used lists prune (B1 against A1, :1521) ...
    assert L(dict(none, A1=M(1, u, x), B1=M(1, u, y)), 2) == [(1, u, 0), Z] and "pruned_B1" in flags(dict(none, A1=M(1, u, x), B1=M(1, u, y)), 2)
    assert "pruned_needs_both_lists" in flags(dict(none, A1=M(3, u, v), B1=M(3, u, v)), 2)
    assert L(dict(none, A1=M(3, u, v), B1=M(3, u, w)), 3)[:2] == [(3, u, v), (3, u, w)]              # list 1 differs: kept
    # ... and a pruning that fails only because the directions differ: the same list-0 vector with directions 1 and 3 is different motion
    nb = dict(none, A1=M(1, u, 0), B1=M(3, u, v))
    assert L(nb, 2) == [(1, u, 0), (3, u, v)] and "kept_because_dir_differs" in flags(nb, 2)
    assert L(nb, 2, mut="equal_motion_ignores_dir") == [(1, u, 0), Z]
    # the stale vector of an unused list does not keep two motions apart
    assert L(dict(none, A1=M(1, u, x), B1=M(1, u, y)), 2, mut="equal_motion_compares_unused") == [(1, u, 0), (1, u, 0)]
    # the pruned pairs are B1-A1, B0-B1, A0-A1, B2-A1, B2-B1 and no other: a B0 equal to A1 stays, an A0 equal to B1 stays
    a, b = M(1, u, 0), M(2, 0, v)
    assert L(dict(none, A1=a, B1=b, B0=a), 3) == [a[:3], b[:3], a[:3]] and "B0_equals_A1_kept" in flags(dict(none, A1=a, B1=b, B0=a), 3)
    assert L(dict(none, A1=a, B1=b, B0=b), 3)[:2] == [a[:3], b[:3]] and "pruned_B0" in flags(dict(none, A1=a, B1=b, B0=b), 5)
    assert L(dict(none, A1=a, B1=b, A0=b), 3) == [a[:3], b[:3], b[:3]] and "pruned_A0" in flags(dict(none, A1=a, B1=b, A0=a), 5)
    assert "pruned_B2" in flags(dict(none, A1=a, B1=b, B2=b), 5) and "pruned_B2" in flags(dict(none, A1=a, B1=b, B2=a), 5)
    # the combined order at count 2: cutoff 2, pairs (0,1) (1,0) (:1655-1661).  A1 = {1, u}, B1 = {2, v}: (0,1) gives {3, u, v}, (1,0) nothing
    assert L(dict(none, A1=a, B1=b), 5) == [a[:3], b[:3], (3, u, v), Z, Z] and origins(dict(none, A1=a, B1=b), 5)[2:] == ["combined", "zero", "zero"]
    # ... two bidirectional neighbours give both crosses, (0,1) first
    p, q = M(3, u, v), M(3, w, x)
    assert L(dict(none, A1=p, B1=q), 5) == [p[:3], q[:3], (3, u, x), (3, w, v), Z]
    assert L(dict(none, A1=p, B1=q), 5, mut="combined_order_swapped") == [p[:3], q[:3], (3, w, v), (3, u, x), Z]
    # count 3: cutoff 6, pairs (0,1) (1,0) (0,2) (2,0) (1,2) (2,1)
    r = M(3, y, u)
    three = dict(none, A1=p, B1=q, B0=r)
    assert L(three, 5) == [p[:3], q[:3], r[:3], (3, u, x), (3, w, v)] and "cut_inside_combined" in flags(three, 5)
    # ... with single-list candidates only the pairs whose first uses list 0 and whose second list 1: A1 {1,u} B1 {2,v} B0 {1,w}: (0,1) -> u,v;
    # (1,0) no; (0,2) no (B0 has no list 1); (2,0) no; (1,2) no; (2,1) -> w,v
    assert L(dict(none, A1=a, B1=b, B0=M(1, w, 0)), 5) == [a[:3], b[:3], (1, w, 0), (3, u, v), (3, w, v)]
    # count 4: cutoff 12, the order goes on (0,3) (3,0) (1,3) (3,1) (2,3) (3,2); only the fourth candidate has list 1 here
    four = dict(none, A1=M(1, u, 0), B1=M(1, v, 0), B0=M(1, w, 0), A0=M(2, 0, x), B2=M(3, y, y))
    assert L(four, 5) == [(1, u, 0), (1, v, 0), (1, w, 0), (2, 0, x), (3, u, x)] and "B2_dropped_at_four" in flags(four, 5)
    assert BM.combined_pairs() == [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (0, 3), (3, 0), (1, 3), (3, 1), (2, 3), (3, 2)]
    # cutoff is fixed before the loop: with count 2 only (0,1) and (1,0) are looked at, although the list grows to 3 and (0,2) would then
    # pair A1 with the new combined candidate
    assert L(dict(none, A1=a, B1=M(3, w, x)), 5) == [a[:3], (3, w, x), (3, u, x), Z, Z]
    assert L(dict(none, A1=a, B1=M(3, w, x)), 5, mut="cutoff_recomputed") == [a[:3], (3, w, x), (3, u, x), (3, u, x), (3, w, x)]
    # the same-picture suppression (:1670): both lists name one picture and the two vectors are equal
    same = dict(none, A1=M(1, u, 0), B1=M(2, 0, u))
    assert L(same, 4, True) == [(1, u, 0), (2, 0, u), Z, Z] and "combined_suppressed_same_picture" in flags(same, 4, True)
    assert L(same, 4, False)[2] == (3, u, u) and L(same, 4, True, "no_same_picture_suppression")[2] == (3, u, u)
    assert L(dict(none, A1=M(1, u, 0), B1=M(2, 0, v)), 4, True)[2] == (3, u, v)                     # other vectors: kept
    # returned once count == max_merge: among the spatial candidates, and inside the combined loop (:1678)
    full = dict(none, A1=p, B1=q, B0=r, A0=M(1, x, 0), B2=M(2, 0, y))
    assert L(full, 1) == [p[:3]] and L(full, 2) == [p[:3], q[:3]] and L(full, 4) == [p[:3], q[:3], r[:3], (1, x, 0)]
    assert flags(full, 2) == {"cut_at_max"} and L(dict(none, A1=p, B1=q), 3) == [p[:3], q[:3], (3, u, x)]
    assert "cut_inside_combined" in flags(dict(none, A1=p, B1=q), 3) and "cut_inside_combined" not in flags(dict(none, A1=p, B1=q), 5)
    # B2 enters while fewer than four are in the list
    assert L(dict(full, A0=None), 4)[3] == (2, 0, y)


def test_clip_and_index_bits_are_the_reference_statements():
    assert BM.clip_mv(BM.pack(400, -400), 160, 0, 192, 128) == BM.pack((192 + 8 - 160 - 1) << 2, -((64 + 8 + 0 - 1) << 2))
    assert [BM.tu_bits(i, 5) for i in range(5)] == [1, 2, 3, 4, 4] and BM.tu_bits(0, 1) == 0
    assert BM.has_equal_motion(BM.motion(1, 5, 9), BM.motion(1, 5, 7)) and not BM.has_equal_motion(BM.motion(3, 5, 9), BM.motion(3, 5, 7))
    assert not BM.has_equal_motion(BM.motion(1, 5, 0), BM.motion(3, 5, 0))


# a mask that cannot reach 3 % of a level's blocks for a reason of geometry: (mask, level) -> (the largest possible share, the reason)
GEOMETRY = {
    ("B0_from_above_right_ctu", 0): (2 / 384, "only the block at the upper right corner of a CTU has its B0 in the above-right CTU, and only CTUs (0, 1) and (1, 1) of "
                                              "192x128 have one: 2 of 384 blocks (DESIGN.md section 19)"),
    ("B0_from_above_right_ctu", 1): (2 / 96, "as at level 0: 2 of 96 blocks"),
}


@pytest.mark.parametrize("level", [0, 1, 2])
def test_the_cases_reach_every_outcome(level):
    """The coverage condition: at each level every mask holds for at least 3 % of the blocks of at least one case - or, where geometry
    bounds it below that, reaches the bound GEOMETRY names."""
    best = {k: (0.0, None) for k in BM.MASKS}
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


# cases of COVER_CASES (51) whose expectation a mutation changes: the numbers of DESIGN.md section 20
MUTATION_COUNTS = {"le_against_inter": 30, "le_among_candidates": 26, "equal_motion_ignores_dir": 29, "equal_motion_compares_unused": 1, "cutoff_recomputed": 11,
                   "combined_order_swapped": 18, "no_same_picture_suppression": 3, "uni_zero_fill": 51, "avg_of_rounded": 45, "no_clip_list1": 9,
                   "clip_stored_list1": 9, "inter_winner_not_final": 37}


def test_mutations_of_the_walk_change_the_counted_cases():
    """Each mutation changes the expectation of exactly MUTATION_COUNTS cases - at least one each; `<=` against the inter cost changes
    exactly the pattern cases."""
    assert set(MUTATION_COUNTS) == set(BM.MUTATIONS)
    for mut in BM.MUTATIONS:
        hit = []
        for c in C.COVER_CASES:
            want, got = C.expectation(c)["e"], C.run_stage(c, mutation=mut)
            if any(not np.array_equal(want[k], got[k]) for k in KEYS):
                hit.append(c.id)
        print(mut, len(hit), "of", len(C.COVER_CASES), hit)
        assert hit and len(hit) == MUTATION_COUNTS[mut], (mut, len(hit))
        if mut == "le_against_inter":
            assert hit == [c.id for c in C.COVER_CASES if c.costs == "pattern"]


@pytest.mark.parametrize("c", [C.COVER_CASES[1], C.COVER_CASES[17 + 10], C.COVER_CASES[34 + 5]], ids=lambda c: c.id)
def test_limits_of_the_walk(c):
    """max_merge = 1 with an inter cost nothing beats: every block merges with index 0.  An inter cost of 0: nothing merges; dir and
    mv*_pred are the inter winner word for word - the TU stages are handed what Sa8dBFramePipeline hands them - and mv*_out differ from it
    only in the vector of an unused list, which is 0."""
    x = C.inputs(c)
    sl = BM.level_slots(c.level, x["nctu"])
    n = len(sl)
    hi = C.run_stage(c, inter_cost=np.full(n, 0x7fffffff, np.int64), max_merge=1)
    assert hi["merge"].all() and not hi["merge_idx"].any() and np.array_equal(hi["best"], hi["cost"])
    for l in (0, 1):
        used = hi["ref_used"][:, l]
        assert np.array_equal(hi["mv%d_out" % l][used, 0], hi["cost"][used, 1]) and np.array_equal(hi["mv%d_out" % l][~used, 0], x["mv%d" % l][sl][~used, 0])
        assert not hi["mv%d_out" % l][~used, 1].any() and not hi["mv%d_pred" % l][~used, 1].any() and (hi["ref%d" % l][~used] == -1).all()
    lo = C.run_stage(c, inter_cost=np.zeros(n, np.int64))
    assert not lo["merge"].any() and not lo["merge_idx"].any() and (lo["best"] == np.array([-1, 0])).all()
    assert np.array_equal(lo["dir"], x["dir_in"])
    for l in (0, 1):
        used = (x["dir_in"] & (1 << l)) != 0
        assert np.array_equal(lo["mv%d_pred" % l], x["mv%d" % l][sl])
        assert np.array_equal(BM.full_records(lo["mv%d_pred" % l], c.level, x["nctu"]), x["mv%d" % l])
        assert np.array_equal(lo["mv%d_out" % l][used], x["mv%d" % l][sl][used]) and np.array_equal(lo["mv%d_out" % l][:, 0], x["mv%d" % l][sl][:, 0])
        assert not lo["mv%d_out" % l][~used, 1].any() and np.array_equal(lo["ref%d" % l] >= 0, used)
    assert not BM.skip_flags(lo["merge"], np.zeros(n, np.int32)).any() and BM.skip_flags(hi["merge"], np.arange(n) % 2).tolist() == [1, 0] * (n // 2)


def test_lambda_zero_ties_go_to_the_lowest_index():
    """At lambda8 = 0 the index is free: among candidates of equal sa8d the first wins (strict <, analysis.cpp:2833)."""
    c = next(c for c in C.COVER_CASES if c.lambda8 == 0 and c.level == 1)
    e = C.expectation(c)["e"]
    assert e["masks"]["tie_lowest_index"].any() and (e["cost"][:, 0] == e["cost"][:, 1]).all()
    flat = C.expectation(next(c for c in C.COVER_CASES if c.kind == "flat" and c.level == 0))["e"]
    assert flat["merge"].all() and not flat["merge_idx"].any() and (flat["cost"][:, 0] == 0).all() and (flat["dir"] == 3).all()


def test_the_walk_decides_like_the_reference_sequence():
    """analysis.cpp:1650-1655 in its own order - merge first, the single list when strictly cheaper, both lists when strictly cheaper than
    what stands - against `inter_cost < merge` with bsa8d_expect.decide's dir, on the decisions of the `real` cases."""
    seen = set()
    for c in C.COVER_CASES:
        if c.costs != "real":
            continue
        x = C.expectation(c)
        d, e = x["decision"], x["e"]
        for b in range(len(e["merge"])):
            merge_cost, uni, bi = int(e["cost"][b, 1]), int(d["cost"][b, 1]), int(d["cost"][b, 2])
            mode, stands = "merge", merge_cost
            if uni < stands:
                mode, stands = "uni", uni
            if bi < stands:
                mode, stands = "bi", bi
            assert (mode == "merge") == bool(e["merge"][b]), (c.id, b)
            if mode != "merge":
                assert (mode == "bi") == (d["dir"][b] == 3) and e["dir"][b] == d["dir"][b] and stands == d["cost"][b, 0]
            seen.add(mode)
    assert seen == {"merge", "uni", "bi"}


REF_CASES = [c for c in C.COVER_CASES if c.kind == "far_edge" and c.max_merge != 1] + [c for c in C.DEEP_CASES if c.kind == "far_edge"]


@pytest.mark.parametrize("c", REF_CASES, ids=lambda c: c.id)
def test_clipped_predictions_equal_the_reference_motion_compensation(c):
    """clipMv on both lists against compiled reference code: the final dir and the UNCLIPPED mv*_out records of a far_edge case go to
    x265ref_motion_compensation with sliceB = 1 (the real Predict::motionCompensation per 2Nx2N CU, which clips every used vector with
    CUData::clipMv); its luma prediction must equal the oracle's prediction of the mv*_pred records on every merged block - clipped here -
    and on every other block whose used vectors lie inside clipMv's range."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", f"libx265ref{c.depth}.so")
    if not os.path.exists(path):
        missing_reference_build()
    lib = ctypes.CDLL(path)
    if not hasattr(lib, "x265ref_motion_compensation"):
        pytest.skip("oracle/_ref predates x265ref_motion_compensation")
    x = C.expectation(c)
    e = x["e"]
    nctu, n = x["nctu"], 8 << c.level
    full = lambda recs: BM.full_records(recs, c.level, nctu)
    want = BM.reference_prediction(lib, x["pref"], c.w, c.h, c.level, e["dir"], full(e["mv0_out"]), full(e["mv1_out"]))
    got = BM.oracle_prediction(c.depth, x["pcur"], x["pref"], c.w, c.h, c.level, e["dir"], full(e["mv0_pred"]), full(e["mv1_pred"]))
    pr = x["pricer"]
    clipped = [0, 0]
    compared = 0
    for b in range(len(e["merge"])):
        gx, gy = pr.position(b)
        inside = True
        for l in (0, 1):
            if e["ref_used"][b, l]:
                v = int(e["vec_out"][b, l])
                cl = BM.clip_mv(v, gx, gy, c.w, c.h)
                if e["merge"][b]:
                    assert cl == int(e["vec_pred"][b, l])
                    clipped[l] += cl != v
                inside &= cl == v
        if not e["merge"][b] and not inside:
            continue
        compared += 1
        assert np.array_equal(got[gy:gy + n, gx:gx + n], want[gy:gy + n, gx:gx + n]), (b, int(e["dir"][b]))
    print(c.id, "blocks compared", compared, "of", len(e["merge"]), "merged blocks clipped in list 0 / list 1", clipped)
    assert compared >= len(e["merge"]) // 2 and clipped[0] > 0 and clipped[1] > 0
