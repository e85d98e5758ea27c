"""CPU-only checks of the chroma-SATD flavours (x265hip_subpel_refine_chroma, x265hip_bidir_decide_chroma): declarations, exports, record
layouts and argument validation, and - with the oracle alone - the conditions that keep the GPU comparisons of
tests/test_gpu_subpel_chroma.py from passing on degenerate inputs."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import bidir_expect as BE
import subpel_cases as SC
import subpel_chroma_cases as CC
import subpel_chroma_expect as CE

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
F = importlib.import_module("x265-yuuki-asuna_amd.frames")

EINVAL, ENODEV = -2, -1


@pytest.mark.parametrize("cname,rec,nfields", [("x265hip_subpel_chroma", "SubpelChroma", 6), ("x265hip_bidir_chroma", "BidirChroma", 8)])
def test_chroma_records_are_laid_out_like_the_header(repo_root, tmp_path, cname, rec, nfields):
    R = getattr(A, rec)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {', f'  printf(". %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in R._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, val = line.split()
        want = ctypes.sizeof(R) if name == "." else getattr(R, name).offset
        assert int(val) == want, f"{cname}.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(R._fields_) + 1 == nfields + 1


def test_chroma_entries_are_declared_exported_and_documented(repo_root):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_subpel_refine_chroma\(const x265hip_subpel_params\* p, const x265hip_subpel_chroma\* c, void\* stream\);", hdr)
    assert re.search(r"int x265hip_bidir_decide_chroma\(const x265hip_bidir_params\* p, const x265hip_bidir_chroma\* c, void\* stream\);", hdr)
    for name in ("x265hip_subpel_refine_chroma", "x265hip_bidir_decide_chroma"):
        assert name in A.exported_symbols() and hasattr(A.lib(), name)
    doc = hdr[hdr.index("The same refinement with the chroma SATD"):hdr.index("} x265hip_subpel_chroma;")]
    assert "subme <= 2 : c is ignored" in doc and "c == NULL" in doc            # the documented luma-only cases


def _subpel_params():
    p = A.SubpelParams()
    p.depth, p.width, p.height, p.range, p.subme = 8, 128, 64, 8, 3
    p.fenc, p.fenc_stride, p.fref, p.fref_stride = 0x10000, 320, 0x20000, 320
    p.best_in, p.cost_q, p.qoff, p.out = 0x30000, 0x40000, 40, 0x50000
    return p


def _subpel_chroma(**kw):
    c = A.SubpelChroma()
    c.fenc_cb, c.fenc_cr, c.fenc_stride_c, c.fref_cb, c.fref_cr, c.fref_stride_c = 0x60000, 0x70000, 256, 0x80000, 0x90000, 256
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_subpel_refine_chroma_validates_the_chroma_record_before_touching_a_device():
    import torch
    f = A.lib().x265hip_subpel_refine_chroma
    f.argtypes = [ctypes.POINTER(A.SubpelParams), ctypes.POINTER(A.SubpelChroma), ctypes.c_void_p]
    p = _subpel_params()
    # the parameter record itself is checked before the device too
    assert f(None, ctypes.byref(_subpel_chroma()), None) == EINVAL and f(None, None, None) == EINVAL
    for k, v in (("depth", 9), ("width", 100), ("subme", 8), ("fenc", None), ("out", None)):
        q = _subpel_params()
        setattr(q, k, v)
        assert f(ctypes.byref(q), ctypes.byref(_subpel_chroma()), None) == EINVAL, k
    for plane in ("fenc_cb", "fenc_cr", "fref_cb", "fref_cr"):
        assert f(ctypes.byref(p), ctypes.byref(_subpel_chroma(**{plane: None})), None) == EINVAL, plane
        assert b"chroma plane" in A.lib().x265hip_last_error()
    for stride in ("fenc_stride_c", "fref_stride_c"):
        for v in (0, -256):
            assert f(ctypes.byref(p), ctypes.byref(_subpel_chroma(**{stride: v})), None) == EINVAL, stride
    # the checks hold at subme <= 2 too, where the operands are then ignored
    p.subme = 2
    assert f(ctypes.byref(p), ctypes.byref(_subpel_chroma(fref_cr=None)), None) == EINVAL
    if not torch.cuda.is_available():
        for subme in (2, 3, 7):
            p.subme = subme
            assert f(ctypes.byref(p), ctypes.byref(_subpel_chroma()), None) == ENODEV
            assert f(ctypes.byref(p), None, None) == ENODEV               # c = NULL: the existing entry


def _bidir_params():
    p = A.BidirParams()
    p.depth, p.width, p.height, p.level = 8, 128, 64, 2
    p.fenc, p.fenc_stride, p.fref0, p.fref1, p.fref_stride = 0x10000, 320, 0x20000, 0x30000, 320
    p.mv0, p.mv1, p.cost_q, p.qoff = 0x40000, 0x50000, 0x60000, 56
    p.dir, p.mv0_out, p.mv1_out = 0x70000, 0x80000, 0x90000
    return p


def _bidir_chroma(**kw):
    c = A.BidirChroma()
    c.fenc_cb, c.fenc_cr, c.fenc_stride_c = 0xa0000, 0xb0000, 256
    c.fref0_cb, c.fref0_cr, c.fref1_cb, c.fref1_cr, c.fref_stride_c = 0xc0000, 0xd0000, 0xe0000, 0xf0000, 256
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_bidir_decide_chroma_validates_before_touching_a_device():
    import torch
    f = A.lib().x265hip_bidir_decide_chroma
    f.argtypes = [ctypes.POINTER(A.BidirParams), ctypes.POINTER(A.BidirChroma), ctypes.c_void_p]
    p = _bidir_params()
    assert f(None, ctypes.byref(_bidir_chroma()), None) == EINVAL
    for plane in ("fenc_cb", "fenc_cr", "fref0_cb", "fref0_cr", "fref1_cb", "fref1_cr"):
        assert f(ctypes.byref(p), ctypes.byref(_bidir_chroma(**{plane: None})), None) == EINVAL, plane
    for stride in ("fenc_stride_c", "fref_stride_c"):
        assert f(ctypes.byref(p), ctypes.byref(_bidir_chroma(**{stride: 0})), None) == EINVAL, stride
    # the luma phase planes hold rounded pixels: planes together with c are refused
    p.phase_planes0, p.phase_planes1, p.phase_plane_samples = 0x100000, 0x200000, 4096
    assert f(ctypes.byref(p), ctypes.byref(_bidir_chroma()), None) == EINVAL
    assert b"phase planes" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        assert f(ctypes.byref(p), None, None) == ENODEV                   # c = NULL: planes are legal
        p = _bidir_params()
        assert f(ctypes.byref(p), ctypes.byref(_bidir_chroma()), None) == ENODEV


def test_walk_without_chroma_is_the_oracles_refinement():
    """The Python walk is pinned to the oracle where the oracle has an answer: luma only, every subme the cases use."""
    for case in CC.CHROMA_CASES + CC.LUMA_ONLY_CASES:
        assert np.array_equal(CE.expected(case, False)["rec"], SC.refined(case)), case.id
    for case in CC.LUMA_ONLY_CASES:                                      # subme 2: bChromaSATD is off, chroma or not
        assert np.array_equal(CE.expected(case, True)["rec"], SC.refined(case)), case.id


def test_subpel_chroma_cases_reach_what_they_are_for():
    """The GPU test's inputs (tests/subpel_chroma_cases.CHROMA_CASES), printed per case.  In EVERY case the chroma walk ends at another
    vector than the luma-only walk on >= 3 % of the PUs at levels 0, 1 and 2; at level 3 (6 PUs per case) on >= 3 % pooled over the cases.
    Every interpolation arm (none, h, v, hv) takes >= 3 % of the chroma comparisons pooled over the cases: the `none` arm needs both
    components of q divisible by 8, which only a PU's first comparison can offer (the half-sample candidates sit at +-2), i.e. at most a
    quarter of the PUs once in 13 - 33 comparisons - the records are subpel_cases.build's and leave no more.  Negative vector components
    with odd q and zero-cost keys occur in every case, PUs pinned to +-R on each axis in every case and at each end over the cases."""
    diff = np.zeros(4, np.int64)
    count = np.zeros(4, np.int64)
    arms = np.zeros(4, np.int64)
    neg_odd = 0
    pinned_any = np.zeros(4, bool)
    for case in CC.CHROMA_CASES:
        cc = CC.build(*case.build)
        lum, ch = CE.expected(case, False), CE.expected(case, True)
        ql, qc = SC.unpack_q(lum["rec"]), SC.unpack_q(ch["rec"])
        moved = (ql[0] != qc[0]) | (ql[1] != qc[1])
        lv = np.array([p[1] for p in SC.pu_list(cc.w64, cc.h64)])
        per = [float(moved[lv == l].mean()) for l in range(4)]
        keys0 = (cc.luma.best >> np.uint64(32)) == 0
        pinned = [bool((cc.luma.imv[:, a] == s * cc.R).any()) for a in (0, 1) for s in (-1, 1)]            # (-R, +R) on x, then on y
        pinned_any |= np.array(pinned)
        print(f"{case.id} (tables {ch['tables']}): moved by level {np.round(per, 3).tolist()}, arms {np.round(ch['arms'] / ch['arms'].sum(), 3).tolist()}, "
              f"negative odd {ch['neg_odd']} of {ch['comparisons']}, zero keys {int(keys0.sum())}, pinned {pinned}")
        for l in range(4):
            diff[l] += moved[lv == l].sum()
            count[l] += (lv == l).sum()
        arms += ch["arms"]
        neg_odd += ch["neg_odd"]
        assert ch["neg_odd"] > 0, case.id
        assert min(per[:3]) >= 0.03, (case.id, per)            # every case carries its weight at levels 0 - 2 (level 3: 6 PUs per case, pooled below)
        assert (pinned[0] or pinned[1]) and (pinned[2] or pinned[3]), (case.id, pinned)            # each axis in every case, each end over the cases
        assert all(keys0[lv == l].any() for l in range(3)), case.id            # zero-cost keys, where the shortcut must hold with chroma too
        # the shortcut: a zero-cost key keeps its vector and returns the vector cost only
        assert np.array_equal(ch["rec"][keys0], lum["rec"][keys0])
    shares = diff / count
    arm_shares = arms / arms.sum()
    print("pooled: moved by level", np.round(shares, 3).tolist(), "arms", dict(zip(CE.ARMS, np.round(arm_shares, 3).tolist())), "negative odd", neg_odd)
    assert (shares >= 0.03).all(), shares
    assert (arm_shares >= 0.03).all(), arm_shares
    assert pinned_any.all(), pinned_any
    assert any(((cc.luma.best >> np.uint64(32)) == 0)[84::85].any() for cc in (CC.build(*c.build) for c in CC.CHROMA_CASES))      # a zero key at the top level too


@pytest.mark.parametrize("case", [CC.CHROMA_CASES[0], CC.CHROMA_CASES[3], CC.CHROMA_CASES[8]], ids=lambda c: c.id)
def test_walk_costs_equal_the_oracles_cost_tables(case):
    """Every SATD comparison the walk made, against oracle_api.cost_tables(shapes = 0, chroma = 1) with the records' integer vectors as
    the candidates - the oracle's own subpelCompare route - wherever the table's 16-bit delta is representable."""
    import cost_oracle as C
    O = C.oracle()
    cc = CC.build(*case.build)
    c = cc.luma
    rects = O.cost_pu_list(0, c.depth)
    assert len(rects) == 85
    at = {(int(x), int(y), int(w)): i for i, (x, y, w, h, _) in enumerate(rects)}
    pus = SC.pu_list(c.w64, c.h64)
    cw = c.w64 // 64
    cand = np.zeros((c.nctu, 85, 1, 2), np.int16)
    slot = np.zeros(len(pus), np.int64)
    for i, (ctu, l, z, px, py, n) in enumerate(pus):
        slot[i] = at[(px - (ctu % cw) * 64, py - (ctu // cw) * 64, n)]
        cand[ctu, slot[i], 0] = c.imv[i]
    tables = O.cost_tables(c.depth, [c.cur, cc.cur_c[0], cc.cur_c[1]], [c.ref, cc.ref_c[0], cc.ref_c[1]], c.stride, cc.stride_c, F.MARGIN_X, F.MARGIN_Y,
                           F.CHROMA_MARGIN_Y, c.w64, 0, c.h64 // 64, 0, 1, case.subme, 1, cand)
    mv, cost = C.parse_records(tables, case.subme)
    pos = {(int(p[0]), int(p[1])): k for k, p in enumerate(O.cost_positions(case.subme, c.depth))}
    dist = CE.expected(case)["dist"]
    checked = 0
    for i, (ctu, l, z, px, py, n) in enumerate(pus):
        for (qx, qy), want in dist[i].items():
            k = pos.get((qx - 4 * int(c.imv[i][0]), qy - 4 * int(c.imv[i][1])))
            assert k is not None, (i, qx, qy)
            got = int(cost[ctu, slot[i], 0, k])
            if got != 0xffffffff:
                assert got == want, (case.id, i, (qx, qy), got, want)
                checked += 1
    print(case.id, "comparisons checked against the cost tables:", checked)
    refined = int(np.count_nonzero(c.best >> np.uint64(32)))
    assert checked >= 4 * refined, (checked, refined)              # every refined PU makes >= 5 SATD comparisons; the cheapest ones are representable


@pytest.mark.parametrize("depth", [8, 10])
def test_six_stripe_b_case_meets_every_outcome_with_chroma(depth):
    """On the six-stripe B case (384 x 128, all three planes, range 12, subme 3) each of dir 1 / 2 / 3 and "the zero candidate won" lies on
    >= 3 % of the blocks at every level, and the chroma decision (`dir` itself - the vectors differ already because the records do) differs from the luma-only decision - the
    oracle's luma-only records through bidir_expect.expect - on >= 3 % of the blocks."""
    b = CC.build_b(depth)
    lrecs = CE.b_records(depth, 3, False)
    for l in (0, 1):                                                    # the luma-only walk is the oracle's chain on this case too
        assert np.array_equal(lrecs[l], BE.oracle_records(depth, b.pad[1][0], b.pad[2 * l][0], b.stride, b.org, b.w64, b.h64, b.R, 3))
    phases = [BE.phases_of(depth, b.pad[l][0], b.stride) for l in (0, 2)]
    cq, qoff = F.qpel_cost_table(b.R)
    for level in (0, 1, 2):
        e = CE.bidir_expected(depth, 3, level)
        lum = BE.expect(depth, b.pad[1][0], b.stride, b.org, b.w64, b.h64, level, lrecs, phases, cq, qoff)
        shares = {k: float(m.mean()) for k, m in e["masks"].items()}
        differs = float((lum["dir"] != e["dir"]).mean())          # the list decision itself: vectors differ already because the records do
        print(f"depth {depth} level {level} (tables {e['tables']}):", {k: round(v, 3) for k, v in shares.items()}, "dir differs from luma only", round(differs, 3))
        for k in CE.OUTCOMES:
            assert shares[k] >= 0.03, (depth, level, k, shares[k])
        assert differs >= 0.03
