"""CPU-only checks of the sa8d choice of a B picture's blocks (x265hip_b_sa8d_decide) and of stages.Sa8dBFramePipeline: declaration,
export, record layout and argument validation of the entry, the bit helper, and the expectation the GPU tests compare against
(tests/bsa8d_expect.py): what the pictures of tests/bsa8d_cases.py reach, its tie rules, and that five mutations of it - what a wrong
kernel would compute - change listed cases."""
import ctypes
import importlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bsa8d_cases as C
import bsa8d_expect as BX
import intra_inter_expect as IX

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
EINVAL, ENODEV = -2, -1
FLOOR = 0.03          # the share of the blocks every outcome must reach: the floor of tests/test_intra_inter_cpu.py and test_bref_cpu.py


def test_the_entry_is_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_b_sa8d_decide\(const x265hip_b_sa8d_params\* p, void\* stream\);", hdr)
    assert "x265hip_b_sa8d_decide" in A.exported_symbols() and hasattr(A.lib(), "x265hip_b_sa8d_decide")
    assert callable(A.b_sa8d_decide) and callable(A.b_sa8d_bits)
    rec = A.BSa8dParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_b_sa8d_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_b_sa8d_params, {f}));' for f, _ in rec._fields_]
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
        assert int(val) == want, f"x265hip_b_sa8d_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(rec._fields_) + 1 == 29


def test_the_bit_helper_restates_the_reference():
    """base_bits = m_listSelBits[l] + MVP_IDX_BITS + getTUBits, bi_bits_delta = listSel[2] - listSel[0] - listSel[1]."""
    assert A.b_sa8d_bits() == (BX.BASE_BITS, BX.BI_BITS_DELTA) == ((4, 4), -1)
    assert A.b_sa8d_bits(nrefs=(2, 1), refs=(1, 0)) == ((5, 4), -1) and A.b_sa8d_bits(nrefs=(4, 4), refs=(1, 3)) == ((6, 7), -1)
    assert A.b_sa8d_bits(list_sel_bits=(1, 2, 6)) == ((2, 3), 3)
    # the list-selection part of base_bits is what dir_cost carries at lambda 4, the rest is b_ref_cost_bits'
    assert tuple(4 * b for b in A.b_sa8d_bits()[0]) == tuple(d + A.b_ref_cost_bits(1)[0] for d in BX.DIR_COST[:2])


def test_the_python_layers_exist():
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    assert issubclass(S.Sa8dBFramePipeline, S._RefListStep) and hasattr(S.Sa8dBFramePipeline, "set_qp_maps")
    assert "b_intra" in inspect.signature(S.Sa8dBFramePipeline.__init__).parameters
    assert "intra" in inspect.signature(S.Deblock.run_b).parameters
    for k in ("base_bits", "lambda8", "rng", "dir_cost", "ref_ids"):
        assert k in inspect.signature(S.BSa8dDecide.__init__).parameters, k


def _params():
    p = A.BSa8dParams()
    p.depth, p.width, p.height, p.level, p.qp, p.lambda8 = 8, 128, 64, 2, 30, 1024
    p.base_bits[0], p.base_bits[1], p.bi_bits_delta = 4, 4, -1
    p.dir_cost[0], p.dir_cost[1], p.dir_cost[2] = 12, 12, 20
    p.ref_id0, p.ref_id1 = 0, 1
    p.fenc, p.fenc_stride, p.fref0, p.fref1, p.fref_stride = 0x10000, 320, 0x20000, 0x30000, 320
    p.mv0, p.mv1, p.bit_sizes, p.bit_sizes_len = 0x40000, 0x50000, 0x60000, 232
    p.dir, p.ref0, p.ref1, p.mv0_out, p.mv1_out, p.cost = 0x70000, 0x71000, 0x72000, 0x80000, 0x90000, 0xa0000
    return p


def test_b_sa8d_decide_validates_before_touching_a_device():
    import torch
    f = A.lib().x265hip_b_sa8d_decide
    f.argtypes = [ctypes.POINTER(A.BSa8dParams), ctypes.c_void_p]
    assert f(None, None) == EINVAL

    def bad(**kw):
        p = _params()
        for k, v in kw.items():
            if k[:-1] in ("base_bits", "dir_cost"):
                getattr(p, k[:-1])[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for req in ("fenc", "fref0", "fref1", "mv0", "mv1", "bit_sizes", "dir", "mv0_out", "mv1_out", "cost"):
        assert bad(**{req: None}) == EINVAL, req
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    assert b"level" in A.lib().x265hip_last_error()
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64), ("fenc_stride", 127), ("fref_stride", 64)):
        assert bad(**{k: v}) == EINVAL, k
    for k, v in (("base_bits0", -1), ("base_bits1", 4097), ("bi_bits_delta", -4097), ("bi_bits_delta", 4097), ("bi_bits_delta", -9), ("lambda8", -1),
                 ("lambda8", (1 << 24) + 1), ("bit_sizes_len", 0), ("qp", 52), ("qp", -1)):
        assert bad(**{k: v}) == EINVAL, (k, v)
    assert bad(base_bits1=5000) == EINVAL and b"base_bits" in A.lib().x265hip_last_error()
    # the outputs must be buffers of their own: 2 CTUs x 85 records x 8 bytes each
    span = 2 * 85 * 8
    for kw in (dict(mv0_out=0x40000), dict(mv1_out=0x50000 + span - 8), dict(mv0_out=0x50000), dict(mv1_out=0x80000 + 8), dict(mv0_out=0x40000 - span + 8)):
        assert bad(**kw) == EINVAL, kw
    assert b"alias" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        assert bad() == ENODEV and bad(ref0=None, ref1=None, base_bits0=4096, base_bits1=0, bi_bits_delta=-4096, lambda8=1 << 24, depth=12, qp=75, level=0) == ENODEV
        assert bad(mv1_out=0x80000 + span) == ENODEV


@pytest.mark.parametrize("level", [0, 1, 2])
def test_the_pictures_reach_every_outcome(level):
    """With the expectation alone, at 8 bits, on the searched records of the 192x128 pictures: each outcome of the decision, a dir that
    differs from x265hip_bidir_decide's for the same records, and - with b_intra - intra over a single list, intra over a bidirectional
    block, inter kept and an intra block beside a bidirectional one each occur on >= 3 % of the blocks."""
    c = C._case(8, level)
    e = C.kernel_expectation(c)["e"]
    share = {k: float(v.mean()) for k, v in e["masks"].items()}
    share["differs_from_bidir_decide"] = float((C.bidir_decision(c)["dir"] != e["dir"]).mean())
    share.update({k: float(v.mean()) for k, v in C.intra_expectation(level)["masks"].items()})
    print(level, {k: round(v, 3) for k, v in share.items()})
    assert set(share) == set(BX.OUTCOMES) | {"differs_from_bidir_decide"} | set(BX.INTRA_MASKS)
    for k, v in share.items():
        assert v >= FLOOR, (level, k, v)
    assert np.array_equal(e["masks"]["list0_kept"] | e["masks"]["list1_kept"], e["dir"] != 3)


def test_outputs_follow_bidir_decides_conventions():
    """-1 for an unused list, zero vectors where the zero pair won, the unused list's record = {its own c_l, 0}, word 0 of cost = the
    smaller of the two candidates."""
    for c in (C._case(8, 1), C._case(8, 2, "far")):
        x = C.kernel_expectation(c)
        e = x["e"]
        d, cost = e["dir"], e["cost"].astype(np.int64)
        assert np.array_equal(e["ref0"], np.where(d & 1, 0, -1)) and np.array_equal(e["ref1"], np.where(d & 2, 1, -1))
        assert np.array_equal(cost[:, 0], np.minimum(cost[:, 1], cost[:, 2])) and np.array_equal(d == 3, cost[:, 2] < cost[:, 1])
        zero = (cost[:, 3] & BX.FLAG_ZERO_WON) != 0
        assert zero.any() and not (zero & ((cost[:, 3] & BX.FLAG_ZERO_TRIED) == 0)).any()
        both = zero & (d == 3)
        assert (e["mv0"][both, 1] == 0).all() and (e["mv1"][both, 1] == 0).all()
        nb, base = 64 >> (2 * c.level), (0, 64, 80)[c.level]
        rec = [r.reshape(x["nctu"], 85, 2)[:, base:base + nb].reshape(-1, 2) for r in x["recs"]]
        only0 = d == 1
        assert np.array_equal(e["mv1"][only0], np.stack([rec[1][only0, 0] + BX.DIR_COST[1], np.zeros(only0.sum(), np.int32)], axis=1))
        assert np.array_equal(e["mv0"][only0, 1], rec[0][only0, 1]) and np.array_equal(e["mv0"][only0, 0], e["cost"][only0, 1])


@pytest.mark.parametrize("c", C.TIE_CASES, ids=lambda c: c.id)
def test_ties_stay_single_list_and_keep_list_0(c):
    """ref1 is the same picture as ref0, the vectors are equal and lambda8 is 0: addAvg of two equal 14-bit intermediates rounds to the
    rounded pixel, so bi == uni exactly and every block stays single-list (the zero pair may still be cheaper: then it wins); the
    records' costs are equal, so list 0 is kept."""
    x = C.kernel_expectation(c)
    e = x["e"]
    assert np.array_equal(x["recs"][0], x["recs"][1])
    cost, sa = e["cost"].astype(np.int64), e["sa8d"]
    assert np.array_equal(sa[:, 0], sa[:, 1]) and np.array_equal(sa[:, 0], sa[:, 2]) and np.array_equal(cost[:, 1], sa[:, 0])
    searched = (cost[:, 3] & BX.FLAG_ZERO_WON) == 0
    assert searched.mean() >= FLOOR and(e["dir"][searched] == 1).all() and (cost[searched, 2] == cost[searched, 1]).all()
    assert ((cost[:, 3] & BX.FLAG_LIST1) == 0).all() and not (e["dir"] == 2).any()


def test_equal_record_costs_keep_list_0():
    """far_records gives every seventh block c0 == c1 with different vectors: list 0 is the single list there, whatever the sa8d says."""
    c = C._case(8, 0, "far")
    x = C.kernel_expectation(c)
    nb = 64
    rec = [r.reshape(x["nctu"], 85, 2)[:, :nb].reshape(-1, 2) for r in x["recs"]]
    tie = rec[0][:, 0] == rec[1][:, 0]
    e = x["e"]
    assert tie.mean() >= 0.1 and ((e["cost"][tie, 3] & BX.FLAG_LIST1) == 0).all()
    assert (e["sa8d"][tie, 1] < e["sa8d"][tie, 0]).any()                # list 1 would have been cheaper by sa8d on some of them
    assert ((e["cost"][~tie, 3] & BX.FLAG_LIST1) != 0).any()


@pytest.mark.parametrize("level", [0, 1, 2])
def test_intra_ties_stay_inter(level):
    """The walk against supplied inter costs of intra cost - 1 / + 0 / + 1 by block index modulo 3 (intra_inter_expect.tie_pattern): a tie
    stays inter - the rule word 0 of `cost` is decided by."""
    w = C.intra_expectation(level, ties=True)["walk"]
    b = np.arange(len(w["intra"]))
    assert np.array_equal(w["intra"], (b % 3 == 2).astype(np.uint8)) and w["masks"]["tie_stays_inter"].mean() > 0.3


def test_the_reference_build_agrees_where_it_is_present():
    c = C._case(8, 1)
    e = C.run_decide(c, with_reference=True)
    assert e["tables"] in (1, 2)
    for k in ("dir", "cost", "mv0", "mv1", "sa8d"):
        assert np.array_equal(e[k], C.kernel_expectation(c)["e"][k]), k


def test_mutations_of_the_expectation_change_listed_cases():
    """Each mutation - what a kernel with that mistake would compute - changes a counted, non-zero number of the 8-bit kernel cases; the
    counts are recorded in DESIGN.md section 18."""
    cases = [c for c in C.KERNEL_CASES if c.depth == 8]
    counts = {}
    for mut in BX.MUTATIONS:
        hit = []
        for c in cases:
            want, got = C.kernel_expectation(c)["e"], C.run_decide(c, mutation=mut)
            if any(not np.array_equal(want[k], got[k]) for k in ("dir", "mv0", "mv1", "cost")):
                hit.append(c.id)
        counts[mut] = len(hit)
        print(mut, len(hit), "of", len(cases), hit)
        assert hit, mut
    # `<=` in the choice shows exactly where bi == uni: the same-reference tie cases
    assert counts["le_in_choice"] >= len(C.TIE_CASES)
