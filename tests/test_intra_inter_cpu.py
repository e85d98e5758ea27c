"""CPU-only checks of the intra-in-inter stages of a P picture (x265hip_inter_sa8d_cost, x265hip_intra_in_inter): declaration, export,
record layout and argument validation of the two entries, the bit-size table, and the expectation the GPU tests compare against
(tests/intra_inter_expect.py): its limits (an inter cost nothing beats = the I walk with the P slice's flags; an inter cost of 0 =
the inter coding untouched), what the pictures of tests/intra_inter_cases.py reach, and that four mutations of the walk - what a wrong
kernel would compute - change the expectation of listed cases."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import bidir_expect as BE
import intra_expect as IE
import intra_inter_cases as C
import intra_inter_expect as IX

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
F = importlib.import_module("x265-yuuki-asuna_amd.frames")
EINVAL, ENODEV = -2, -1
KEYS = ("mode", "intra", "levels", "num_sig", "dist", "recon", "levels_c0", "num_sig_c0", "dist_c0", "recon_c0", "levels_c1", "num_sig_c1", "dist_c1", "recon_c1")


def test_the_entries_are_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_inter_sa8d_cost\(const x265hip_inter_sa8d_cost_params\* p, void\* stream\);", hdr)
    assert re.search(r"int x265hip_intra_in_inter\(const x265hip_intra_picture_params\* p, const int32_t\* inter_cost, intptr_t inter_cost_stride, uint8_t\* intra,", hdr)
    for name in ("x265hip_inter_sa8d_cost", "x265hip_intra_in_inter"):
        assert name in A.exported_symbols() and hasattr(A.lib(), name)
    assert callable(A.inter_sa8d_cost) and callable(A.intra_in_inter) and callable(A.mv_bit_sizes)
    rec = A.InterSa8dCostParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_inter_sa8d_cost_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_inter_sa8d_cost_params, {f}));' for f, _ in rec._fields_]
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
        assert int(val) == want, f"x265hip_inter_sa8d_cost_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(rec._fields_) + 1 == 18


def test_bit_size_table_is_the_reference_formula_and_prices_like_the_search():
    """hipabi.mv_bit_sizes = the statements of bitcost.cpp:105-108, and rounds to the uint16 costs frames.mv_cost_table gives the search."""
    t = A.mv_bit_sizes(4 * 64 + 4)
    assert t.dtype == np.float32 and np.array_equal(t, IX.s_bitsizes(len(t))) and t[0] == np.float32(0.718)
    d = np.abs(np.arange(-64, 65)) * 4
    for lam in (1.0, 4.0, 7.25):
        assert np.array_equal(np.minimum(t[d] * np.float32(lam) + np.float32(0.5), np.float32(32767.0)).astype(np.uint16), F.mv_cost_table(64, lam))
    assert A.ref_cost_bits(1, lam=1)[0] == IX.BASE_BITS
    assert IX.mv_bits(IX.pack_mv(-5, 8), t) == int(t[5] + t[8] + np.float32(0.5)) and IX.mv_bits(IX.pack_mv(0, 0), t) == 1
    assert IX.mv_bits(IX.pack_mv(-300, 4), t[:100]) == int(t[99] + t[4] + np.float32(0.5))         # beyond the table: its last entry


def _cost_params():
    p = A.InterSa8dCostParams()
    p.depth, p.width, p.height, p.level, p.qp, p.base_bits, p.lambda8 = 8, 128, 64, 2, 30, 2, 1024
    p.fenc, p.fenc_stride, p.fref, p.fref_stride = 0x10000, 320, 0x20000, 320
    p.mv, p.bit_sizes, p.bit_sizes_len, p.cost = 0x30000, 0x40000, 232, 0x50000
    return p


def test_inter_sa8d_cost_validates_before_touching_a_device():
    import torch
    f = A.lib().x265hip_inter_sa8d_cost
    f.argtypes = [ctypes.POINTER(A.InterSa8dCostParams), ctypes.c_void_p]
    assert f(None, None) == EINVAL

    def bad(**kw):
        p = _cost_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for req in ("fenc", "fref", "mv", "bit_sizes", "cost"):
        assert bad(**{req: None}) == EINVAL, req
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    assert b"level" in A.lib().x265hip_last_error()
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64), ("fenc_stride", 127), ("fref_stride", 64)):
        assert bad(**{k: v}) == EINVAL, k
    for k, v in (("base_bits", -1), ("base_bits", 4097), ("lambda8", -1), ("lambda8", (1 << 24) + 1), ("bit_sizes_len", 0), ("qp", 52), ("qp", -1)):
        assert bad(**{k: v}) == EINVAL, (k, v)
    assert bad(base_bits=5000) == EINVAL and b"base_bits" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        assert bad() == ENODEV and bad(base_bits=4096, lambda8=1 << 24, depth=12, qp=75, level=0) == ENODEV


def test_intra_in_inter_validates_before_touching_a_device():
    """The I entry's refusals, plus NULL inter_cost / intra, a stride below 1 and X265HIP_TU_INTRA_SLICE in the flags of a P slice."""
    import torch
    from test_ipicture_cpu import _valid_params
    f = A.lib().x265hip_intra_in_inter
    f.argtypes = [ctypes.POINTER(A.IntraPictureParams), ctypes.c_void_p, ctypes.c_ssize_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert f(None, 0x200000, 2, 0x210000, None, None, None) == EINVAL

    def bad(chroma=True, inter_cost=0x200000, stride=2, intra=0x210000, **kw):
        p = _valid_params(chroma)
        p.flags = 2
        for k, v in kw.items():
            if k.startswith("mode_bits"):
                p.mode_bits[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return f(ctypes.byref(p), inter_cost, stride, intra, None, None, None)
    assert bad(inter_cost=None) == EINVAL and bad(intra=None) == EINVAL and bad(stride=0) == EINVAL and bad(stride=-2) == EINVAL
    for flags in (1, 3):
        assert bad(flags=flags) == EINVAL
    assert b"INTRA_SLICE" in A.lib().x265hip_last_error()
    for kw in (dict(depth=9), dict(level=3), dict(level=-1), dict(width=100), dict(height=0), dict(qp=52), dict(qp_cb=-1), dict(lambda8=(1 << 24) + 1),
               dict(mode_bits1=4097), dict(fenc=None), dict(recon=None), dict(mode=None), dict(levels=None), dict(num_sig=None), dict(dist=None),
               dict(recon_cr=None), dict(levels_cb=None), dict(recon=0x10000), dict(recon_cr=0x90000), dict(flags=4), dict(fenc_stride=127),
               dict(recon_stride_c=0), dict(tables=0x110000)):
        assert bad(**kw) == EINVAL, kw
    if not torch.cuda.is_available():
        assert bad() == ENODEV and bad(chroma=False, flags=0, stride=1) == ENODEV


COVER = [c for c in C.MID_CASES + C.TIE_CASES if c.depth == 8 and c.flags]


@pytest.mark.parametrize("level", [0, 1, 2])
def test_the_pictures_reach_every_outcome(level):
    """With the walk alone, at 8 bits: `split` and `swapped` at the mid point each have intra and inter winners on >= 20 % of their blocks, and
    over those two and their supplied-cost tie patterns every mask is reached on >= 3 % of the blocks (a natural tie is rare: the tie mask
    comes from the patterns, where a third of the blocks tie)."""
    cases = [c for c in COVER if c.level == level]
    assert len(cases) == 4
    share = {k: 0.0 for k in IX.MASKS}
    for c in cases:
        m = C.expectation(c)["e"]["masks"]
        print(c.id, {k: round(float(v.mean()), 3) for k, v in m.items()})
        if not c.ties:
            assert m["intra_won"].mean() >= 0.2 and m["inter_won"].mean() >= 0.2, c.id
        for k in IX.MASKS:
            share[k] += float(m[k].mean()) / len(cases)
    print(level, {k: round(v, 3) for k, v in share.items()})
    for k, v in share.items():
        assert v >= 0.03, (level, k, v)


def test_whole_pictures_go_one_way():
    for c in C.WHOLE_CASES:
        m = C.expectation(c)["e"]["masks"]
        assert (m["intra_won"] if c.kind == "all_new" else m["inter_won"]).mean() >= 0.9, c.id


@pytest.mark.parametrize("c", [C.MID_CASES[2], C.MID_CASES[9]], ids=lambda c: c.id)
def test_limits_of_the_walk(c):
    """inter_cost = INT32_MAX everywhere: every block is intra, and the walk is intra_expect.expect with the P slice's flags (whatever the
    recon planes held).  inter_cost = 0 everywhere: nothing of the inter coding changes."""
    x = C.inter_expectation(c)
    n = len(x["inter"]["inter_cost"])
    hi = C.run_walk(c, inter_cost=np.full(n, 0x7fffffff, np.int64))
    i_pic = IE.expect(c.depth, x["pcur"], x["w64"], x["h64"], c.level, x["qp"], qp_c=x["qp_c"], flags=c.flags, lambda8=x["lambda8"], mode_bits=x["mode_bits"],
                      with_reference=False, recon_init=[x["inter"]["recon" + s] for s in ("", "_c0", "_c1")])
    assert hi["intra"].all()
    bad = BE.compare({k: hi[k] for k in KEYS if k != "intra"}, {k: i_pic[k] for k in KEYS if k != "intra"})
    assert not bad, bad
    assert np.array_equal(hi["cost"], i_pic["cost"])
    lo = C.run_walk(c, inter_cost=np.zeros(n, np.int64))
    assert not lo["intra"].any() and (lo["mode"] == 1).all()
    for k in KEYS[2:]:
        assert np.array_equal(lo[k], x["inter"][k]), k


def test_the_reference_build_reproduces_the_winners():
    """Where oracle/_ref is built, its slots are called beside the oracle's and x265ref_pred_intra must reproduce every intra winner's
    prediction (the walk asserts it block by block); without the build the walk is the oracle's alone."""
    c = C.MID_CASES[2]
    e = C.run_walk(c, with_reference=True)
    assert e["tables"] in (1, 2)
    bad = BE.compare({k: e[k] for k in KEYS}, {k: C.expectation(c)["e"][k] for k in KEYS})
    assert not bad, bad


def test_mutations_of_the_walk_change_listed_cases():
    """Each mutation - what a kernel with that mistake would compute - changes the expectation of at least one case; the counts are
    recorded in DESIGN.md section 17."""
    cases = [c for c in C.ALL_CASES if c.depth == 8 and c.chroma]
    counts = {}
    for mut in IX.MUTATIONS:
        hit = []
        for c in cases:
            want, got = C.expectation(c)["e"], C.run_walk(c, mutation=mut)
            if any(not np.array_equal(want[k], got[k]) for k in KEYS):
                hit.append(c.id)
        counts[mut] = len(hit)
        print(mut, len(hit), "of", len(cases), hit)
        assert hit, mut
    # `<=` in the choice shows exactly where costs tie: the supplied-cost patterns
    ties = [c for c in cases if c.ties]
    assert counts["le_in_choice"] >= len(ties)
