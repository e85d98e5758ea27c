"""CPU-only checks of the P step with several references: the C entries' declarations, exports, record layouts and argument validation,
the conditions the six-stripe picture of tests/multiref_expect.py has to meet for the GPU comparison to mean something, and the resource
report of the new kernels."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import multiref_expect as ME

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

EINVAL, ENODEV = -2, -1
ENTRIES = ("x265hip_ref_select", "x265hip_inter_recon_refs", "x265hip_inter_recon_chroma_refs", "x265hip_inter_recon_chroma_pair_refs")


def test_entries_are_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_ref_select\(const x265hip_ref_select_params\* p, void\* stream\);", hdr)
    assert re.search(r"int x265hip_inter_recon_refs\(const x265hip_recon_refs_params\* p, void\* stream\);", hdr)
    assert re.search(r"int x265hip_inter_recon_chroma_refs\(const x265hip_recon_refs_params\* p, void\* stream\);", hdr)
    assert re.search(r"int x265hip_inter_recon_chroma_pair_refs\(const x265hip_recon_refs_params\* cb, const x265hip_recon_refs_params\* cr, void\* stream\);", hdr)
    assert re.search(r"#define X265HIP_MAX_REFS 8\b", hdr) and A.MAX_REFS == 8
    for name in ENTRIES:
        assert name in A.exported_symbols() and hasattr(A.lib(), name), name
    # the two entries x265hip_tu_launch_grid learns sit in an enum of their own behind x265hip_tu_entry, whose values stay
    src = tmp_path / "entries.c"
    src.write_text('#include <stdio.h>\n#include "x265hip.h"\nint main(void) { printf("%d %d %d\\n", (int)X265HIP_TU_ENTRY_INTRA, '
                   '(int)X265HIP_TU_ENTRY_INTER_REFS, (int)X265HIP_TU_ENTRY_INTER_CHROMA_REFS); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(tmp_path / "entries")], check=True)
    vals = subprocess.run([str(tmp_path / "entries")], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in vals] == [A.TU_ENTRY_INTRA, A.TU_ENTRY_INTER_REFS, A.TU_ENTRY_INTER_CHROMA_REFS] == [4, 8, 9]
    pairs = {"x265hip_ref_select_params": A.RefSelectParams, "x265hip_recon_refs_params": A.ReconRefsParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} . %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in filter(None, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")):
        cname, name, val = line.split()
        cls = pairs[cname]
        want = ctypes.sizeof(cls) if name == "." else getattr(cls, name).offset
        assert int(val) == want, f"{cname}.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(A.RefSelectParams._fields_) + len(A.ReconRefsParams._fields_) + 2 == 18


def _select_params(nrefs=4):
    p = A.RefSelectParams()
    p.depth, p.width, p.height, p.level, p.nrefs = 8, 128, 64, 2, nrefs
    for r in range(nrefs):
        p.mv[r], p.ref_cost[r], p.ref_ids[r] = 0x100000 * (r + 1), 4 * r, r
    p.ref_idx, p.mv_out = 0x10000, 0x900000
    return p


def test_ref_select_validates_before_touching_a_device():
    """Every invalid-argument case returns X265HIP_EINVAL with no device call in front of it; a valid record without a device returns
    X265HIP_ENODEV (the pointers of these records are never dereferenced on the host)."""
    import torch
    f = A.lib().x265hip_ref_select
    f.argtypes = [ctypes.POINTER(A.RefSelectParams), ctypes.c_void_p]
    assert f(None, None) == EINVAL

    def bad(nrefs=4, mv=None, **kw):
        p = _select_params(nrefs)
        for k, v in kw.items():
            setattr(p, k, v)
        for r, v in (mv or {}).items():
            p.mv[r] = v
        return f(ctypes.byref(p), None)
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    assert b"level" in A.lib().x265hip_last_error()
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64)):
        assert bad(**{k: v}) == EINVAL
    for nrefs in (0, -1, 9):
        p = _select_params(4)
        p.nrefs = nrefs
        assert f(ctypes.byref(p), None) == EINVAL
    assert b"nrefs" in A.lib().x265hip_last_error()
    assert bad(ref_idx=None) == EINVAL and bad(mv_out=None) == EINVAL
    for r in range(4):
        assert bad(mv={r: None}) == EINVAL, r
    for r in range(4):                                                            # mv_out aliasing or overlapping any input
        assert bad(mv_out=0x100000 * (r + 1)) == EINVAL and bad(mv_out=0x100000 * (r + 1) + 8) == EINVAL
        assert bad(mv_out=0x100000 * (r + 1) - 8) == EINVAL
    assert b"alias" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        for depth in (8, 10, 12):
            assert bad(depth=depth) == ENODEV
        assert bad(nrefs=1) == ENODEV and bad(nrefs=8, ref_id=0x20000, cost_out=0x30000) == ENODEV
        assert bad(nrefs=2, mv={3: None}) == ENODEV                               # entries behind nrefs are not looked at
        assert bad(mv_out=0x100000 * 2 - 2 * 64 // 64 * 85 * 8) == ENODEV         # ends where mv[1] begins: no overlap


def _recon_params(nrefs=4):
    q = A.ReconRefsParams()
    p = q.base
    p.depth, p.width, p.height, p.level, p.qp = 8, 128, 64, 2, 30
    p.fenc, p.fenc_stride, p.fref_stride, p.recon, p.recon_stride = 0x10000, 320, 320, 0x20000, 320
    p.mv, p.levels, p.num_sig, p.dist = 0x30000, 0x40000, 0x50000, 0x60000
    q.nrefs = nrefs
    for r in range(min(max(nrefs, 0), A.MAX_REFS)):
        q.fref[r] = 0x100000 * (r + 1)
    q.ref_idx = 0x70000
    return q


@pytest.mark.parametrize("entry", ENTRIES[1:])
def test_inter_recon_refs_validates_before_touching_a_device(entry):
    import torch
    f = getattr(A.lib(), entry)
    pair = entry.endswith("pair_refs")
    f.argtypes = [ctypes.POINTER(A.ReconRefsParams)] * (2 if pair else 1) + [ctypes.c_void_p]

    def call(q, q2=None):
        return f(ctypes.byref(q), ctypes.byref(q2 if q2 is not None else q), None) if pair else f(ctypes.byref(q), None)

    def bad(nrefs=4, planes=None, second=False, **kw):
        q = _recon_params(nrefs)
        for k, v in kw.items():
            setattr(q if k in ("nrefs", "ref_idx") else q.base, k, v)
        for r, v in (planes or {}).items():
            q.fref[r] = v
        return call(_recon_params(nrefs), q) if second else call(q)
    assert (f(None, None, None) if pair else f(None, None)) == EINVAL
    for second in ((False, True) if pair else (False,)):
        for depth in (0, 9, 16):
            assert bad(depth=depth, second=second) == EINVAL
        for level in (-1, 3):
            assert bad(level=level, second=second) == EINVAL
        for k, v in (("width", 100), ("height", 32), ("width", 0)):
            assert bad(second=second, **{k: v}) == EINVAL
        assert bad(qp=52, second=second) == EINVAL and bad(qp=-1, second=second) == EINVAL
        for nrefs in (0, 9):
            assert bad(nrefs=nrefs, second=second) == EINVAL
        for req in ("fenc", "recon", "mv", "levels", "num_sig", "dist", "ref_idx"):
            assert bad(second=second, **{req: None}) == EINVAL, req
        for r in range(4):
            assert bad(planes={r: None}, second=second) == EINVAL
        assert bad(tables=0x80000, second=second) == EINVAL                       # scaling lists / the denoiser are refused
        assert b"tables" in A.lib().x265hip_last_error()
    if pair:
        assert bad(level=1, second=True) == EINVAL and call(_recon_params(4), _recon_params(3)) == EINVAL     # the planes differ
    if not torch.cuda.is_available():
        for depth in (8, 10, 12):
            assert bad(depth=depth, qp=30) == ENODEV
        assert bad(fref=0x90000) == ENODEV                                        # base.fref is ignored
        assert bad(nrefs=1) == ENODEV and bad(nrefs=8, qp_map=0xa0000) == ENODEV
        assert bad(nrefs=2, planes={3: None}) == ENODEV


def test_tu_launch_grid_knows_the_new_entries():
    f = A.lib().x265hip_tu_launch_grid
    f.argtypes = [ctypes.c_int] * 6
    assert f(7, 16, 8, 0, 1, 100) == EINVAL and f(10, 16, 8, 0, 1, 100) == EINVAL
    assert f(A.TU_ENTRY_INTER_REFS, 4, 8, 0, 1, 100) == EINVAL and f(A.TU_ENTRY_INTER_CHROMA_REFS, 32, 8, 0, 1, 100) == EINVAL
    assert f(A.TU_ENTRY_INTER_REFS, 16, 8, 1, 1, 100) == EINVAL                   # no table flavour
    assert f(A.TU_ENTRY_INTER_REFS, 16, 8, 0, 2, 100) == EINVAL and f(A.TU_ENTRY_INTER_CHROMA_REFS, 16, 8, 0, 3, 100) == EINVAL
    import torch
    if not torch.cuda.is_available():
        assert f(A.TU_ENTRY_INTER_REFS, 32, 10, 0, 1, 100) == ENODEV and f(A.TU_ENTRY_INTER_CHROMA_REFS, 16, 8, 0, 2, 100) == ENODEV


def test_ref_cost_is_the_reference_index_code():
    """lambda x (1 + 1 + r + (r < nrefs - 1)): the truncated unary code of the index (getTUBits, search.h:246-249)"""
    assert A.ref_cost_bits(1) == (8,) == ME.ref_cost_bits(1)
    assert A.ref_cost_bits(4) == (12, 16, 20, 20) == ME.COST_DEFAULT
    assert A.ref_cost_bits(2) == (12, 12) and A.ref_cost_bits(5) == (12, 16, 20, 24, 24)


@pytest.mark.parametrize("subme", [2, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_six_stripe_picture_meets_every_condition(depth, subme):
    """The conditions that keep the GPU comparison from passing on a degenerate field, each on at least 3 % of the blocks at every level:
    every reference wins with the default ref_cost; ties - also ties the first reference takes no part in - with equal ref_cost; and the
    bias decides (the smallest raw record cost is not the winner's) with the reversed vector."""
    case = ME.five_ref(depth, subme)
    for level in (0, 1, 2):
        what = f"depth {depth} subme {subme} level {level}"
        e = case.expect(level, ME.COST_DEFAULT)
        shares = {k: float(e["masks"][k].mean()) for k in ("ref0", "ref1", "ref2", "ref3")}
        flat, rev = case.expect(level, ME.COST_FLAT), case.expect(level, ME.COST_REVERSED)
        shares.update({k: float(flat["masks"][k].mean()) for k in ("tie", "tie_not_ref0")})
        shares["bias_decides"] = float(rev["masks"]["bias_decides"].mean())
        print(what, {k: round(v, 3) for k, v in shares.items()}, "bias_decides with the default vector", round(float(e["masks"]["bias_decides"].mean()), 4))
        for k in ME.MASKS:
            assert shares[k] >= 0.03, f"{what}: {k} on {shares[k]:.3%} of the blocks"
        # the outputs' own consistency
        rows = np.arange(len(e["ref_idx"]))
        assert (e["cost"][rows, e["ref_idx"]] == e["cost"].min(axis=1)).all() and (e["mv_out"][:, 0] == e["cost"].min(axis=1)).all()
        assert (flat["ref_idx"][flat["masks"]["tie"] & ~flat["masks"]["tie_not_ref0"]] == 0).all()
        # the four planes twice: the first copy wins
        e8 = case.expect(level, ME.COST_FLAT + ME.COST_FLAT, nrefs=8)
        assert np.array_equal(e8["ref_idx"], flat["ref_idx"]) and np.array_equal(e8["mv_out"], flat["mv_out"])


def _kernels():
    from test_kernel_regs import _kernels as read
    return read()


REFS_INSTANCES = [f"inter_recon_kernel<{px}, {n}, {c}, false, TuRefsArgs>" for px in ("unsigned char", "unsigned short") for n, c in ((16, "false"), (32, "false"), (16, "true"))]


@pytest.mark.parametrize("name", REFS_INSTANCES)
def test_new_tu_kernels_keep_two_waves_without_spills_or_scratch(name):
    """The resource report of the new 16 / 32-point instances, read from the built library: two wavefronts per SIMD or more, nothing
    spilled, no scratch - what their single-reference twins were tuned for.  (The 10-bit 32-point instance gets there by building its
    MFMA operands per block: kept over the whole walk, as in its twin, 30 registers were spilled - DESIGN.md section 14.)"""
    k = _kernels()
    assert name in k, name
    assert min(8, 512 // k[name]["vgpr"]) >= 2 and k[name]["vspill"] == 0 and k[name]["scratch"] == 0, (name, k[name])


def test_ref_select_kernel_has_no_scratch():
    k = _kernels()
    assert k["ref_select_kernel"]["scratch"] == 0 and k["ref_select_kernel"]["vspill"] == 0, k["ref_select_kernel"]
