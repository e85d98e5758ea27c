"""CPU-only checks of the bidirectional decision: the C entry's declaration, export, record layout and argument validation, and the
expectation helper the GPU tests compare against (tests/bidir_expect.py) - that it meets every outcome on the six-stripe picture, and
that its predictions are the real reference's."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import bidir_expect as BE
import harness
from conftest import missing_reference_build

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
spec = importlib.import_module("x265-yuuki-asuna_amd.table_spec")


def test_bidir_decide_is_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_bidir_decide\(const x265hip_bidir_params\* p, void\* stream\);", hdr)
    assert "x265hip_bidir_decide" in A.exported_symbols()
    assert hasattr(A.lib(), "x265hip_bidir_decide")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_bidir_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_bidir_params, {f}));' for f, _ in A.BidirParams._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, val = line.split()
        want = ctypes.sizeof(A.BidirParams) if name == "." else getattr(A.BidirParams, name).offset
        assert int(val) == want, f"x265hip_bidir_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(A.BidirParams._fields_) + 1 == 26


def _valid_params():
    p = A.BidirParams()
    p.depth, p.width, p.height, p.level = 8, 128, 64, 2
    p.fenc, p.fenc_stride, p.fref0, p.fref1, p.fref_stride = 0x10000, 320, 0x20000, 0x30000, 320
    p.mv0, p.mv1, p.cost_q, p.qoff = 0x40000, 0x50000, 0x60000, 56
    p.dir, p.mv0_out, p.mv1_out = 0x70000, 0x80000, 0x90000
    return p


def test_bidir_decide_validates_before_touching_a_device():
    """Every invalid-argument case returns X265HIP_EINVAL with no device call in front of it; a valid record without a device returns
    X265HIP_ENODEV (the pointers of these records are never dereferenced on the host)."""
    import torch
    f = A.lib().x265hip_bidir_decide
    f.argtypes = [ctypes.POINTER(A.BidirParams), ctypes.c_void_p]
    EINVAL, ENODEV = -2, -1
    assert f(None, None) == EINVAL

    def bad(**kw):
        p = _valid_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    assert b"level" in A.lib().x265hip_last_error()
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64)):
        assert bad(**{k: v}) == EINVAL
    for req in ("fenc", "fref0", "fref1", "mv0", "mv1", "cost_q", "dir", "mv0_out", "mv1_out"):
        assert bad(**{req: None}) == EINVAL, req
    assert bad(mv0_out=0x40000) == EINVAL and bad(mv1_out=0x50000) == EINVAL          # mv*_out aliasing mv*
    assert bad(mv0_out=0x50000) == EINVAL and bad(mv1_out=0x40000) == EINVAL
    assert bad(mv0_out=0x40000 + 8) == EINVAL                                         # overlapping, not only equal
    assert b"alias" in A.lib().x265hip_last_error()
    assert bad(phase_planes0=0xa0000) == EINVAL                                       # one list's planes only
    assert bad(phase_planes0=0xa0000, phase_planes1=0xb0000, phase_plane_samples=0) == EINVAL
    if not torch.cuda.is_available():
        for depth in (8, 10, 12):
            assert bad(depth=depth) == ENODEV
        assert bad(ref0=0xc0000, ref1=0xd0000, cost_out=0xe0000, phase_planes0=0xa0000, phase_planes1=0xb0000, phase_plane_samples=4096) == ENODEV


@pytest.mark.parametrize("subme", [2, 3])
@pytest.mark.parametrize("depth", [8, 10])
def test_six_stripe_picture_meets_every_outcome(depth, subme):
    """The condition that keeps the GPU comparison from passing on a degenerate field: on the six-stripe picture (768x192, range 12,
    lambda 4, dir_cost (12, 12, 20), seed 21) each of {dir 1, dir 2, dir 3 at the refined vectors, dir 3 at zero vectors, zero candidate
    not tried, c0 == c1} holds for at least 3 % of the blocks, at every level."""
    case = BE.SixStripe(depth, subme)
    for level in (0, 1, 2):
        e = case.expect(level)
        shares = {k: float(m.mean()) for k, m in e["masks"].items()}
        print(f"depth {depth} subme {subme} level {level} (tables {e['tables']}):", {k: round(v, 3) for k, v in shares.items()})
        for k in BE.OUTCOMES:
            assert shares[k] >= 0.03, f"depth {depth} subme {subme} level {level}: outcome {k} on {shares[k]:.3%} of the blocks"
        # the outputs' own consistency
        assert set(np.unique(e["dir"])) == {1, 2, 3}
        assert ((e["ref0"] >= 0) == ((e["dir"] & 1) != 0)).all() and ((e["ref1"] >= 0) == ((e["dir"] & 2) != 0)).all()
        assert (e["cost"][e["masks"]["not_tried"], 3] == -1).all() and (e["cost"][~e["masks"]["not_tried"], 3] >= 0).all()


@pytest.mark.parametrize("depth", [8, 10])
def test_helper_predictions_are_the_reference_filters(depth, repo_root):
    """The helper's P0 / P1 (phase-plane reads) equal the real reference table's luma_hpp / luma_vpp / luma_hvpp (copy for phase 0) on 200
    blocks - x265ref_motion_compensation is not the decision's prediction (it is addAvg of 14-bit intermediates), so the helper is
    pinned to the reference through the filters predInterLumaPixel calls."""
    ref = harness.load_reference(depth, repo_root)
    if ref is None:
        missing_reference_build()
    case = BE.SixStripe(depth, 3)
    rs = np.random.default_rng([5, depth])
    es = case.cur.itemsize
    seen_phases = set()
    for k in range(200):
        level = k % 3
        n, nb, base = 8 << level, (64 >> (3 + level)) ** 2, BE.LEVEL_BASE[level]
        idx = spec.LUMA_PU_INDEX[f"{n}x{n}"]
        ctu, z, l = int(rs.integers(case.nctu)), int(rs.integers(nb)), int(rs.integers(2))
        qx, qy = BE.unpack_mv(case.recs[l][ctu * 85 + base + z][1])
        if k % 4 == 3:                                    # the records alone leave some phases rare: walk all 16 as well
            qx, qy = (qx & ~3) | (k // 4 % 4), (qy & ~3) | (k // 16 % 4)
        bx, by = BE.zorder(z)
        cw = case.w64 // 64
        off = case.org + ((ctu // cw) * 64 + by * n + (qy >> 2)) * case.stride + (ctu % cw) * 64 + bx * n + (qx >> 2)
        xf, yf = qx & 3, qy & 3
        seen_phases.add((xf, yf))
        ph = case.phases[l]
        got = ph[yf * 4 + xf].reshape(-1)[off:off + n * case.stride].reshape(n, case.stride)[:, :n]
        src = case.refs[l].ctypes.data + off * es
        dst = np.zeros((n, n), case.cur.dtype)
        if not (xf | yf):
            dst[:] = case.refs[l].reshape(-1)[off:off + n * case.stride].reshape(n, case.stride)[:, :n]
        elif not yf:
            ref.fn(f"pu[{idx}].luma_hpp")(src, case.stride, dst.ctypes.data, n, xf)
        elif not xf:
            ref.fn(f"pu[{idx}].luma_vpp")(src, case.stride, dst.ctypes.data, n, yf)
        else:
            ref.fn(f"pu[{idx}].luma_hvpp")(src, case.stride, dst.ctypes.data, n, xf, yf)
        assert np.array_equal(got, dst), f"block {k}: level {level} ctu {ctu} z {z} list {l} mv ({qx}, {qy})"
    assert len(seen_phases) == 16
