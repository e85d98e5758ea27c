"""CPU-only checks of the I-picture stage: the C entries' declaration, export, record layout and argument validation, the wave
arithmetic, the schedule (every block a block reads from runs earlier), hand-made cases of the reference-sample fill, and that the
expectation the GPU tests compare against (tests/intra_expect.py) meets every outcome on the test picture."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import intra_expect as IE

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")


def test_intra_picture_is_declared_exported_and_laid_out_like_the_header(repo_root, tmp_path):
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_intra_picture\(const x265hip_intra_picture_params\* p, void\* stream\);", hdr)
    assert re.search(r"int x265hip_intra_picture_waves\(int width, int height\);", hdr)
    for name in ("x265hip_intra_picture", "x265hip_intra_picture_waves"):
        assert name in A.exported_symbols() and hasattr(A.lib(), name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {',
             '  printf(". %zu\\n", sizeof(x265hip_intra_picture_params));']
    lines += [f'  printf("{f} %zu\\n", offsetof(x265hip_intra_picture_params, {f}));' for f, _ in A.IntraPictureParams._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for line in filter(None, out):
        name, val = line.split()
        want = ctypes.sizeof(A.IntraPictureParams) if name == "." else getattr(A.IntraPictureParams, name).offset
        assert int(val) == want, f"x265hip_intra_picture_params.{name}: C says {val}, ctypes says {want}"
        seen += 1
    assert seen == len(A.IntraPictureParams._fields_) + 1 == 34


def _valid_params(chroma=True):
    p = A.IntraPictureParams()
    p.depth, p.width, p.height, p.level, p.qp, p.qp_cb, p.qp_cr, p.flags = 8, 128, 64, 2, 30, 29, 29, 3
    p.strong_intra_smoothing, p.lambda8 = 1, 1024
    p.mode_bits[0], p.mode_bits[1], p.mode_bits[2] = 2, 3, 6
    p.fenc, p.fenc_stride, p.recon, p.recon_stride = 0x10000, 320, 0x20000, 320
    p.mode, p.levels, p.num_sig, p.dist = 0x30000, 0x40000, 0x50000, 0x60000
    if chroma:
        p.fenc_cb, p.fenc_cr, p.fenc_stride_c, p.recon_cb, p.recon_cr, p.recon_stride_c = 0x70000, 0x80000, 256, 0x90000, 0xa0000, 256
        p.levels_cb, p.num_sig_cb, p.dist_cb, p.levels_cr, p.num_sig_cr, p.dist_cr = 0xb0000, 0xc0000, 0xd0000, 0xe0000, 0xf0000, 0x100000
    return p


def test_intra_picture_validates_before_touching_a_device():
    """Every invalid-argument case returns X265HIP_EINVAL with no device call in front of it; a valid record without a device returns
    X265HIP_ENODEV (the pointers of these records are never dereferenced on the host).  `tables` is refused: the stage does not support
    scaling lists or the denoiser."""
    import torch
    f = A.lib().x265hip_intra_picture
    f.argtypes = [ctypes.POINTER(A.IntraPictureParams), ctypes.c_void_p]
    EINVAL, ENODEV = -2, -1
    assert f(None, None) == EINVAL

    def bad(chroma=True, **kw):
        p = _valid_params(chroma)
        for k, v in kw.items():
            if k.startswith("mode_bits"):
                p.mode_bits[int(k[-1])] = v
            else:
                setattr(p, k, v)
        return f(ctypes.byref(p), None)
    for depth in (0, 9, 11, 16):
        assert bad(depth=depth) == EINVAL
    for level in (-1, 3):
        assert bad(level=level) == EINVAL
    assert b"level" in A.lib().x265hip_last_error()
    for k, v in (("width", 100), ("height", 32), ("width", 0), ("height", -64)):
        assert bad(**{k: v}) == EINVAL
    for k, v in (("qp", -1), ("qp", 52), ("qp_cb", 52), ("qp_cr", -1), ("lambda8", -1), ("mode_bits0", -1), ("mode_bits2", 5000)):
        assert bad(**{k: v}) == EINVAL, k
    for req in ("fenc", "recon", "mode", "levels", "num_sig", "dist"):
        assert bad(**{req: None}) == EINVAL, req
    for req in ("fenc_cb", "fenc_cr", "recon_cb", "recon_cr", "levels_cb", "num_sig_cb", "dist_cb", "levels_cr", "num_sig_cr", "dist_cr"):
        assert bad(**{req: None}) == EINVAL, req            # chroma: all or none
    assert bad(recon=0x10000) == EINVAL and bad(recon_cb=0x70000) == EINVAL             # recon aliasing the source
    assert bad(recon_cr=0x90000) == EINVAL                                              # ... or Cb's reconstruction
    assert b"alias" in A.lib().x265hip_last_error()
    # the winning cost must fit the int32 of `cost`: lambda8 is bounded by 2^24 (mode_bits by 4096)
    assert bad(lambda8=(1 << 24) + 1) == EINVAL and bad(lambda8=0x7fffffff) == EINVAL
    assert b"lambda8" in A.lib().x265hip_last_error()
    assert bad(flags=4) == EINVAL and bad(flags=1 << 30) == EINVAL                      # unknown flag bits
    for k, v in (("fenc_stride", 127), ("recon_stride", 64), ("fenc_stride_c", 63), ("recon_stride_c", 0)):
        assert bad(**{k: v}) == EINVAL, k
    assert b"stride" in A.lib().x265hip_last_error()
    assert bad(tables=0x110000) == EINVAL
    assert b"tables" in A.lib().x265hip_last_error()
    if not torch.cuda.is_available():
        for depth, qp in ((8, 51), (10, 63), (12, 75)):
            assert bad(depth=depth, qp=qp) == ENODEV
        assert bad(chroma=False) == ENODEV and bad(cost=0x120000, strong_intra_smoothing=0) == ENODEV
        assert bad(lambda8=1 << 24, mode_bits2=4096, fenc_stride=128, recon_stride=128, fenc_stride_c=64, recon_stride_c=64, flags=0) == ENODEV


def test_waves_is_the_formula_and_needs_no_device():
    for w in range(64, 64 * 9, 64):
        for h in range(64, 64 * 7, 64):
            assert A.intra_picture_waves(w, h) == w // 64 + 2 * (h // 64 - 1) == IE.waves(w, h)
    assert A.intra_picture_waves(3840, 2176) == 126
    f = A.lib().x265hip_intra_picture_waves
    for w, h in ((0, 64), (64, 0), (100, 64), (64, 65), (-64, 64)):
        assert f(w, h) == -2


@pytest.mark.parametrize("w64,h64", [(256, 192), (64, 192), (256, 64)])
def test_every_block_a_block_reads_runs_earlier(w64, h64):
    """The schedule, in pure Python: CTU (cx, cy) runs in wave cx + 2 cy.  For every block of every level, every block whose
    reconstruction the walk reads lies in a CTU of an EARLIER wave, or in the same CTU with a smaller z; every CTU has exactly one wave
    below x265hip_intra_picture_waves, and no wave is empty unless the picture is one CTU wide (odd waves have no CTU then)."""
    cw = w64 // 64
    wave = lambda ctu: ctu % cw + 2 * (ctu // cw)
    nwaves = IE.waves(w64, h64)
    assert sorted({wave(c) for c in range(cw * (h64 // 64))}) == list(range(0, nwaves, 2 if cw == 1 else 1))
    reads = 0
    for level in (0, 1, 2):
        n = 8 << level
        for gy in range(0, h64, n):
            for gx in range(0, w64, n):
                ctu, z = IE.coding_position(gx, gy, n, w64)
                for rc, rz in IE.reads_of_block(gx, gy, n, w64, h64):
                    assert (rc == ctu and rz < z) or wave(rc) < wave(ctu), (level, gx, gy, rc, rz)
                    reads += 1
    assert reads > 0 or (w64, h64) == (64, 64)


def _plane(depth=8, w=64, h=64, seed=3):
    r = np.random.default_rng(seed)
    stride = w + 64
    p = r.integers(0, 1 << depth, size=(h + 64, stride)).astype(np.uint8 if depth == 8 else np.uint16)
    return p.reshape(-1), stride, 32 * stride + 32            # flat plane, stride, element of sample (0, 0)


def test_fill_hand_made_cases():
    """Predict::fillReferenceSamples on hand-made availability: nothing, everything, top row of the picture, left column, above-right
    unavailable, below-left available, a leading unavailable run - against values read off the plane by hand."""
    n, unit, depth = 8, 4, 8
    pl, stride, org = _plane()
    off = org + 16 * stride + 16
    at = lambda x, y: int(pl[off + y * stride + x])
    units = n // unit
    lu = 2 * units
    total = 2 * lu + 1

    def fill(flags):
        return IE.fill_reference_samples(pl, off, stride, flags, n, unit, depth).astype(np.int64)
    above = lambda d: d[1:2 * n + 1]
    left = lambda d: d[2 * n + 1:]
    # nothing available: 1 << (depth - 1) everywhere
    assert (fill([False] * total) == 128).all()
    # everything available: copies
    d = fill([True] * total)
    assert d[0] == at(-1, -1) and list(above(d)) == [at(x, -1) for x in range(2 * n)] and list(left(d)) == [at(-1, y) for y in range(2 * n)]
    # top row of the picture (left + below-left available only): corner and the whole top row take the TOP sample of the left column
    f = [True] * lu + [False] * (lu + 1)
    d = fill(f)
    assert list(left(d)) == [at(-1, y) for y in range(2 * n)] and d[0] == at(-1, 0) and (above(d) == at(-1, 0)).all()
    # left column of the picture (above + above-right only): the leading run (below-left, left, corner) takes the first above sample
    f = [False] * (lu + 1) + [True] * lu
    d = fill(f)
    assert list(above(d)) == [at(x, -1) for x in range(2 * n)] and d[0] == at(0, -1) and (left(d) == at(0, -1)).all()
    # above-right unavailable: it repeats the last above sample; below-left unavailable: it takes the first (lowest) left sample
    f = [False] * units + [True] * units + [True] + [True] * units + [False] * units
    d = fill(f)
    assert list(above(d)[:n]) == [at(x, -1) for x in range(n)] and (above(d)[n:] == at(n - 1, -1)).all()
    assert list(left(d)[:n]) == [at(-1, y) for y in range(n)] and (left(d)[n:] == at(-1, n - 1)).all() and d[0] == at(-1, -1)
    # below-left available, above-right not
    f = [True] * lu + [True] + [True] * units + [False] * units
    d = fill(f)
    assert list(left(d)) == [at(-1, y) for y in range(2 * n)] and (above(d)[n:] == at(n - 1, -1)).all()
    # a leading unavailable run of three units, then one available unit, a hole, the rest available
    f = [False] * 3 + [True] + [False] + [True] * (total - 5)
    d = fill(f)
    path = np.concatenate([left(d)[::-1], d[0:1], above(d)])               # bottom of below-left ... corner ... end of above-right
    src = np.array([at(-1, 2 * n - 1 - i) for i in range(2 * n)] + [at(-1, -1)] + [at(x, -1) for x in range(2 * n)])
    assert (path[:12] == src[12]).all() and list(path[12:16]) == list(src[12:16]) and list(path[17:]) == list(src[17:])
    assert path[16] == src[15]                     # the hole (the corner unit: one sample of the path) takes the sample just before it
    # a hole of one above unit in the middle of the top row
    f = [True] * (lu + 1) + [True, False, True, True]
    d = fill(f)
    assert (above(d)[4:8] == at(3, -1)).all() and list(above(d)[8:]) == [at(x, -1) for x in range(8, 16)]
    # chroma units of two samples walk the same way
    dc = IE.fill_reference_samples(pl, off, stride, [False] * units + [True] * units + [True] + [True] * units + [False] * units, 4, 2, depth)
    assert (dc[1 + 4:1 + 8] == at(3, -1)).all() and (dc[8 + 1 + 4:] == at(-1, 3)).all()
    # the contents of unavailable samples do not matter
    f = [False] * units + [True] * units + [False] + [True] * units + [False] * units
    d0 = fill(f)
    pl2 = pl.copy()
    for y in range(n, 2 * n):
        pl2[off + y * stride - 1] ^= 0x55
    for x in range(n, 2 * n):
        pl2[off - stride + x] ^= 0x55
    pl2[off - stride - 1] ^= 0x55
    assert np.array_equal(d0, IE.fill_reference_samples(pl2, off, stride, f, n, unit, depth))


def test_neighbour_flags_follow_coding_order():
    """First block of a picture: nothing; a CTU's first block inside the picture: below-left from the CTU on the left, above-right from
    the CTU above; the rightmost block column of a CTU reaches into the CTU above-right; the last CTU row has no below-left outside."""
    n, w64, h64 = 16, 256, 192
    u = n // 4
    assert not any(IE.neighbour_flags(0, 0, n, w64, h64))
    f = IE.neighbour_flags(64, 64, n, w64, h64)
    assert all(f)                                                  # below-left: CTU (0, 1), z 5 of it ... all coded
    f = IE.neighbour_flags(64 + 48, 64, n, w64, h64)                # rightmost column: above-right = CTU (2, 0)
    assert all(f[2 * u:]) and not any(f[:u]) and all(f[u:2 * u])    # below-left (64 + 32, 64 + 16) comes later in z-order
    f = IE.neighbour_flags(64, 64 + 48, n, w64, h64)                # bottom-left block of a CTU: below-left lies in the CTU row below
    assert not any(f[:u]) and all(f[u:])
    f = IE.neighbour_flags(192 + 48, 64, n, w64, h64)               # right edge of the picture: above-right is outside
    assert not any(f[3 * u + 1:]) and all(f[2 * u:3 * u + 1])
    f = IE.neighbour_flags(16, 16, n, w64, h64)                     # z 3 of the first CTU: above-right (z 1... no: (32, 0) is z 4) not coded
    assert not any(f[3 * u + 1:]) and not any(f[:u]) and all(f[u:3 * u + 1])


@pytest.mark.parametrize("depth", [8, 10])
def test_picture_meets_every_outcome(depth):
    """The condition that keeps the GPU comparison from passing on a degenerate field.  On intra_expect.test_picture (256x192, qp 30 / 42,
    sign hiding, lambda8 1024, mode bits (2, 3, 6)) the oracle expectation alone meets, each on at least 3 % of the blocks: at level 1
    winners DC, planar, angular below 18, angular from 18, an MPM-priced winner, a non-MPM winner, a block whose left and above modes
    differ, num_sig == 0, num_sig > 1; at level 2 strong smoothing taken and refused; plus at least one decision the mode bits flip.
    Smallest share found: planar at level 1, 6.8 % (8-bit) / 6.2 % (10-bit); strong smoothing taken at level 2: 12.5 % / 10.4 %."""
    pl, w64, h64 = IE.padded_planes(IE.test_picture(depth))
    qp = 30 + 12 * (depth == 10)
    e = IE.expect(depth, pl, w64, h64, 1, qp, flags=3)
    shares = {k: float(m.mean()) for k, m in e["masks"].items()}
    print(f"depth {depth} level 1 (tables {e['tables']}):", {k: round(v, 3) for k, v in shares.items()})
    for k in ("dc", "planar", "angular_lt18", "angular_ge18", "mpm_priced", "non_mpm", "left_above_differ", "num_sig_0", "num_sig_gt1"):
        assert shares[k] >= 0.03, f"depth {depth} level 1: outcome {k} on {shares[k]:.3%} of the blocks"
    assert e["masks"]["bits_flip"].any()
    assert (e["cost"][:, 1] >= e["cost"][:, 0]).all() and (e["mode"] < 35).all()
    e2 = IE.expect(depth, pl, w64, h64, 2, qp, flags=3)
    shares = {k: float(m.mean()) for k, m in e2["masks"].items()}
    print(f"depth {depth} level 2:", {k: round(v, 3) for k, v in shares.items()})
    for k in ("strong_taken", "strong_refused"):
        assert shares[k] >= 0.03, f"depth {depth} level 2: outcome {k} on {shares[k]:.3%} of the blocks"
    # the walk does not depend on what the recon planes held before, and switching strong smoothing off changes the result
    other = IE.expect(depth, pl, w64, h64, 2, qp, flags=3, recon_init=IE.garbage_planes(depth, [np.asarray(p).reshape(-1).shape for p in pl], seed=78))
    for k in ("mode", "levels", "num_sig", "dist", "cost", "levels_c0", "levels_c1"):
        assert np.array_equal(e2[k], other[k]), k
    _, _, stride, rows, org = IE.F.padded_dims(w64, h64)
    inner = lambda a: a.reshape(rows, stride)[IE.F.MARGIN_Y:IE.F.MARGIN_Y + h64, IE.F.MARGIN_X:IE.F.MARGIN_X + w64]
    assert np.array_equal(inner(e2["recon"]), inner(other["recon"]))
    weak = IE.expect(depth, pl, w64, h64, 2, qp, flags=3, strong=False)
    assert not weak["masks"]["strong_taken"].any() and not np.array_equal(inner(weak["recon"]), inner(e2["recon"]))
