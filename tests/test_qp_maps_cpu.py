"""CPU: the step between the lookahead's QP offsets and the coding stages (x265hip_cu_qp_maps - host logic in libx265hip.so, no device) against
a literal Python restatement of Analysis::calculateQpforCuSize + Quant::setQPforQuant / setChromaQP (tests/qp_map_expect.py), the records
that carry the maps against the header, the argument checks, and the coverage of the map the GPU tests code with."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import qp_map_expect as QE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("x265-yuuki-asuna_amd.frames")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")


EINVAL = -2          # X265HIP_EINVAL


def _both(depth, w, h, level, qg, base, offs, **kw):
    cu, tu = A.cu_qp_maps(depth, w, h, level, qg, base, offs, **kw)
    ecu, etu = QE.cu_qp_maps_restated(depth, w, h, level, qg, base, offs, **kw)
    assert cu.dtype == np.int8 and tu.dtype == np.int8 and cu.shape == (h // 8, w // 8) and tu.shape == (3, h // 8, w // 8)
    assert np.array_equal(cu, ecu), f"cu_qp differs in {np.count_nonzero(cu != ecu)} cells"
    assert np.array_equal(tu, etu), f"tu_qp differs in {np.count_nonzero(tu != etu)} cells"
    return cu, tu


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("qg", [8, 16])
@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("w,h", [(256, 192), (64, 64)])
def test_builder_equals_the_restated_loop(depth, qg, level, w, h):
    """Random offsets of AQ's magnitude (a few QP either way, arbitrary fractions), random base QPs and chroma offsets."""
    rng = np.random.default_rng([31, depth, qg, level, w])
    n = -(-h // qg) * -(-w // qg)
    for it in range(4):
        offs = rng.normal(0, 3.0, n)
        base = float(rng.uniform(10, 45))
        cu, tu = _both(depth, w, h, level, qg, base, offs, cb_qp_offset=int(rng.integers(-12, 13)), cr_qp_offset=int(rng.integers(-12, 13)))
        assert len(np.unique(cu)) > 1 or (w, h) == (64, 64)
        # every 8x8 cell of a block holds the block's value
        c = 1 << level
        assert np.array_equal(cu, np.kron(cu[::c, ::c], np.ones((c, c), np.int8)))
        assert np.array_equal(tu[0], cu + 6 * (depth - 8))
    cu, tu = _both(depth, w, h, level, qg, 30.5, None)          # no offsets: the rounded base QP everywhere
    assert (cu == 31).all()


@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("qg,level", [(8, 1), (8, 2), (16, 2), (16, 1), (16, 0), (8, 0)])
def test_hand_made_offsets_hit_ties_and_clips(depth, qg, level):
    """Multiples of 0.125 around base QPs ending in .0 and .5: averages of 4 and of 16 groups are exact in double, so ties at x.5 occur
    and must round up ((int)(qp + 0.5)); offsets large enough for both clips; chroma on both sides of 30 and at the clip to 57."""
    w, h = 256, 192
    rng = np.random.default_rng([37, depth, qg, level])
    n = -(-h // qg) * -(-w // qg)
    bd = 6 * (depth - 8)
    ties = clips_lo = clips_hi = 0
    seen_c = set()
    for base, lo, hi, cb, cr in ((30.0, 0, 51, 0, 0), (26.5, 0, 51, 3, -3), (33.5, 20, 40, 12, -12), (45.0, 0, 51, 12, 10), (8.5, 4, 51, -12, 6)):
        offs = rng.integers(-64, 65, n) * 0.125
        offs[rng.random(n) < 0.1] = 40.0
        offs[rng.random(n) < 0.1] = -40.0
        # the first row of blocks: every group of block i at (i - 3) + the fraction that puts base + offset on x.5
        gw, g = -(-w // qg), max(1, (8 << level) // qg)
        for i in range(w // (8 << level)):
            offs.reshape(-1, gw)[0:g, (i * (8 << level)) // qg:(i * (8 << level)) // qg + g] = (i - 3) + 0.5 - base % 1
        cu, tu = _both(depth, w, h, level, qg, base, offs, qp_min=lo, qp_max=hi, cb_qp_offset=cb, cr_qp_offset=cr)
        # count the ties from the exact averages
        bs, per = 8 << level, max(1, (8 << level) // qg)
        o2 = offs.reshape(-(-h // qg), -(-w // qg))
        for by in range(0, h, bs):
            for bx in range(0, w, bs):
                blk = o2[by // qg:by // qg + per, bx // qg:bx // qg + per]
                q = base + float(blk.sum()) / blk.size
                ties += (q * 2) % 2 == 1 and lo <= q + 0.5 <= hi
                if (q * 2) % 2 == 1 and lo <= q + 0.5 <= hi:
                    assert cu[by // 8, bx // 8] == int(q + 0.5) == int(q) + 1
        clips_lo += int((cu == lo).sum())
        clips_hi += int((cu == hi).sum())
        assert cu.min() >= lo and cu.max() <= hi
        seen_c |= set(np.unique(tu[1:] - bd).tolist())
    assert ties > 0 and clips_lo > 0 and clips_hi > 0
    assert min(seen_c) < 29 and max(seen_c) > 30 and {29, 30, 33, 34} & seen_c, sorted(seen_c)


def test_chroma_mapping_reaches_the_clip_to_57():
    """qp_max 51 + offset 12 = 63 -> clipped to 57 -> g_chromaScale 51; the low end clips to -QP_BD_OFFSET."""
    for depth in (8, 10, 12):
        bd = 6 * (depth - 8)
        offs = np.array([40.0] * 8 + [-40.0] * 8)
        cu, tu = _both(depth, 64, 64, 1, 16, 30.0, offs, cb_qp_offset=12, cr_qp_offset=-12)
        assert cu.max() == 51 and cu.min() == 0
        assert tu[1].max() == 51 + bd and tu[1].min() == 12 + bd
        assert tu[2].max() == QE.CHROMA_SCALE[39] + bd and tu[2].min() == max(-12, -bd) + bd
        # the uniform value is what stages.chroma_quant_qp forms today
        for q in np.unique(cu):
            i = np.argwhere(cu == q)[0]
            assert tu[1][i[0], i[1]] == S.chroma_quant_qp(int(q) + bd, depth, 12) and tu[2][i[0], i[1]] == S.chroma_quant_qp(int(q) + bd, depth, -12)


@pytest.mark.parametrize("depth,qg,mode", [(8, 16, 2), (8, 8, 2), (10, 16, 3), (10, 8, 1)])
def test_real_offsets_of_the_aq_fixture_picture(depth, qg, mode):
    """The oracle's calcAdaptiveQuantFrame offsets of the AQ fixture picture (tests/test_aq_host.py: synth_clip 320x176, seed 7; here over
    its padded 320x192 whole-CTU size) through the builder, every level."""
    import oracle_api as O
    clip = F.synth_clip(320, 176, 1, depth=depth, seed=7)
    yp, stride, org, w64, h64 = F.pad_plane(clip[0][0])
    _, offs, _, _, _ = O.aq_frame(depth, yp, stride, org, w64, h64, qg_size=qg, aq_mode=mode, aq_strength=1.0, weightp=False)
    assert len(offs) == -(-h64 // qg) * -(-w64 // qg) and len(np.unique(offs)) > 8
    for level in (0, 1, 2):
        cu, _ = _both(depth, w64, h64, level, qg, 28.0, offs)
        assert len(np.unique(cu)) >= 2, "AQ offsets that move no block's QP"


def test_records_match_the_header(tmp_path):
    """Sizes and offsets of the changed and the new records against include/x265hip.h as gcc lays them out."""
    pairs = {"x265hip_recon_params": S.ReconParams, "x265hip_recon_bi_params": S.ReconBiParams, "x265hip_cu_qp_params": A.CuQpParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "x265hip.h"', 'int main(void) {']
    for cname, cls in pairs.items():
        lines.append(f'  printf("{cname} . %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        cname, fname, val = line.split()
        cls = pairs[cname]
        expect = ctypes.sizeof(cls) if fname == "." else getattr(cls, fname).offset
        assert int(val) == expect, f"{cname}.{fname}: C says {val}, ctypes says {expect}"
        seen += 1
    assert seen == 19 + 7 + 14
    # the maps are the LAST fields: a caller that zero-initialises the longer record passes NULL
    assert S.ReconParams._fields_[-1][0] == "qp_map"
    for name in ("x265hip_cu_qp_maps", "x265hip_intra_picture_qp"):
        assert name in A.exported_symbols() and hasattr(A.lib(), name)


def test_cu_qp_maps_rejects_bad_arguments():
    offs = np.zeros(16)
    good = dict(depth=8, width=64, height=64, level=1, qg_size=16, base_qp=30.0, qp_offsets=offs)
    A.cu_qp_maps(**good)
    for bad in (dict(qg_size=32), dict(qg_size=4), dict(level=3), dict(level=-1), dict(width=72), dict(height=0), dict(depth=9), dict(qp_min=-1),
                dict(qp_max=52), dict(qp_min=40, qp_max=30), dict(cb_qp_offset=25), dict(cr_qp_offset=-25)):
        with pytest.raises(A.X265HipError) as e:
            A.cu_qp_maps(**dict(good, **bad))
        assert "cu_qp_maps" in str(e.value), bad
    with pytest.raises(A.X265HipError):
        A.cu_qp_maps(**dict(good, qp_offsets=np.zeros(15)))
    # NULL record / both outputs NULL
    f = A.lib().x265hip_cu_qp_maps
    f.argtypes = [ctypes.POINTER(A.CuQpParams)]
    assert f(None) < 0
    p = A.CuQpParams()
    p.depth, p.width, p.height, p.level, p.qg_size, p.qp_max = 8, 64, 64, 1, 16, 51
    assert f(ctypes.byref(p)) < 0 and b"NULL" in A.lib().x265hip_last_error()


def test_qp_map_together_with_tables_is_refused_without_a_device():
    """Scaling-list tables are selected per qp % 6 on the host: a record with both is an argument error, found before any device is asked for."""
    tab = A.TuTablesRec()
    L = A.lib()
    for name, rec in (("x265hip_inter_recon", S.ReconParams()), ("x265hip_inter_recon_chroma", S.ReconParams())):
        rec.depth, rec.width, rec.height, rec.level, rec.qp = 8, 64, 64, 1, 30
        rec.tables, rec.qp_map = ctypes.addressof(tab), 4096
        f = getattr(L, name)
        f.argtypes = [ctypes.POINTER(S.ReconParams), ctypes.c_void_p]
        assert f(ctypes.byref(rec), None) == EINVAL and b"qp_map together with tables" in L.x265hip_last_error(), name
    pair = L.x265hip_inter_recon_chroma_pair
    pair.argtypes = [ctypes.POINTER(S.ReconParams), ctypes.POINTER(S.ReconParams), ctypes.c_void_p]
    ok = S.ReconParams()
    assert pair(ctypes.byref(ok), ctypes.byref(rec), None) == EINVAL and b"qp_map together with tables" in L.x265hip_last_error()
    for name in ("x265hip_inter_recon_bi", "x265hip_inter_recon_chroma_bi"):
        q = S.ReconBiParams()
        q.base = rec
        f = getattr(L, name)
        f.argtypes = [ctypes.POINTER(S.ReconBiParams), ctypes.c_void_p]
        assert f(ctypes.byref(q), None) == EINVAL and b"qp_map together with tables" in L.x265hip_last_error(), name


@pytest.mark.parametrize("depth", [8, 10, 12])
@pytest.mark.parametrize("level,grid", [(1, 2048), (2, 2048), (2, 1024), (0, 1 << 30)])
@pytest.mark.parametrize("swizzled", [True, False])
def test_map_of_the_gpu_tests_covers_the_quantiser(depth, level, grid, swizzled, capsys):
    """The map the GPU tests code with (qp_map_expect.block_qps over the geometry of tests/test_gpu_tu_passes.py; level 0 at 256x192): every
    qp % 6 on at least 3 % of the blocks, at least four qp / 6, 0 and the depth's maximum, neighbours that differ in raster and z-order,
    and blocks v / v + grid of a wavefront's walk never at one QP.  The GPU tests assert the same on the maps they really use."""
    n = 8 << level
    per_ctu = (64 // n) ** 2
    if level == 0:
        w, h = 256, 192
    else:
        rows = 1
        while 37 * rows * per_ctu < 2 * grid + 1 or (37 * rows * per_ctu) % grid == 0:
            rows += 2
        w, h = 37 * 64, rows * 64
    nb = (w // 64) * (h // 64) * per_ctu
    vals = QE.map_values(depth)
    assert len(vals) <= 8 and {v % 6 for v in vals} == set(range(6)) and max(vals) == 51 + 6 * (depth - 8) and min(vals) == 0
    qpb = QE.block_qps(nb, min(grid, nb), vals, np.random.default_rng([41, depth, level]), swizzled)
    share = QE.coverage(qpb, w, h, level, depth)
    with capsys.disabled():
        print(f"\n  qp map {depth}-bit level {level} grid {grid} {'xcd' if swizzled else 'raster'} walk: smallest qp % 6 share {share:.3f} of {nb} blocks")
    cells = QE.cells_of_blocks(qpb, w, h, level)
    assert np.array_equal(QE.blocks_of_cells(cells, w, h, level), qpb)
