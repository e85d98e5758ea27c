"""GPU parity of the TU stages under a per-block QP map (qp_map of x265hip_recon_params) and of x265hip_intra_picture with its map and
lambda table.

The oracle stages take one QP, and stay as they are: inter blocks do not depend on each other, so the expectation for a map with the
values q1..qk (k <= 8) is the oracle stage run once per q, every block taken from the run of its own q (qp_map_expect.compose).  At 16 and 32
points the geometry is that of tests/test_gpu_tu_passes.py (37 CTUs wide, at least two full passes of the resident grid and part of a third),
and the map gives blocks v and v + grid of a wavefront's walk different QPs: where the 16-point luma kernel fetches block v + grid while it
codes block v, a QP that travelled with the wrong block changes levels.  Everything is compared bit for bit, sentinel-filled outputs and
recon margins included.  I pictures: the coding-order walk of tests/intra_expect.py with the block's own QPs (qp_map_expect.walk)."""
import importlib

import numpy as np
import pytest

import qp_map_expect as QE
from test_gpu_tu_passes import (_assert_outputs, _assert_plane, _chroma_planes, _dev_plane, _fill_outputs, _mvs, _nthreads, _oracle, _passes, _phases,
                                _picture, _sentinel)

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

ENTRIES = {"inter": A.TU_ENTRY_INTER, "bi": A.TU_ENTRY_INTER_BI, "chroma": A.TU_ENTRY_INTER_CHROMA, "pair": A.TU_ENTRY_INTER_CHROMA,
           "chroma_bi": A.TU_ENTRY_INTER_CHROMA_BI}
WEIGHTS = ((1, 61, 4, 6), None)


def _geometry(kind, depth, level):
    """(w, h, nblocks, grid, description): the multi-pass picture of test_gpu_tu_passes at 16 / 32 points, 256x192 at level 0 (one block
    per workgroup: every block is a wavefront's first)"""
    chroma = kind in ("chroma", "pair", "chroma_bi")
    n = (4 if chroma else 8) << level
    per_ctu = (64 // (8 << level)) ** 2
    if level == 0:
        w, h = 256, 192
        nb = 12 * per_ctu
        g = A.tu_launch_grid(ENTRIES[kind], n, depth, False, 2 if kind == "pair" else 1, nb)
        assert g == nb
        return w, h, nb, g, f"{kind} {n}x{n} {depth}-bit: {nb} blocks, one per workgroup"
    w, h, nb, g = _picture(ENTRIES[kind], n, depth, False, per_ctu, 2 if kind == "pair" else 1)
    return w, h, nb, g, f"{kind} {n}x{n} {depth}-bit: " + _passes(nb, g, tail=level == 2)


class _Case:
    """Planes, vectors and stage objects of one entry: run(maps) launches it (maps: one device int8 map per plane or None), expect(run_q)
    composes the oracle's answer for one block QP array per plane."""

    def __init__(self, kind, depth, level, flags, qp, seed):
        import torch
        self.kind, self.depth, self.level, self.flags = kind, depth, level, flags
        self.dev = dev = torch.device("cuda:0")
        self.w, self.h, self.nb, self.g, self.what = _geometry(kind, depth, level)
        w, h = self.w, self.h
        self.nctu = nctu = (w // 64) * (h // 64)
        self.rng = rng = np.random.default_rng([83, depth, level, seed])
        self.chroma = kind in ("chroma", "pair", "chroma_bi")
        self.bi = kind in ("bi", "chroma_bi")
        self.nplanes = 2 if kind == "pair" else 1
        self.mvs = [_mvs(rng, nctu) for _ in range(2 if self.bi else 1)]
        assert len(_phases(self.mvs[0], nctu, level, 7 if self.chroma else 3)) == (64 if self.chroma else 16) or level == 0
        self.d_mvs = [torch.from_numpy(m.reshape(-1)).to(dev) for m in self.mvs]
        self.dirs = rng.integers(1, 4, size=self.nb).astype(np.uint8) if self.bi else None
        self.d_dirs = torch.from_numpy(self.dirs).to(dev) if self.bi else None
        nref = 3 if self.bi else 2
        if self.chroma:
            self.host = []                   # per plane: [cur, ref0(, ref1)] flat padded planes
            for c in range(self.nplanes):
                clip = F.synth_clip(w // 2, h // 2, nref, depth=depth, seed=830 + 7 * depth + c + seed)
                pads = [F.pad_chroma(clip[k][0], w, h) for k in ((1, 0, 2) if self.bi else (1, 0))]
                self.stride, self.org = pads[0][1], pads[0][2]
                self.host.append([p[0].reshape(-1) for p in pads])
            self.devp = [[_dev_plane(p, dev) for p in planes] for planes in self.host]
            cls = S.InterReconChromaBi if self.bi else S.InterReconChroma
            self.sts = [cls(nctu, w, h, depth, level, qp - 3 * c, dev, intra_slice=flags) for c in range(self.nplanes)]
            self.pw, self.ph, self.n, self.sub = w // 2, h // 2, 4 << level, 4
        else:
            clip = F.synth_clip(w, h, nref, depth=depth, seed=810 + level + seed)
            self.pics = [P.DevicePicture(clip[k][0], dev) for k in ((1, 0, 2) if self.bi else (1, 0))]
            self.stride, self.org = self.pics[0].stride, self.pics[0].org
            self.host = [[p.host.reshape(-1) for p in self.pics]]
            cls = S.InterReconBi if self.bi else S.InterRecon
            self.sts = [cls(nctu, w, h, depth, level, qp, dev, intra_slice=flags)]
            self.pw, self.ph, self.n, self.sub = w, h, 8 << level, 8
        self.recons = None

    def run(self, maps):
        import torch
        for st, m in zip(self.sts, maps or [None] * self.nplanes):
            _fill_outputs(st)
            st.qp_map = m
        sent = _sentinel(self.depth)
        if self.chroma:
            self.recons = [torch.full_like(p[0], sent) for p in self.devp]
            if self.kind == "pair":
                S.InterReconChroma.run_pair(self.sts, [p[0] for p in self.devp], [p[1] for p in self.devp], self.recons, self.stride, self.org, self.d_mvs[0])
            elif self.bi:
                p = self.devp[0]
                self.sts[0].run(p[0], p[1], p[2], self.recons[0], self.stride, self.org, self.d_mvs[0], self.d_mvs[1], dir_flags=self.d_dirs, weights=WEIGHTS)
            else:
                p = self.devp[0]
                self.sts[0].run(p[0], p[1], self.recons[0], self.stride, self.org, self.d_mvs[0])
        else:
            self.recons = [torch.full_like(self.pics[0].t, sent)]
            if self.bi:
                self.sts[0].run(self.pics[0], self.pics[1], self.pics[2], self.recons[0], self.d_mvs[0], self.d_mvs[1], dir_flags=self.d_dirs, weights=WEIGHTS)
            else:
                self.sts[0].run(self.pics[0], self.pics[1], self.recons[0], self.d_mvs[0])
        torch.cuda.synchronize()

    def outputs(self):
        """every output buffer of every plane, as host arrays"""
        return [(r.cpu().numpy().copy(), st.levels.cpu().numpy().copy(), st.num_sig.cpu().numpy().copy(), st.dist.cpu().numpy().copy())
                for r, st in zip(self.recons, self.sts)]

    def oracle(self, c, q):
        O, d, h = _oracle(), self.depth, self.host[c]
        st = self.sts[c]
        kw = dict(intra_slice=st.intra, nthreads=_nthreads())
        if self.kind == "inter":
            return O.inter_recon(d, h[0], self.stride, self.org, h[1], self.stride, self.org, self.w, self.h, self.level, self.mvs[0], q, **kw)
        if self.kind == "bi":
            return O.inter_recon_bi(d, h[0], self.stride, self.org, h[1], h[2], self.w, self.h, self.level, self.mvs[0], self.mvs[1], q, dir_flags=self.dirs,
                                    weights=WEIGHTS, **kw)
        if self.kind == "chroma_bi":
            return O.inter_recon_chroma_bi(d, h[0], h[1], h[2], self.stride, self.org, self.w, self.h, self.level, self.mvs[0], self.mvs[1], q, dir_flags=self.dirs,
                                           weights=WEIGHTS, **kw)
        return O.inter_recon_chroma(d, h[0], h[1], self.stride, self.org, self.w, self.h, self.level, self.mvs[0], q, **kw)

    def check(self, qpbs):
        """qpbs: per plane the QP of every block"""
        for c, (st, qpb) in enumerate(zip(self.sts, qpbs)):
            cells = QE.cells_of_blocks(qpb, self.w, self.h, self.level)
            erec, elev, ens, edist = QE.compose(lambda q: self.oracle(c, q), qpb, self.n, QE.sample_qps(cells, self.sub), self.stride, self.org, self.pw, self.ph)
            what = f"plane {c}, {self.what}"
            _assert_outputs(st, elev, ens, edist, what)
            _assert_plane(self.recons[c].cpu().numpy().view(self.host[c][0].dtype), erec, self.stride, self.org, self.pw, self.ph, _sentinel(self.depth), what)


def _maps(case, seed):
    """per plane: (block QPs, device map); the walk is the XCD order for the uni-predictive persistent kernels, the plain one for the others"""
    import torch
    out = []
    for c in range(case.nplanes):
        swizzled = not case.bi and case.level > 0
        g = min(case.g, case.nb)
        qpb = QE.block_qps(case.nb, g, QE.map_values(case.depth), np.random.default_rng([89, seed, c]), swizzled)
        share = QE.coverage(qpb, case.w, case.h, case.level, case.depth)
        print(f"  {case.what}: plane {c}, smallest qp % 6 share {share:.3f}")
        cells = QE.cells_of_blocks(qpb, case.w, case.h, case.level)
        out.append((qpb, torch.from_numpy(cells.reshape(-1)).to(case.dev)))
    if case.nplanes == 2:
        assert not np.array_equal(out[0][0], out[1][0])
    return out


# every entry at 16 and 32 points (chroma: 16 points at level 2); 8- and 10-bit, 12-bit once; sign hiding (flag 2) on and off
PERSISTENT = [("inter", 8, 1, 2), ("inter", 8, 2, 0), ("inter", 10, 1, 0), ("inter", 10, 2, 2), ("inter", 12, 1, 2),
              ("chroma", 8, 2, 2), ("chroma", 10, 2, 0), ("pair", 8, 2, 0), ("pair", 10, 2, 2),
              ("bi", 8, 1, 0), ("bi", 10, 2, 2), ("bi", 8, 2, 2), ("bi", 10, 1, 0),
              ("chroma_bi", 8, 2, 2), ("chroma_bi", 10, 2, 0)]


@pytest.mark.parametrize("kind,depth,level,flags", PERSISTENT)
def test_tu_stage_with_a_qp_map_equals_the_oracle_block_by_block(kind, depth, level, flags):
    case = _Case(kind, depth, level, flags, 30 + 6 * (depth - 8), seed=1)
    maps = _maps(case, 1)
    case.run([m for _, m in maps])
    case.check([q for q, _ in maps])


@pytest.mark.parametrize("kind,depth,flags", [("inter", 8, 2), ("inter", 10, 0), ("chroma", 8, 0), ("pair", 10, 2), ("bi", 8, 2), ("chroma_bi", 10, 0),
                                              ("inter", 12, 2)])
def test_level_0_with_a_qp_map(kind, depth, flags):
    """8-point luma / 4-point chroma blocks, one block per workgroup, 256x192"""
    case = _Case(kind, depth, 0, flags, 28 + 6 * (depth - 8), seed=2)
    maps = _maps(case, 2)
    case.run([m for _, m in maps])
    case.check([q for q, _ in maps])


@pytest.mark.parametrize("kind,depth,level", [("inter", 8, 1), ("inter", 8, 2), ("pair", 8, 2), ("bi", 10, 1), ("bi", 8, 2), ("chroma_bi", 8, 2), ("chroma", 10, 2),
                                              ("inter", 8, 0), ("pair", 10, 0)])
def test_a_map_filled_with_qp_changes_nothing(kind, depth, level):
    """Identity: a map that holds the record's qp in every cell gives byte-identical outputs - every buffer, margins and all - to the map-less
    launch of the same tree; and a map of another QP gives other levels (the map is read)."""
    import torch
    qp = 31 + 6 * (depth - 8)
    case = _Case(kind, depth, level, 2, qp, seed=3)
    case.run(None)
    plain = case.outputs()
    cells = (case.h // 8) * (case.w // 8)
    case.run([torch.full((cells,), st.qp, dtype=torch.int8, device=case.dev) for st in case.sts])
    for a, b in zip(plain, case.outputs()):
        for x, y, name in zip(a, b, ("recon", "levels", "num_sig", "dist")):
            assert np.array_equal(x, y), f"{case.what}: {name} changed under a map filled with qp"
    case.run([torch.full((cells,), st.qp - 7, dtype=torch.int8, device=case.dev) for st in case.sts])
    assert all(not np.array_equal(a[1], b[1]) for a, b in zip(plain, case.outputs())), f"{case.what}: the map is not read"


def test_out_of_range_entries_are_clamped():
    """Entries below 0 and above the depth's maximum code like 0 and like the maximum."""
    import torch
    case = _Case("inter", 8, 1, 0, 30, seed=4)
    cells = (case.h // 8) * (case.w // 8)
    outs = []
    for v in (-128, 0, 127, 51):
        case.run([torch.full((cells,), v, dtype=torch.int8, device=case.dev)])
        outs.append(case.outputs()[0])
    for k in range(4):
        assert np.array_equal(outs[0][k], outs[1][k]) and np.array_equal(outs[2][k], outs[3][k])
    assert not np.array_equal(outs[0][1], outs[2][1])
