"""GPU parity of the persistent TU-stage kernels past their first resident pass.

At 16 and 32 points every TU-stage entry launches one resident set of single-wavefront workgroups (x265hip_tu_launch_grid) and each
wavefront walks blocks v, v + grid, ...  What only happens from a wavefront's second block on - the 16-point luma kernel's next block
prefetched into registers, the MFMA operands and LDS buffers reused, sNumSig reset, the XCD order's tail past the last multiple of 8 -
needs launches of more than two full passes.  Every case here asks the library for the grid g and sizes its picture or job list to
nblocks >= 2 g + 1 with nblocks % g != 0 (and, where the block count allows, nblocks % 8 != 0), asserts that, and compares EVERY output
buffer, started as a sentinel, with the oracle bit for bit: recon with its margins, levels, num_sig, dist, the captured coefficients /
deltaU and the denoiser's running sums.  Motion vectors are synthesised (quarter samples of every phase) instead of searched."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
S = importlib.import_module("x265-yuuki-asuna_amd.stages")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")

CTUS_W = 37                      # odd: with an odd CTU height the picture has an odd CTU count (4 blocks per CTU -> nblocks % 8 == 4)
SENT8, SENT16 = 0xA5, 0x5A5A     # sentinel samples (0x5A5A is no 10 / 12-bit sample)
QUANT_SCALES, INV_QUANT_SCALES = (26214, 23302, 20560, 18396, 16384, 14564), (40, 45, 51, 57, 64, 72)      # scalinglist.cpp:129-130


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_api
    return oracle_api


def _nthreads():
    sys.path.insert(0, ROOT)
    import bench
    return min(16, bench.effective_cpus())


def _passes(nblocks, g, tail):
    """asserts the multi-pass geometry; returns the description every assertion message of the case carries"""
    what = f"nblocks {nblocks}, grid {g}, {-(-nblocks // g)} passes"
    assert nblocks >= 2 * g + 1, what + ": fewer than two full passes"
    assert nblocks % g != 0, what + ": no partial last pass"
    if tail:
        assert nblocks % 8 != 0, what + ": no tail past the last multiple of 8 (XCD order)"
    return what


def _picture(entry, n, depth, tables, per_ctu, nplanes=1):
    """(w64, h64, nblocks, g): CTUS_W CTUs wide and the smallest odd number of CTU rows whose blocks fill two passes of the entry's grid
    and part of a third"""
    g = A.tu_launch_grid(entry, n, depth, tables, nplanes, 1 << 30)
    rows = 1
    while CTUS_W * rows * per_ctu < 2 * g + 1 or (CTUS_W * rows * per_ctu) % g == 0:
        rows += 2
    nb = CTUS_W * rows * per_ctu
    assert A.tu_launch_grid(entry, n, depth, tables, nplanes, nb) == g
    return CTUS_W * 64, rows * 64, nb, g


def _mvs(rng, nctu):
    """mv records [nctu * 85, 2] with quarter-sample vectors of every phase in .y; integer parts in [-24, 24] keep every block's filter
    apron inside the picture margins (luma 96 x 80, chroma 96 x 40 samples at 1/8 of a chroma sample)"""
    q = rng.integers(-96, 100, size=(nctu * 85, 2))
    m = np.zeros((nctu * 85, 2), np.int32)
    m[:, 1] = (q[:, 0] & 0xffff) | (q[:, 1] << 16)
    return m


def _phases(m, nctu, level, mask):
    """the fractional phases (x, y) of the records a stage at `level` reads"""
    lbase, npu = (0, 64, 80)[level], (64, 16, 4)[level]
    v = m.reshape(nctu, 85, 2)[:, lbase:lbase + npu, 1].reshape(-1).astype(np.int64)
    return {(int(a), int(b)) for a, b in zip(v & mask, (v >> 16) & mask)}


def _sentinel(depth):
    return SENT8 if depth == 8 else SENT16


def _dev_plane(buf, dev):
    import torch
    return torch.from_numpy(buf.reshape(-1) if buf.dtype == np.uint8 else buf.reshape(-1).view(np.int16)).to(dev)


def _fill_outputs(st):
    st.levels.fill_(0x5a5a)
    st.num_sig.fill_(0x5a5a5a5a)
    st.dist.fill_(0x5a5a5a5a5a5a5a5a)


def _assert_plane(got, erec, stride, org, w, h, sentinel, what):
    """got: the whole device plane; erec: the oracle's plane, which writes exactly the w x h picture area at org - every other sample
    (the margins) must still hold the sentinel"""
    got = got.reshape(-1)
    exp = np.full_like(got, sentinel)
    r0, c0 = divmod(org, stride)
    exp.reshape(-1, stride)[r0:r0 + h, c0:c0 + w] = erec.reshape(-1, stride)[r0:r0 + h, c0:c0 + w]
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (f"{what}: recon differs at {bad.size} samples, first (row, col) from sample (0,0) "
                           f"{[((int(b) - org) // stride, (int(b) - org) % stride) for b in bad[:4]]}")


def _assert_outputs(st, elev, ens, edist, what):
    assert np.array_equal(st.levels.cpu().numpy(), elev), f"{what}: levels differ"
    assert np.array_equal(st.num_sig.cpu().numpy().view(np.uint32), ens), f"{what}: numSig differs"
    assert np.array_equal(st.dist.cpu().numpy().view(np.uint64), edist), f"{what}: SSE differs"
    assert (ens > 1).any() and np.count_nonzero(elev) > 1000, f"{what}: a degenerate case"


class _Tables:
    """Scaling-list coefficients, denoiser offsets with running sums that start from the same non-zero values on both sides, and the
    capture of the coefficients / deltaU for `ncoef` coefficients - the device record and the oracle's copies."""

    def __init__(self, rng, n, qp, depth, ncoef, dev):
        import torch
        m = rng.integers(8, 64, size=n * n)
        self.depth = depth
        self.qc = ((QUANT_SCALES[qp % 6] << 4) // m).astype(np.int32)
        self.dqc = (INV_QUANT_SCALES[qp % 6] * m).astype(np.int32)
        self.off = rng.integers(0, 5 << (depth - 8), size=n * n).astype(np.uint16)
        self.sum0 = rng.integers(0, 1 << 20, size=n * n).astype(np.uint32)
        self.osum = self.sum0.copy()
        self.e_dct, self.e_du = np.full(ncoef, 0x5a5a, np.int16), np.full(ncoef, 0x5a5a5a5a, np.int32)
        t = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)
        self.d_sum = t(self.sum0.view(np.int32).copy())
        self.d_dct = torch.full((ncoef,), 0x5a5a, dtype=torch.int16, device=dev)
        self.d_du = torch.full((ncoef,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
        self.rec = A.tu_tables(t(self.qc), t(self.dqc), t(self.off), self.d_sum, self.d_dct, self.d_du)

    def run_oracle(self, O, fn):
        O.set_tu_tables(self.depth, self.qc, self.dqc, self.off, self.osum)
        O.set_tu_capture(self.depth, self.e_dct, self.e_du)
        try:
            return fn()
        finally:
            O.set_tu_tables(self.depth)
            O.set_tu_capture(self.depth)

    def check(self, what):
        assert np.array_equal(self.d_sum.cpu().numpy().view(np.uint32), self.osum), f"{what}: denoiser residual sums differ"
        assert not np.array_equal(self.osum, self.sum0), f"{what}: the denoiser summed nothing"
        assert np.array_equal(self.d_dct.cpu().numpy(), self.e_dct), f"{what}: captured coefficients differ"
        assert np.array_equal(self.d_du.cpu().numpy(), self.e_du), f"{what}: captured deltaU differs"
        assert np.count_nonzero(self.e_dct) > 1000, f"{what}: the capture holds almost nothing"


@pytest.mark.parametrize("depth,level,qp,flags,tables", [(8, 1, 30, 2, False), (8, 2, 24, 0, False), (10, 1, 36, 3, False), (10, 2, 34, 2, False),
                                                         (12, 1, 44, 0, False), (12, 2, 40, 3, False),
                                                         # scaling lists + denoiser + coefficient capture (the TB = true instances)
                                                         (8, 1, 28, 3, True), (10, 2, 36, 2, True)])
def test_inter_recon_multi_pass_matches_oracle(depth, level, qp, flags, tables):
    """x265hip_inter_recon at 16 points (the AHEAD register prefetch of the next block) and 32 points (only its vector travels ahead)."""
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    n = 8 << level
    w, h, nb, g = _picture(A.TU_ENTRY_INTER, n, depth, tables, (64 // n) ** 2)
    what = f"luma {n}x{n} {depth}-bit flags {flags}{' tables' if tables else ''}: " + _passes(nb, g, tail=level == 2)
    rng = np.random.default_rng([71, depth, level, qp])
    clip = F.synth_clip(w, h, 2, depth=depth, seed=710 + level)
    cur, ref = P.DevicePicture(clip[1][0], dev), P.DevicePicture(clip[0][0], dev)
    nctu = (w // 64) * (h // 64)
    mv = _mvs(rng, nctu)
    assert len(_phases(mv, nctu, level, 3)) == 16
    st = S.InterRecon(nctu, w, h, depth, level, qp, dev, intra_slice=flags)
    _fill_outputs(st)
    tab = _Tables(rng, n, qp, depth, st.levels.numel(), dev) if tables else None
    st.tables = tab.rec if tables else None
    recon = torch.full_like(cur.t, _sentinel(depth))
    st.run(cur, ref, recon, torch.from_numpy(mv.reshape(-1)).to(dev))
    torch.cuda.synchronize()
    call = lambda: O.inter_recon(depth, cur.host, cur.stride, cur.org, ref.host, ref.stride, ref.org, w, h, level, mv, qp, intra_slice=flags,
                                 nthreads=_nthreads())
    erec, elev, ens, edist = tab.run_oracle(O, call) if tables else call()
    _assert_outputs(st, elev, ens, edist, what)
    _assert_plane(recon.cpu().numpy().view(cur.host.dtype), erec, cur.stride, cur.org, w, h, _sentinel(depth), what)
    if tables:
        tab.check(what)


def _chroma_planes(w, h, depth, seed):
    """(current, reference) padded chroma planes of a w x h (luma) picture: textured planes of chroma size"""
    clip = F.synth_clip(w // 2, h // 2, 2, depth=depth, seed=seed)
    return [F.pad_chroma(clip[k][0], w, h) for k in (1, 0)]


@pytest.mark.parametrize("depth,qp,pair", [(8, 30, False), (10, 38, False), (8, 26, True), (10, 34, True)])
def test_inter_recon_chroma_multi_pass_matches_oracle(depth, qp, pair):
    """x265hip_inter_recon_chroma at level 2 (the persistent 16-point chroma kernel); pair: x265hip_inter_recon_chroma_pair, whose grid
    is split over the two planes in y - each plane with its own planes, QP and flags against the oracle."""
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    level, nplanes = 2, 2 if pair else 1
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_CHROMA, 16, depth, False, 4, nplanes)
    what = f"chroma 16x16 {depth}-bit {'pair' if pair else 'one plane'}: " + _passes(nb, g, tail=True)
    rng = np.random.default_rng([73, depth, qp])
    nctu = (w // 64) * (h // 64)
    mv = _mvs(rng, nctu)
    assert len(_phases(mv, nctu, level, 7)) == 64
    d_mv = torch.from_numpy(mv.reshape(-1)).to(dev)
    planes = [_chroma_planes(w, h, depth, 730 + 7 * depth + c) for c in range(nplanes)]
    stride, org = planes[0][0][1], planes[0][0][2]
    sts = [S.InterReconChroma(nctu, w, h, depth, level, qp - 3 * c, dev, intra_slice=2 + c) for c in range(nplanes)]
    fencs = [_dev_plane(p[0][0], dev) for p in planes]
    frefs = [_dev_plane(p[1][0], dev) for p in planes]
    recons = [torch.full_like(f, _sentinel(depth)) for f in fencs]
    for st in sts:
        _fill_outputs(st)
    if pair:
        S.InterReconChroma.run_pair(sts, fencs, frefs, recons, stride, org, d_mv)
    else:
        sts[0].run(fencs[0], frefs[0], recons[0], stride, org, d_mv)
    torch.cuda.synchronize()
    for c, st in enumerate(sts):
        fenc_h, fref_h = planes[c][0][0].reshape(-1), planes[c][1][0].reshape(-1)
        erec, elev, ens, edist = O.inter_recon_chroma(depth, fenc_h, fref_h, stride, org, w, h, level, mv, st.qp, intra_slice=st.intra,
                                                      nthreads=_nthreads())
        _assert_outputs(st, elev, ens, edist, f"plane {c}, {what}")
        _assert_plane(recons[c].cpu().numpy().view(fenc_h.dtype), erec, stride, org, w // 2, h // 2, _sentinel(depth), f"plane {c}, {what}")
    if pair:
        assert not torch.equal(sts[0].levels, sts[1].levels)


@pytest.mark.parametrize("depth,level,qp,weights", [(12, 1, 46, ((1, -20, 100, 4), (1, 90, 7, 3))), (10, 2, 38, ((1, 61, 4, 6), None))])
def test_inter_recon_bi_multi_pass_matches_oracle(depth, level, qp, weights):
    """x265hip_inter_recon_bi with explicit weights: 12-bit 16-point (the mix the 4K test lacks), and a 32-point case with a partial
    list of blocks past the last multiple of 8."""
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    n = 8 << level
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_BI, n, depth, False, (64 // n) ** 2)
    what = f"bi luma {n}x{n} {depth}-bit: " + _passes(nb, g, tail=level == 2)
    rng = np.random.default_rng([75, depth, level])
    clip = F.synth_clip(w, h, 3, depth=depth, seed=750 + level)
    cur, r0, r1 = P.DevicePicture(clip[1][0], dev), P.DevicePicture(clip[0][0], dev), P.DevicePicture(clip[2][0], dev)
    nctu = (w // 64) * (h // 64)
    mvs = [_mvs(rng, nctu) for _ in range(2)]
    dirs = rng.integers(1, 4, size=nb).astype(np.uint8)
    st = S.InterReconBi(nctu, w, h, depth, level, qp, dev, intra_slice=2)
    _fill_outputs(st)
    recon = torch.full_like(cur.t, _sentinel(depth))
    st.run(cur, r0, r1, recon, torch.from_numpy(mvs[0].reshape(-1)).to(dev), torch.from_numpy(mvs[1].reshape(-1)).to(dev),
           dir_flags=torch.from_numpy(dirs).to(dev), weights=weights)
    torch.cuda.synchronize()
    erec, elev, ens, edist = O.inter_recon_bi(depth, cur.host.reshape(-1), cur.stride, cur.org, r0.host.reshape(-1), r1.host.reshape(-1), w, h, level,
                                              mvs[0], mvs[1], qp, dir_flags=dirs, intra_slice=2, weights=weights, nthreads=_nthreads())
    _assert_outputs(st, elev, ens, edist, what)
    _assert_plane(recon.cpu().numpy().view(cur.host.dtype), erec, cur.stride, cur.org, w, h, _sentinel(depth), what)
    assert all((dirs == d).any() for d in (1, 2, 3))


@pytest.mark.parametrize("depth,qp,weights", [(8, 28, None), (10, 36, ((1, 45, 6, 6), (1, 70, -9, 6)))])
def test_inter_recon_chroma_bi_multi_pass_matches_oracle(depth, qp, weights):
    """x265hip_inter_recon_chroma_bi at level 2 (persistent 16-point chroma blocks), with and without explicit weights."""
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    level = 2
    w, h, nb, g = _picture(A.TU_ENTRY_INTER_CHROMA_BI, 16, depth, False, 4)
    what = f"bi chroma 16x16 {depth}-bit{' weighted' if weights else ''}: " + _passes(nb, g, tail=True)
    rng = np.random.default_rng([77, depth, qp])
    nctu = (w // 64) * (h // 64)
    mvs = [_mvs(rng, nctu) for _ in range(2)]
    dirs = rng.integers(1, 4, size=nb).astype(np.uint8)
    clip = F.synth_clip(w // 2, h // 2, 3, depth=depth, seed=770 + depth)
    (cur, stride, org), (p0, _, _), (p1, _, _) = (F.pad_chroma(clip[k][0], w, h) for k in (1, 0, 2))
    st = S.InterReconChromaBi(nctu, w, h, depth, level, qp, dev, intra_slice=2)
    _fill_outputs(st)
    d_cur = _dev_plane(cur, dev)
    recon = torch.full_like(d_cur, _sentinel(depth))
    st.run(d_cur, _dev_plane(p0, dev), _dev_plane(p1, dev), recon, stride, org, torch.from_numpy(mvs[0].reshape(-1)).to(dev),
           torch.from_numpy(mvs[1].reshape(-1)).to(dev), dir_flags=torch.from_numpy(dirs).to(dev), weights=weights)
    torch.cuda.synchronize()
    erec, elev, ens, edist = O.inter_recon_chroma_bi(depth, cur.reshape(-1), p0.reshape(-1), p1.reshape(-1), stride, org, w, h, level, mvs[0], mvs[1], qp,
                                                     dir_flags=dirs, intra_slice=2, weights=weights, nthreads=_nthreads())
    _assert_outputs(st, elev, ens, edist, what)
    _assert_plane(recon.cpu().numpy().view(cur.dtype), erec, stride, org, w // 2, h // 2, _sentinel(depth), what)


@pytest.mark.parametrize("depth,n,qp,islice,chroma,tables", [(8, 16, 30, 3, False, False), (10, 16, 33, 2, True, True),
                                                             (8, 32, 24, 1, True, False), (10, 32, 36, 3, False, True)])
def test_intra_recon_multi_pass_matches_oracle(depth, n, qp, islice, chroma, tables):
    """x265hip_intra_recon_batch at 16 / 32 points: (TU, mode) jobs - all 35 modes of one TU after the other - past two passes."""
    import torch
    from test_gpu_intra_recon import _smooth
    dev = torch.device("cuda:0")
    O = _oracle()
    g = A.tu_launch_grid(A.TU_ENTRY_INTRA, n, depth, tables, 1, 1 << 30)
    njobs = 2 * g + g // 2 + 3
    what = f"intra {n}x{n} {depth}-bit {'chroma' if chroma else 'luma'}{' tables' if tables else ''}: " + _passes(njobs, g, tail=True)
    assert A.tu_launch_grid(A.TU_ENTRY_INTRA, n, depth, tables, 1, njobs) == g
    rng = np.random.default_rng([79, depth, n, qp])
    dt = np.uint8 if depth == 8 else np.uint16
    pmax = (1 << depth) - 1
    ntu = -(-njobs // 35)
    W = n * ntu
    yy, xx = np.mgrid[0:n, 0:W]
    src = np.clip(np.rint((0.5 + 0.35 * np.sin(xx / 9.0) * np.cos(yy / 5.0)) * pmax + rng.normal(0, 3.0 * (1 << (depth - 8)), (n, W))), 0, pmax).astype(dt)
    fenc_stride = W + 16
    fenc = np.zeros((n, fenc_stride), dtype=dt)
    fenc[:, :W] = src
    nbw = 4 * n + 1
    nbr = np.zeros((ntu, 2, nbw + 3), dtype=dt)
    for t in range(ntu):
        base = int(src[:, t * n:(t + 1) * n].mean())
        a = np.clip(base + rng.integers(-12 << (depth - 8), 13 << (depth - 8), nbw), 0, pmax).astype(dt)
        nbr[t, 0, :nbw] = a
        nbr[t, 1, :nbw] = _smooth(a)
    jobs = np.zeros(njobs, dtype=A.job_dtype())
    rs = n + 5
    j = np.arange(njobs)
    t = j // 35
    jobs["off"] = np.stack([t * n, (2 * t) * (nbw + 3), (2 * t + 1) * (nbw + 3), j * n * rs], axis=1)
    jobs["arg"][:, 0] = j % 35
    recon_len = njobs * n * rs
    tab = _Tables(rng, n, qp, depth, njobs * n * n, dev) if tables else None
    call = lambda: O.intra_recon(depth, n, fenc.reshape(-1), fenc_stride, nbr.reshape(-1), recon_len, rs, qp, islice, jobs, chroma=chroma,
                                 nthreads=_nthreads())
    erec, elev, ens, edist = tab.run_oracle(O, call) if tables else call()
    sent = _sentinel(depth)
    d_rec = torch.full((recon_len,), sent, dtype=torch.uint8 if depth == 8 else torch.int16, device=dev)
    d_lev = torch.full((njobs * n * n,), 0x5a5a, dtype=torch.int16, device=dev)
    d_ns = torch.full((njobs,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    d_dist = torch.full((njobs,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
    A.intra_recon_batch(depth, n, _dev_plane(fenc, dev), fenc_stride, _dev_plane(nbr, dev), d_rec, rs, qp, islice,
                        torch.from_numpy(jobs.view(np.uint8).reshape(-1)).to(dev), njobs, d_lev, d_ns, d_dist, chroma=chroma, tables=tab.rec if tables else None)
    torch.cuda.synchronize()
    assert np.array_equal(d_lev.cpu().numpy(), elev), f"{what}: levels differ"
    assert np.array_equal(d_ns.cpu().numpy().view(np.uint32), ens), f"{what}: numSig differs"
    assert np.array_equal(d_dist.cpu().numpy().view(np.uint64), edist), f"{what}: SSE differs"
    assert (ens > 1).any(), f"{what}: a degenerate case"
    # only the n x n block of each job is written; the row padding of the recon stride keeps the sentinel
    exp = np.full(recon_len, sent, dt)
    exp.reshape(njobs, n, rs)[:, :, :n] = erec.reshape(njobs, n, rs)[:, :, :n]
    got = d_rec.cpu().numpy().view(dt)
    assert np.array_equal(got, exp), f"{what}: recon differs at {np.count_nonzero(got != exp)} samples"
    if tables:
        tab.check(what)
