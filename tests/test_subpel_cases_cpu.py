"""The inputs of the hostile-content sub-pel tests (tests/subpel_cases.py) checked with the oracle alone: every case the GPU modules run must
really reach the paths it is listed for - zero-cost keys at every level, vectors at the window's edge and far from the origin, both ends of
the interpolation clip, full-amplitude differences at 12 bits, a reconstruction that clips at both ends.  These are conditions on the
inputs: a case that misses one gets another seed, never a looser condition."""
import importlib

import numpy as np
import pytest

import subpel_cases as SC

F = importlib.import_module("x265-yuuki-asuna_amd.frames")


def measure(case):
    """What the oracle makes of a case: the figures the assertions below are about."""
    c = SC.build(*case.build)
    out = SC.refined(case)
    n = c.best.size
    qx, qy = SC.unpack_q(out)
    dqx, dqy = qx - 4 * c.imv[:, 0], qy - 4 * c.imv[:, 1]
    zero = (c.best >> np.uint64(32)) == 0
    level = np.tile(np.repeat(np.arange(4), (64, 16, 4, 1)), c.nctu)
    m = SimpleStats()
    m.zero_share = zero.mean()
    m.zero_levels = sorted(set(level[zero].tolist()))
    m.zero_kept = bool(((dqx == 0) & (dqy == 0))[zero].all())
    m.moved_share = ((dqx != 0) | (dqy != 0)).mean()
    m.sign_pairs = len(set(zip(np.sign(dqx).tolist(), np.sign(dqy).tolist())))
    m.max_dq = int(max(np.abs(dqx).max(), np.abs(dqy).max()))
    m.edge_share = ((np.abs(c.imv[:, 0]) == c.R) | (np.abs(c.imv[:, 1]) == c.R)).mean()
    m.qx_neg, m.qx_pos, m.qy_neg, m.qy_pos = (qx < 0).mean(), (qx > 0).mean(), (qy < 0).mean(), (qy > 0).mean()
    m.max_q = int(max(np.abs(qx).max(), np.abs(qy).max()))
    m.n = n
    if c.planes is not None:
        inner = np.stack([p[8:-8, 8:-8] for p in c.planes[1:]])
        m.planes_at_0, m.planes_at_max = (inner == 0).mean(), (inner == (1 << c.depth) - 1).mean()
    return m, c, out


class SimpleStats:
    def __repr__(self):
        return " ".join(f"{k}={v:.3f}" if isinstance(v, float) else f"{k}={v}" for k, v in vars(self).items())


def full_amplitude_tiles(c, thr):
    """4x4 tiles of PUs whose 16 differences against the reference at the record's integer vector all have |d| >= thr."""
    cur, ref = c.cur_img.astype(np.int64), c.ref.astype(np.int64)
    count = 0
    for (ctu, l, z, px, py, n), v in zip(SC.pu_list(c.w64, c.h64), c.imv):
        ry, rx = F.MARGIN_Y + py + int(v[1]), F.MARGIN_X + px + int(v[0])
        d = np.abs(cur[py:py + n, px:px + n] - ref[ry:ry + n, rx:rx + n]) >= thr
        count += int(d.reshape(n // 4, 4, n // 4, 4).all(axis=(1, 3)).sum())
    return count


def free_zero_keys(c):
    """Zero-cost keys with a non-zero vector on both axes whose reference block, and everything within 8 samples of it, is constant: every candidate
    of such a PU costs its mv bits alone, so without the zero-residual shortcut the cheaper vectors next to it would win."""
    ref = c.ref.astype(np.int64)
    count = 0
    for (ctu, l, z, px, py, n), v, key in zip(SC.pu_list(c.w64, c.h64), c.imv, c.best):
        if int(key) >> 32 or not v.all():
            continue
        ry, rx = F.MARGIN_Y + py + int(v[1]), F.MARGIN_X + px + int(v[0])
        blk = ref[ry - 8:ry + n + 8, rx - 8:rx + n + 8]
        count += int(blk.min() == blk.max())
    return count


@pytest.mark.parametrize("case", SC.PLANTED_CASES, ids=lambda c: c.id)
def test_planted_case_reaches_its_paths(case):
    m, c, out = measure(case)
    print(case.id, m)
    assert 0.10 <= m.zero_share <= 0.60, m
    assert m.zero_levels == [0, 1, 2, 3], m                    # a zero-cost key at each of the four levels (the 64x64 one crosses wavefronts)
    assert m.zero_kept                                          # the reference's shortcut: such a PU keeps its integer vector
    assert free_zero_keys(c) >= 4, free_zero_keys(c)           # ... where refining it would move it (8x8 and 16x16 PUs over the constant patch)
    assert m.moved_share >= 0.30, m
    # every sign pair of (dqx, dqy); subme 0 is one round of the four axis candidates and nothing after it, so a vector moves on one axis
    # or stays: five pairs are all it can reach
    assert m.sign_pairs == (9 if case.subme else 5), m
    if case.subme >= 3:
        assert m.max_dq >= 3, m                                 # two half-sample steps
    assert m.edge_share >= 0.10, m
    assert min(m.qx_neg, m.qx_pos, m.qy_neg, m.qy_pos) >= 0.20, m
    assert m.max_q <= 4 * c.R + 8, m                            # inside frames.qpel_cost_table
    if case.kind in ("edges", "inverse"):
        assert m.planes_at_0 >= 0.05 and m.planes_at_max >= 0.05, m
    if case.kind == "noise":
        assert m.planes_at_0 >= 0.01 and m.planes_at_max >= 0.01, m
    if case.kind == "inverse" and case.depth == 12:
        assert full_amplitude_tiles(c, 4000) >= 1               # 8 * 4095 = 32760: the int16 headroom of the packed Hadamard


@pytest.mark.parametrize("case", SC.FLAT_CASES, ids=lambda c: c.id)
def test_flat_case_is_decided_by_the_mv_cost(case):
    """Current all max against reference all 0 (or the other way round) with real, non-zero records: every candidate has the same distortion,
    so only the mv cost can move a vector - towards the origin, never away - and the cost table is read as far out as |q| = 4R."""
    m, c, out = measure(case)
    print(case.id, m)
    assert m.zero_share == 0
    qx, qy = SC.unpack_q(out)
    assert (np.abs(qx) <= 4 * np.abs(c.imv[:, 0])).all() and (np.abs(qy) <= 4 * np.abs(c.imv[:, 1])).all()
    assert m.moved_share >= 0.30, m
    assert m.edge_share >= 0.10, m
    assert min(m.qx_neg, m.qx_pos, m.qy_neg, m.qy_pos) >= 0.20, m
    assert m.max_q <= 4 * c.R + 8 and m.max_q > 4 * 40, m
    full = ((1 << c.depth) - 1) * np.tile(np.repeat(np.array([8, 16, 32, 64]) ** 2, (64, 16, 4, 1)), c.nctu)
    assert np.array_equal((c.best >> np.uint64(32)).astype(np.int64) - full,
                          F.mv_cost_table(c.R).astype(np.int64)[c.imv[:, 0] + c.R] + F.mv_cost_table(c.R).astype(np.int64)[c.imv[:, 1] + c.R])


def measure_recon(case, level, qp):
    c = SC.build(*case.build)
    mv = SC.refined(case)
    rec, levels, num_sig, dist = SC.oracle().inter_recon(c.depth, c.cur, c.stride, c.org, c.ref, c.stride, c.org, c.w64, c.h64, level, mv, qp)
    maxv = (1 << c.depth) - 1
    r = rec[F.MARGIN_Y:F.MARGIN_Y + c.h64, F.MARGIN_X:F.MARGIN_X + c.w64]
    return (num_sig > 0).mean(), ((r == 0) & (c.cur_img != 0)).mean(), ((r == maxv) & (c.cur_img != maxv)).mean()


@pytest.mark.parametrize("case,level,qp", SC.RECON_CASES, ids=lambda v: v.id if isinstance(v, SC.Case) else str(v))
def test_recon_case_codes_and_clips(case, level, qp):
    """The prediction and reconstruction clips of the TU stage: the oracle codes at least 30 % of the blocks, and at least 1 % of its
    reconstructed samples sit at 0, and 1 % at max, where the source does not."""
    coded, at0, atmax = measure_recon(case, level, qp)
    print(case.id, level, qp, f"coded {coded:.3f} at 0 {at0:.4f} at max {atmax:.4f}")
    assert coded >= 0.30
    assert at0 >= 0.01 and atmax >= 0.01
