"""GPU parity of the SAO stage's decision walk and of its reworked statistics kernel against the oracle, bit for bit, on the shapes that decide which code runs.

The serial decision walk (x265hip_sao_rdo -> sao_rdo_rows2_kernel): one CTU, one CTU row, one CTU column, two columns (the staging depth of
the candidate records), tall two-column strips of 44 and 50 CTU rows, 1080p and 4K, luma-only, per-CTU lambdas, B / P / I contexts.
Every case is CONDITIONED on the oracle's own luma parameters, computed on the CPU from the oracle's statistics: at least one merge-left
where there are two CTU columns, one merge-up where there are two CTU rows, and from 24 CTUs on also one CTU left without SAO - a walk
whose merge lanes did nothing cannot pass.

The statistics kernel (x265hip_sao_stats / x265hip_sao_planes): 64x64 luma, 32x32 chroma (plane_offset 2: four samples per lane), 16x16 and
32x32 luma footprints, partial right / bottom CTUs, 8 / 10 / 12 bits (8 bits takes the packed accumulators), and the three-plane launch
against the single-plane entry."""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
H = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def walk_case(depth, width, height, slice_type, qp, planes, per_ctu):
    """Everything of a decision-walk case the CPU can compute: the oracle's statistics of sao_rdo_case(depth, w, h, 11, 2 + qp // 12), the
    lambdas, the contexts and the oracle's decision.  Returns (counts, offset_orgs, ctus_w, ctus_h, lam, ctx_m, ctx_t, bits, eparams, enos)."""
    from test_oracle_classes_vs_reference import sao_rdo_case, pad_any
    O = _oracle()
    tabs = HT.load()
    src, rec = sao_rdo_case(depth, width, height, 11, 2 + qp // 12)
    ctus_w, ctus_h = (width + 63) // 64, (height + 63) // 64
    nctu = ctus_w * ctus_h
    counts, orgs = [], []
    for pl in range(planes):
        fp, st, og = pad_any(src[pl], margin=64)
        rp = pad_any(rec[pl], margin=64)[0]
        h, w = src[pl].shape
        c, o = O.sao_stats(depth, fp, rp, st, og, w, h, ctu=(64, 64) if pl == 0 else (32, 32), plane_offset=0 if pl == 0 else 2)
        assert c.shape[0] == nctu
        counts.append(c); orgs.append(o)
    rng = np.random.default_rng([41, depth, width, height, qp])
    ctu_qp = np.clip(qp + rng.integers(-3, 4, size=nctu), 0, 51) if per_ctu else np.full(nctu, qp)
    lam = np.array([HT.sao_lambdas(tabs, int(q), csp400=planes == 1) for q in ctu_qp], dtype=np.int64)
    ctx_m, ctx_t = HT.sao_contexts(slice_type, qp)
    flag = (1, 1 if planes == 3 else 0)
    eparams, enos = O.sao_rdo(depth, counts, orgs, ctus_w, ctus_h, lam, ctx_m, ctx_t, tabs["entropy_bits"], sao_flag=flag)
    return counts, orgs, ctus_w, ctus_h, lam, ctx_m, ctx_t, tabs["entropy_bits"], eparams, enos


def merge_census(eparams, ctus_w, ctus_h):
    """(merge-left, merge-up, off) CTUs of the oracle's luma parameters."""
    y = eparams[0]
    return int((y[:, 6] == 1).sum()), int((y[:, 6] == 2).sum()), int((y[:, 0] < 0).sum())


def assert_walk_is_exercised(eparams, ctus_w, ctus_h):
    left, up, off = merge_census(eparams, ctus_w, ctus_h)
    if ctus_w >= 2:
        assert left >= 1, "the oracle's luma parameters hold no merge-left: the case does not exercise the merge lanes"
    if ctus_h >= 2:
        assert up >= 1, "the oracle's luma parameters hold no merge-up: the case does not exercise the merge lanes"
    if ctus_w >= 2 and ctus_h >= 2 and ctus_w * ctus_h >= 24:
        assert off >= 1, "the oracle leaves no CTU without SAO"
    if ctus_w == 1:
        assert left == 0
    if ctus_h == 1:
        assert up == 0


# Tall two-column strips: 44 and 50 CTU rows take four wavefronts of merge lanes where 4K takes three (a lane per row and candidate set,
# five sets per row); 4352 rows of samples (68 CTU rows, two wavefronts of decision lanes) are in tests/test_gpu_sao.py.  44 rows is also
# where two staged anti-diagonals of per-CTU records that carry the merge candidates' statistics (1632 bytes) would stop fitting the 150 KB of
# LDS the launch asks for - 44 * (2 * 1632 + 128 + 96) = 153472 <= 153600 < 45 * 3488 - a variant that was measured and not kept
# (profiles/r07_sao_stage.txt); the cases on both sides of it stay.
WALK_CASES = [
    # depth, width, height, slice_type (0 B, 1 P, 2 I), qp, planes, per-CTU lambdas
    (8, 64, 64, 1, 27, 3, False),            # one CTU
    (8, 768, 64, 1, 27, 3, False),           # one CTU row: merge-left only
    (8, 64, 768, 1, 27, 3, False),           # one CTU column: merge-up only
    (8, 128, 768, 1, 27, 3, False),          # two columns
    (8, 128, 2816, 1, 27, 3, False),         # 2 x 44
    (8, 128, 3200, 1, 27, 3, False),         # 2 x 50
    (8, 1920, 1080, 1, 30, 3, False),
    (8, 3840, 2160, 1, 27, 3, False),
    (8, 128, 768, 1, 27, 1, False),          # luma only
    (8, 1920, 1080, 1, 30, 1, False),
    (8, 128, 768, 1, 27, 3, True),           # per-CTU lambdas
    (8, 1920, 1080, 1, 30, 3, True),
    (8, 128, 768, 0, 27, 3, False),          # B
    (8, 128, 768, 2, 27, 3, False),          # I
    (8, 1920, 1080, 0, 30, 3, False),
    (8, 1920, 1080, 2, 30, 3, False),
]


@pytest.mark.parametrize("depth,width,height,slice_type,qp,planes,per_ctu", WALK_CASES)
def test_sao_rdo_walk_matches_oracle_where_it_merges(depth, width, height, slice_type, qp, planes, per_ctu):
    import torch
    dev = torch.device("cuda:0")
    counts, orgs, ctus_w, ctus_h, lam, ctx_m, ctx_t, bits, eparams, enos = walk_case(depth, width, height, slice_type, qp, planes, per_ctu)
    nctu = ctus_w * ctus_h
    print(f"{width}x{height} ({ctus_w} x {ctus_h} CTUs): merge-left / merge-up / off in luma = {merge_census(eparams, ctus_w, ctus_h)}")
    assert_walk_is_exercised(eparams, ctus_w, ctus_h)
    d_cnt = [torch.from_numpy(c.reshape(-1)).to(dev) for c in counts]
    d_org = [torch.from_numpy(o.reshape(-1)).to(dev) for o in orgs]
    d_par = [torch.full((nctu * 7,), 0x5a5a5a5a, dtype=torch.int32, device=dev) for _ in range(planes)]
    scratch = torch.zeros(H.sao_rdo_scratch_bytes(ctus_w, ctus_h), dtype=torch.uint8, device=dev)
    nos = torch.full((2,), -1, dtype=torch.int32, device=dev)
    H.sao_rdo(depth, d_cnt, d_org, ctus_w, ctus_h, lam[0], ctx_m, ctx_t, bits, d_par, scratch,
              lambda_ctu=torch.from_numpy(lam).to(dev) if per_ctu else None, sao_flag=(1, 1 if planes == 3 else 0), num_no_sao=nos)
    torch.cuda.synchronize()
    for pl in range(planes):
        got = d_par[pl].cpu().numpy().reshape(nctu, 7)
        bad = np.argwhere((got != eparams[pl]).any(axis=1))[:5].reshape(-1).tolist()
        assert np.array_equal(got, eparams[pl]), f"plane {pl}: CTUs {bad}: device {got[bad].tolist()} oracle {eparams[pl][bad].tolist()}"
    gn = nos.cpu().numpy()
    assert int(gn[0]) == int(enos[0]) and (planes == 1 or int(gn[1]) == int(enos[1]))


def _stats_pair(depth, width, height, seed):
    from test_oracle_classes_vs_reference import sao_case, pad_any
    y, rec, _ = sao_case(depth, width, height, seed)
    fp, st, og = pad_any(y, margin=64)
    rp = pad_any(rec, margin=64)[0]
    return fp, rp, st, og


STATS_CASES = [
    # depth, width, height, footprint, plane_offset
    (8, 256, 128, (64, 64), 0), (8, 200, 150, (64, 64), 0), (8, 70, 66, (64, 64), 0), (10, 200, 150, (64, 64), 0), (12, 200, 150, (64, 64), 0),
    (8, 128, 64, (32, 32), 2), (8, 100, 75, (32, 32), 2), (8, 35, 33, (32, 32), 2), (10, 100, 75, (32, 32), 2), (12, 100, 75, (32, 32), 2),
    (8, 960, 540, (32, 32), 2),
    (8, 200, 150, (16, 16), 0), (10, 200, 150, (16, 16), 0), (8, 200, 150, (32, 32), 0), (12, 70, 66, (32, 32), 0),
    (8, 200, 150, (8, 8), 0), (8, 200, 150, (64, 32), 0), (8, 200, 150, (32, 64), 1),
]


@pytest.mark.parametrize("depth,width,height,ctu,plane_offset", STATS_CASES)
def test_sao_stats_footprints_match_oracle(depth, width, height, ctu, plane_offset):
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    fp, rp, st, og = _stats_pair(depth, width, height, 13)
    cnt, off = O.sao_stats(depth, fp, rp, st, og, width, height, ctu=ctu, plane_offset=plane_offset)
    nctu = cnt.shape[0]
    d_f = torch.from_numpy(fp.view(np.uint8)).to(dev)
    d_r = torch.from_numpy(rp.view(np.uint8)).to(dev)
    d_cnt = torch.full((nctu * 160,), -1, dtype=torch.int32, device=dev)
    d_off = torch.full((nctu * 160,), -1, dtype=torch.int32, device=dev)
    H.sao_stats(depth, d_f, st, og, d_r, st, og, width, height, d_cnt, d_off, ctu=ctu, plane_offset=plane_offset)
    torch.cuda.synchronize()
    gc, go = d_cnt.cpu().numpy().reshape(cnt.shape), d_off.cpu().numpy().reshape(off.shape)
    assert np.array_equal(gc, cnt), f"count differs in CTU/type {np.argwhere((gc != cnt).any(axis=2))[:6].tolist()}"
    assert np.array_equal(go, off), f"offsetOrg differs in CTU/type {np.argwhere((go != off).any(axis=2))[:6].tolist()}"
    assert cnt[:, :4, :5].sum() > 0 and cnt[:, 4].sum() > 0 and (off[:, :4, 0] != 0).any()


@pytest.mark.parametrize("depth,width,height", [(8, 200, 152), (10, 200, 152), (12, 136, 72), (8, 1920, 1080)])
def test_sao_three_plane_launch_equals_single_plane_entry_and_oracle(depth, width, height):
    """x265hip_sao_planes without application records (the statistics launch of the frame step: Y 64x64 next to Cb, Cr 32x32) gives the
    counts of x265hip_sao_stats plane by plane, and both give the oracle's."""
    import torch
    dev = torch.device("cuda:0")
    O = _oracle()
    S = importlib.import_module("x265-yuuki-asuna_amd.stages")
    geo = [(width, height, (64, 64), 0), (width // 2, height // 2, (32, 32), 2), (width // 2, height // 2, (32, 32), 2)]
    fused, keep = [], []
    for i, (w, h, ctu, po) in enumerate(geo):
        fp, rp, st, og = _stats_pair(depth, w, h, 17 + i)
        cnt, off = O.sao_stats(depth, fp, rp, st, og, w, h, ctu=ctu, plane_offset=po)
        d_f = torch.from_numpy(fp.view(np.uint8)).to(dev)
        d_r = torch.from_numpy(rp.view(np.uint8)).to(dev)
        if depth > 8:
            d_f, d_r = d_f.view(torch.int16), d_r.view(torch.int16)
        a, b = S.Sao(w, h, depth, dev, ctu=ctu, plane_offset=po), S.Sao(w, h, depth, dev, ctu=ctu, plane_offset=po)
        a.count.fill_(-1); a.offset_org.fill_(-1); b.count.fill_(-1); b.offset_org.fill_(-1)
        fused.append(dict(a.plane(d_f, st, og, d_r, st, og, d_r.clone()), out=None))
        b.stats(None, d_r, st, og, src_plane=d_f)
        keep.append((a, b, cnt, off))
    H.sao_planes(depth, fused)
    torch.cuda.synchronize()
    for i, (a, b, cnt, off) in enumerate(keep):
        assert torch.equal(a.count, b.count) and torch.equal(a.offset_org, b.offset_org), f"plane {i}: three-plane launch != single-plane entry"
        assert np.array_equal(a.count.cpu().numpy().reshape(cnt.shape), cnt) and np.array_equal(a.offset_org.cpu().numpy().reshape(off.shape), off), f"plane {i}: != oracle"
