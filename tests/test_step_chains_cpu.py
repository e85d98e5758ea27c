"""The pin of the oracle chains the GPU step tests compare against: every chain of the *_expect.py modules on a 128x128 picture (four
CTUs: SAO merge-left and merge-up exist, the per-CTU lambda is tiled, deblocking meets a CTU edge in both directions), each output
dictionary reduced to one SHA-256 and compared with tests/golden/step_chains.json.  The digests were recorded from the chains as they
stood BEFORE they shared tests/step_chain.py (python tests/test_step_chains_cpu.py --record on that commit), so a chain that computes
anything else since then fails here, without a GPU.  The inputs do not go through the code under the pin: the SAO record is built here
from host_tables (tests/test_step_chain_cpu.py holds step_chain.sao_rdo_inputs against it).  Needs the plain-C oracle only."""
import functools
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)                    # under pytest, conftest.py has done this

import bidir_expect as BE                       # noqa: E402
import bmerge_expect as BM                      # noqa: E402
import bref_expect as BR                        # noqa: E402
import bsa8d_expect as BX                       # noqa: E402
import intra_expect as IE                       # noqa: E402
import intra_inter_expect as IX                 # noqa: E402
import merge_expect as ME                       # noqa: E402
import multiref_expect as MR                    # noqa: E402
import qp_map_expect as QE                      # noqa: E402
import subpel_chroma_expect as CE               # noqa: E402

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_chains.json")
W = H = 128
R = 6
SEED = 9
DEPTHS, LEVELS = (8, 10), (0, 2)
RDO, DECIDE, NOSAO, MAPS, PLAIN = "rdo", "decide", "nosao", "maps", "plain"


def _qp(depth):
    return 30 + 6 * (depth - 8)


def _record(depth, slice_type):
    """What a step takes as sao_rdo at the pinned QP, from the host tables themselves."""
    tabs = HT.load()
    cu_qp = max(_qp(depth) - 6 * (depth - 8), 0)
    cm, ct = HT.sao_contexts(slice_type, cu_qp)
    return {"lambdas": HT.sao_lambdas(tabs, cu_qp), "ctx_merge": cm, "ctx_type": ct, "entropy_bits": tabs["entropy_bits"]}


@functools.lru_cache(maxsize=None)
def _planes(depth):
    """the four pictures' padded (Y, Cb, Cr) host planes: shared, read only"""
    hp = []
    for yuv in F.synth_clip(W, H, 4, depth=depth, seed=SEED):
        planes, w64, h64 = BE.padded_planes(yuv)
        assert (w64, h64) == (W, H)
        hp.append(planes)
    return hp


@functools.lru_cache(maxsize=None)
def _maps(depth, level):
    """(cu_qp int8 [16, 16], tu_qp int8 [3, 16, 16]): one of four quantiser QPs per block, dealt differently on each plane."""
    values = _qp(depth) + np.array([-5, -2, 0, 4])
    nblocks = 4 * (64 >> (2 * level))
    r = np.random.default_rng([17, depth, level])
    tu = np.stack([QE.cells_of_blocks(values[r.integers(0, 4, nblocks)], W, H, level) for _ in range(3)])
    cu = np.clip(tu[0].astype(np.int64) - 6 * (depth - 8), 0, 51).astype(np.int8)
    assert len(np.unique(cu)) >= 3 and all(len(np.unique(t)) >= 3 for t in tu)
    return cu, tu


def _chains():
    """name -> (slice type of its SAO record, the variants it takes, call(depth, level, hp, **keywords of the variant))"""
    q = _qp
    P, B, I = HT.SLICE_P, HT.SLICE_B, HT.SLICE_I
    sao, maps, refs = (RDO, DECIDE), (RDO, DECIDE, MAPS), (RDO, DECIDE, NOSAO, MAPS)
    return {
        "bidir.b_chain": (B, sao, lambda d, l, hp, **kw: BE.b_chain(d, hp[1], hp[0], hp[2], W, H, R, 2, l, q(d), **kw)),
        "intra.i_chain": (I, sao, lambda d, l, hp, **kw: IE.i_chain(d, hp[0], W, H, l, q(d), **kw)),
        "intra_inter.p_chain": (P, sao, lambda d, l, hp, **kw: IX.p_chain(d, hp[1], hp[0], W, H, R, 2, l, q(d), **kw)),
        "merge.p_chain": (P, maps, lambda d, l, hp, **kw: ME.p_chain(d, hp[1], hp[0], W, H, R, 2, l, q(d), **kw)),
        "bsa8d.sa8d_b_chain[intra]": (B, sao, lambda d, l, hp, **kw: BX.sa8d_b_chain(d, hp[1], hp[0], hp[2], W, H, R, 2, l, q(d), True, **kw)),
        "bsa8d.sa8d_b_chain[inter]": (B, sao, lambda d, l, hp, **kw: BX.sa8d_b_chain(d, hp[1], hp[0], hp[2], W, H, R, 2, l, q(d), False, **kw)),
        "bmerge.merge_b_chain": (B, maps, lambda d, l, hp, **kw: BM.merge_b_chain(d, hp[1], hp[0], hp[2], W, H, R, 2, l, q(d), **kw)),
        "multiref.p_chain_refs": (P, refs, lambda d, l, hp, **kw: MR.p_chain_refs(d, hp[3], [hp[2], hp[1], hp[0]], W, H, R, 2, l, q(d), **kw)),
        "bref.b_chain_refs": (B, refs, lambda d, l, hp, **kw: BR.b_chain_refs(d, hp[2], [hp[1], hp[0]], [hp[3], hp[1]], W, H, R, 2, l, q(d), **kw)),
        "qp_map.p_chain": (None, (MAPS,), lambda d, l, hp, cu_qp, tu_qp: QE.p_chain(d, hp[1], hp[0], W, H, R, 2, l, q(d), cu_qp, tu_qp)),
        "qp_map.b_chain": (None, (MAPS,), lambda d, l, hp, cu_qp, tu_qp: QE.b_chain(d, hp[1], hp[0], hp[2], W, H, R, 2, l, q(d), cu_qp, tu_qp)),
        "qp_map.i_chain": (None, (MAPS,), lambda d, l, hp, cu_qp, tu_qp: QE.i_chain(d, hp[0], W, H, l, q(d), cu_qp, tu_qp, lambda8_by_qp=QE.lambda8_table(d))),
        "subpel_chroma.p_chain[chroma_satd]": (None, (PLAIN,), lambda d, l, hp: CE.p_chain(d, hp[1], hp[0], W, H, R, 3, l, q(d), True)),
        "subpel_chroma.p_chain[luma]": (None, (PLAIN,), lambda d, l, hp: CE.p_chain(d, hp[1], hp[0], W, H, R, 3, l, q(d), False)),
        "subpel_chroma.b_chain": (None, (PLAIN,), lambda d, l, hp: CE.b_chain(d, [hp[0], hp[1], hp[2]], W, H, R, 3, l, q(d))),
    }


CASES = [(name, variant, depth, level) for name, (_, variants, _) in _chains().items() for variant in variants for depth in DEPTHS for level in LEVELS]


def _id(case):
    return "%s-%s-d%d-l%d" % case


@functools.lru_cache(maxsize=None)
def _run(name, variant, depth, level):
    """The chain's dictionary: shared between its own case and the conditions, read only."""
    slice_type, _, call = _chains()[name]
    kw = {}
    if variant in (RDO, MAPS) and slice_type is not None:
        kw["sao_rdo"] = _record(depth, slice_type)
    if variant == NOSAO:
        kw["sao"] = False
    if variant == MAPS:
        kw["cu_qp"], kw["tu_qp"] = _maps(depth, level)
        if name in ("merge.p_chain", "bmerge.merge_b_chain"):
            kw["lambda8_by_qp"] = QE.lambda8_table(depth)
    return call(depth, level, _planes(depth), **kw)


def _arrays(out, prefix=""):
    for name, v in out.items():
        if isinstance(v, dict):
            yield from _arrays(v, prefix + name + ".")
        else:
            yield prefix + name, np.ascontiguousarray(v)


def digest(out):
    """SHA-256 over the sorted names: of every name its text, dtype, shape and bytes (a dictionary inside counts as name.key)."""
    h = hashlib.sha256()
    for name, a in sorted(_arrays(out), key=lambda t: t[0]):
        h.update(repr((name, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_chain_is_the_recorded_one(case):
    assert digest(_run(*case)) == _golden()[_id(case)]


def test_every_recorded_case_is_run():
    assert sorted(_golden()) == sorted(_id(c) for c in CASES)


@pytest.mark.parametrize("depth", DEPTHS)
def test_the_pinned_pictures_reach_every_branch_of_the_tail(depth):
    """A degenerate clip would pin nothing: over the depth's cases SAO switches on for luma and chroma, the rate-distortion decision merges
    left and up, both Bs maps have edges to filter, and blocks with and without coefficients exist."""
    luma_on = chroma_on = left = up = ver = hor = coded = empty = False
    for name, variant, d, level in CASES:
        if d != depth:
            continue
        out = _run(name, variant, d, level)
        ver, hor = ver or bool(np.any(out["bs_ver"])), hor or bool(np.any(out["bs_hor"]))
        coded, empty = coded or bool(np.any(out["num_sig"] > 0)), empty or bool(np.any(out["num_sig"] == 0))
        if "sao_params" not in out:
            continue
        rows = [np.asarray(out[k]).reshape(-1, 7) for k in ("sao_params", "sao_params_c0", "sao_params_c1")]
        luma_on, chroma_on = luma_on or bool(np.any(rows[0][:, 0] != -1)), chroma_on or bool(np.any(rows[1][:, 0] != -1) or np.any(rows[2][:, 0] != -1))
        if variant in (RDO, MAPS):
            left, up = left or any(bool(np.any(r[:, 6] == 1)) for r in rows), up or any(bool(np.any(r[:, 6] == 2)) for r in rows)
    assert luma_on and chroma_on, (luma_on, chroma_on)
    assert left and up, (left, up)
    assert ver and hor and coded and empty, (ver, hor, coded, empty)


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_step_chains_cpu.py --record"
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
        json.dump({_id(c): digest(_run(*c)) for c in CASES}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d digests in %s" % (len(CASES), GOLDEN))
