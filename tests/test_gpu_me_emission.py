"""GPU parity of the search kernel's row-emission flags (me_ctu_q2_kernel flags 4096 ROWLDS and 8192 OFFCHAIN, both part of the default set) against the oracle's
full search; all 85 minima of every CTU compared bit for bit.

ROWLDS takes a row's `costY[m] << 8 | m` from the table in LDS with wave-uniform reads, a pair of rows at a time two rows ahead (the pair of rows 6 / 7 is the NEXT
block's rows 0 / 1), and a block fetches its own per-lane 64x64 constants.  What can go wrong: a row with its neighbour's constant (the first block completes only
m = 0 and clamps the entries before it; the 2 / 4 / 6-row tails end the chain), so the synthetic clip runs with a motion-vector cost (lambda 4).
OFFCHAIN hands the LDS address of a block of 8 window rows on from block to block and adds the next block's skew from a per-lane constant of four bytes indexed
by the block number: a lane meets all four skews, and the index wraps, within four blocks.  What can go wrong is a block read from the wrong bytes: uniform noise
with zero motion-vector cost makes every candidate row a possible winner (asserted on the oracle's output: some PU's best vector lies in the last candidate
rows), a flat pair leaves raster order alone to decide.
Ranges: +-1 .. +-8 and +-55 .. +-58 (every tail length of the walk, T = 2 R + 8, T mod 8 = 0, 2, 4, 6, small and at the workload's size; +-1 .. +-3: the first
block is the last full one), +-12, +-14, +-17 (4 - 5 blocks: every skew phase and the wrap); +-17 and up also deal a CTU's column groups over several workgroups."""
import ctypes
import functools
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

pkg = importlib.import_module("x265-yuuki-asuna_amd")
F = importlib.import_module("x265-yuuki-asuna_amd.frames")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")
A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")


def _oracle():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import oracle_api
    return oracle_api


def _size(rng):
    return (192, 128) if rng >= 55 else (128, 64)


CONTENT = {"clip": 4.0, "noise": 0.0, "flat": 0.0}          # content -> lambda of the motion-vector cost (0: every tie decided by raster order alone)


@functools.lru_cache(maxsize=None)
def _case(rng, content):
    """(luma of the current picture, luma of the reference, cost table, the oracle's minima): computed once per case, shared by every flag set, never written to."""
    width, height = _size(rng)
    clip = F.synth_clip(width, height, 2, depth=8, seed=70 + rng)
    y0, y1 = clip[0][0], clip[1][0]
    if content == "flat":
        y0 = np.zeros_like(y0); y1 = np.full_like(y1, 255)
    if content == "noise":
        r = np.random.default_rng(23)
        y0 = r.integers(0, 256, y0.shape).astype(y0.dtype); y1 = r.integers(0, 256, y1.shape).astype(y1.dtype)
    cb, cstride, corg, w64, h64 = F.pad_plane(y1)
    rb, rstride, rorg, _, _ = F.pad_plane(y0)
    cost = F.mv_cost_table(rng, CONTENT[content])
    nctu = (w64 // 64) * (h64 // 64)
    _, best = _oracle().me_fullsearch(8, cb, cstride, corg, rb, rstride, rorg, w64, h64, rng, 0, nctu, cost, cost, want_surf=False, want_best=True)
    best.setflags(write=False)
    if content == "noise":
        nc = 2 * rng + 1
        row = (best & np.uint64(0xffffffff)).astype(np.int64) // nc
        assert np.any(row >= max(2 * rng - 6, 0)), "noise case: no PU's best vector lies in candidate rows 2 R - 6 .. 2 R (pick another seed)"
    return y1, y0, cost, best


def _kernel_name(rng):
    f = A.lib().x265hip_me_minima_kernel_name
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.c_int] * 2
    return f(8, rng).decode()


def _search(rng, content, centres=None):
    import torch
    dev = torch.device("cuda:0")
    y1, y0, cost, _ = _case(rng, content)
    cur, ref = P.DevicePicture(y1, dev), P.DevicePicture(y0, dev)
    ms = P.MotionSearch(cur.w64, cur.h64, rng, 8, dev, want_surf=False, lam=CONTENT[content])
    assert np.array_equal(ms.cost_host, cost)
    ms.run(cur, ref, centres=None if centres is None else torch.from_numpy(centres).to(dev))
    torch.cuda.synchronize()
    return cur, ref, ms, ms.best.cpu().numpy().view(np.uint64)


def _select(variant, monkeypatch, rng):
    monkeypatch.delenv("X265HIP_ME_BEST_VARIANT", raising=False)
    monkeypatch.delenv("X265HIP_ME_Q2_FLAGS", raising=False)
    if variant:
        monkeypatch.setenv("X265HIP_ME_Q2_FLAGS", variant[1:])
    A.lib().x265hip_me_env_refresh()          # the switches are read once per process (tests/conftest.py re-reads them after every test)
    name = _kernel_name(rng)
    want = f"me_ctu_q2_kernel<256,{variant[1:]}>" if variant else "me_ctu_q2_kernel<256,"
    if not name.startswith(want):
        pytest.skip(f"+-{rng}: the minima-only launch is answered by {name}, not by {want}")


RANGES = [1, 2, 3, 4, 5, 6, 7, 8, 12, 14, 17, 55, 56, 57, 58]
VARIANTS = ["", "q1278", "q5374", "q9470"]          # the library's default (1278 | ROWLDS | OFFCHAIN), the set it extends, ROWLDS alone, OFFCHAIN alone


def test_default_holds_both_flags(monkeypatch):
    """The default of the 8-bit minima-only launch is 1278 | 4096 | 8192 (so "" below is the case of both flags together)."""
    _select("", monkeypatch, 57)
    assert _kernel_name(57) == "me_ctu_q2_kernel<256,13566>"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("content", list(CONTENT))
@pytest.mark.parametrize("rng", RANGES)
def test_me_minima_emission_flags(rng, content, variant, monkeypatch):
    _select(variant, monkeypatch, rng)
    _, _, _, gb = _search(rng, content)
    best = _case(rng, content)[3]
    assert np.array_equal(gb, best), f"variant {variant!r} +-{rng} {content}: {np.count_nonzero(gb != best)} of {gb.size} minima differ"


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("content", ["clip", "noise"])
def test_me_minima_emission_one_workgroup_per_ctu(content, variant, monkeypatch):
    """+-57 with X265HIP_ME_SPLIT_GROUPS=0: one workgroup walks all 29 column groups of a CTU, as a whole-picture launch does (a small picture otherwise deals
    a CTU's column groups over several workgroups: the cases above)."""
    monkeypatch.setenv("X265HIP_ME_SPLIT_GROUPS", "0")
    _select(variant, monkeypatch, 57)
    _, _, _, gb = _search(57, content)
    best = _case(57, content)[3]
    assert np.array_equal(gb, best), f"variant {variant!r} {content}: {np.count_nonzero(gb != best)} of {gb.size} minima differ"


@pytest.mark.parametrize("variant", VARIANTS)
def test_me_minima_emission_windows_centred_per_ctu(variant, monkeypatch):
    """Per-CTU search centres (+-7, T mod 8 = 6): each CTU against the oracle's search of its own window."""
    rng = 7
    _select(variant, monkeypatch, rng)
    y1 = _case(rng, "clip")[0]
    nctu = (y1.shape[1] // 64) * (y1.shape[0] // 64)
    cen = np.random.default_rng(5).integers(-20, 21, size=(nctu, 2)).astype(np.int16)
    cur, ref, ms, gb = _search(rng, "clip", centres=cen)
    gb = gb.reshape(ms.nctu, 85)
    O = _oracle()
    cw = cur.w64 // 64
    for c in range(ms.nctu):
        o = cur.org + (c // cw) * 64 * cur.stride + (c % cw) * 64
        _, best = O.me_fullsearch(8, cur.host, cur.stride, o, ref.host, ref.stride, o + int(cen[c, 1]) * ref.stride + int(cen[c, 0]), 64, 64, rng, 0, 1,
                                  ms.cost_host, ms.cost_host, want_surf=False, want_best=True)
        assert np.array_equal(gb[c], best.reshape(-1)), (c, variant)
