"""GPU parity of the search kernel's MAD16 flag (me_ctu_q2_kernel flag 1024, part of the default set) against the oracle's full search, at every tail length of
the ring walk.

MAD16 builds the four 8x8 keys of a row from the packed accumulator halves (v_mad_u32_u16 with and without op_sel).  What can go wrong is a key built from the
wrong half, or a minimum of the LAST candidate rows of the window going missing (the file was written for MAD16 together with a cut of the ring's dead tail -
TAILCUT, flag 512, and X265HIP_ME_W2=2 - which was measured, lost and is not in the tree: profiles/me_tailcut_mad16.txt; its cases stay, they cost a few
milliseconds each and the existing tests have no range with T mod 8 = 6).  So: every tail length of the walk (T = 2 R + 8, T mod 8 = 0, 2, 4, 6) at small
ranges and at the workload's, the ranges whose first block is the last full one (+-1 .. +-3), uniform noise with zero motion-vector cost (ties, every candidate
row can win - asserted on the oracle's output: some PU's best vector lies in rows 2 R - 6 .. 2 R), a flat pair (everything ties, raster order alone decides)
and the synthetic clip; all minima compared bit for bit."""
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
    return (256, 64) if rng == 58 else ((192, 128) if rng in (4, 55, 56, 57) else (128, 64))


CONTENT = {"clip": 4.0, "noise": 0.0, "flat": 0.0}          # content -> lambda of the motion-vector cost (0: every tie decided by raster order alone)


@functools.lru_cache(maxsize=None)
def _case(depth, rng, content):
    """(luma of the current picture, luma of the reference, padded host pictures' geometry, cost table, the oracle's minima): computed once per case, shared by every
    flag set, never written to."""
    width, height = _size(rng)
    clip = F.synth_clip(width, height, 2, depth=depth, seed=40 + rng)
    y0, y1 = clip[0][0], clip[1][0]
    if content == "flat":
        y0 = np.zeros_like(y0); y1 = np.full_like(y1, (1 << depth) - 1)
    if content == "noise":
        r = np.random.default_rng(11 + depth)
        y0 = r.integers(0, 1 << depth, y0.shape).astype(y0.dtype); y1 = r.integers(0, 1 << depth, y1.shape).astype(y1.dtype)
    cb, cstride, corg, w64, h64 = F.pad_plane(y1)
    rb, rstride, rorg, _, _ = F.pad_plane(y0)
    cost = F.mv_cost_table(rng, CONTENT[content])
    nctu = (w64 // 64) * (h64 // 64)
    _, best = _oracle().me_fullsearch(depth, cb, cstride, corg, rb, rstride, rorg, w64, h64, rng, 0, nctu, cost, cost, want_surf=False, want_best=True)
    best.setflags(write=False)
    if content == "noise":
        # the case that finds a wrongly skipped slot must contain minima in the candidate rows whose slots start in the last seven window rows
        nc = 2 * rng + 1
        row = (best & np.uint64(0xffffffff)).astype(np.int64) // nc
        assert np.any(row >= max(2 * rng - 6, 0)), "noise case: no PU's best vector lies in candidate rows 2 R - 6 .. 2 R (pick another seed)"
    return y1, y0, cost, best


def _kernel_name(depth, rng):
    f = A.lib().x265hip_me_minima_kernel_name
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.c_int] * 2
    return f(depth, rng).decode()


def _search(depth, rng, content, centres=None):
    import torch
    dev = torch.device("cuda:0")
    y1, y0, cost, _ = _case(depth, rng, content)
    cur, ref = P.DevicePicture(y1, dev), P.DevicePicture(y0, dev)
    ms = P.MotionSearch(cur.w64, cur.h64, rng, depth, dev, want_surf=False, lam=CONTENT[content])
    assert np.array_equal(ms.cost_host, cost)
    ms.run(cur, ref, centres=None if centres is None else torch.from_numpy(centres).to(dev))
    torch.cuda.synchronize()
    return cur, ref, ms, ms.best.cpu().numpy().view(np.uint64)


def _select8(variant, monkeypatch, rng):
    monkeypatch.delenv("X265HIP_ME_BEST_VARIANT", raising=False)
    monkeypatch.delenv("X265HIP_ME_Q2_FLAGS", raising=False)
    if variant:
        monkeypatch.setenv("X265HIP_ME_Q2_FLAGS", variant[1:])
    A.lib().x265hip_me_env_refresh()          # the switches are read once per process (tests/conftest.py re-reads them after every test)
    name = _kernel_name(8, rng)
    want = f"me_ctu_q2_kernel<256,{variant[1:]}>" if variant else "me_ctu_q2_kernel<256,"
    if not name.startswith(want):
        pytest.skip(f"+-{rng}: the minima-only launch is answered by {name}, not by {want}")


RANGES8 = [1, 2, 3, 4, 5, 6, 7, 8, 55, 56, 57, 58]
VARIANTS8 = ["", "q1278", "q254"]


@pytest.mark.parametrize("variant", VARIANTS8)
@pytest.mark.parametrize("content", list(CONTENT))
@pytest.mark.parametrize("rng", RANGES8)
def test_me_minima_8bit_mad16_every_tail_length(rng, content, variant, monkeypatch):
    """The library's default, the new flag set and the one it extends (qN = X265HIP_ME_Q2_FLAGS): +-1 .. +-3 (the first block is the last full block), +-4 (one steady
    block), +-5 .. +-8 and +-55 .. +-58 (T mod 8 = 2, 4, 6, 0 / 6, 0, 2, 4: every tail length, small and at the workload's size)."""
    _select8(variant, monkeypatch, rng)
    _, _, _, gb = _search(8, rng, content)
    best = _case(8, rng, content)[3]
    assert np.array_equal(gb, best), f"variant {variant!r} +-{rng} {content}: {np.count_nonzero(gb != best)} of {gb.size} minima differ"


@pytest.mark.parametrize("variant", VARIANTS8)
def test_me_minima_8bit_mad16_one_workgroup_per_ctu(variant, monkeypatch):
    """+-57 with X265HIP_ME_SPLIT_GROUPS=0: one workgroup walks all 29 column groups of a CTU, as a whole-picture launch does (a small picture otherwise deals
    a CTU's column groups over several workgroups)."""
    monkeypatch.setenv("X265HIP_ME_SPLIT_GROUPS", "0")
    _select8(variant, monkeypatch, 57)
    _, _, _, gb = _search(8, 57, "noise")
    best = _case(8, 57, "noise")[3]
    assert np.array_equal(gb, best), f"variant {variant!r}: {np.count_nonzero(gb != best)} of {gb.size} minima differ"


@pytest.mark.parametrize("variant", VARIANTS8)
def test_me_minima_8bit_mad16_windows_centred_per_ctu(variant, monkeypatch):
    """Per-CTU search centres (+-7, T mod 8 = 6): each CTU against the oracle's search of its own window."""
    rng = 7
    _select8(variant, monkeypatch, rng)
    y1 = _case(8, rng, "clip")[0]
    nctu = (y1.shape[1] // 64) * (y1.shape[0] // 64)
    cen = np.random.default_rng(5).integers(-20, 21, size=(nctu, 2)).astype(np.int16)
    cur, ref, ms, gb = _search(8, rng, "clip", centres=cen)
    gb = gb.reshape(ms.nctu, 85)
    O = _oracle()
    cw = cur.w64 // 64
    for c in range(ms.nctu):
        o = cur.org + (c // cw) * 64 * cur.stride + (c % cw) * 64
        _, best = O.me_fullsearch(8, cur.host, cur.stride, o, ref.host, ref.stride, o + int(cen[c, 1]) * ref.stride + int(cen[c, 0]), 64, 64, rng, 0, 1,
                                  ms.cost_host, ms.cost_host, want_surf=False, want_best=True)
        assert np.array_equal(gb[c], best.reshape(-1)), (c, variant)


@pytest.mark.parametrize("w2", ["1"])
@pytest.mark.parametrize("content", list(CONTENT))
@pytest.mark.parametrize("rng", [5, 6, 7, 8, 55, 57])
def test_me_minima_10bit_every_tail_length(rng, content, w2, monkeypatch):
    """The 16-bit twin (X265HIP_ME_W2 = 1; its code is unchanged): +-5 .. +-8 (256-byte LDS pitch) and +-55 / +-57 (512 bytes), every tail length."""
    monkeypatch.delenv("X265HIP_ME_BEST_VARIANT", raising=False)
    monkeypatch.setenv("X265HIP_ME_W2", w2)
    A.lib().x265hip_me_env_refresh()
    name = _kernel_name(10, rng)
    want = "me_ctu_w2_kernel"
    if name != want:
        pytest.skip(f"+-{rng}: the minima-only launch is answered by {name}, not by {want}")
    _, _, _, gb = _search(10, rng, content)
    best = _case(10, rng, content)[3]
    assert np.array_equal(gb, best), f"X265HIP_ME_W2={w2} +-{rng} {content}: {np.count_nonzero(gb != best)} of {gb.size} minima differ"
