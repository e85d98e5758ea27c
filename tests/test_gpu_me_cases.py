"""GPU parity of the exhaustive search (x265hip_me_fullsearch) with mv-cost tables that fill the keys: the cases of tests/me_cases.py (which
tests/test_me_cases_cpu.py shows to tell a wrong cost handling from the right one at every PU level) through every kernel the launch table can select at
8, 10 and 12 bits - cost tables up to 65535 per component, x and y different, flat pictures whose SADs fill the accumulators, winners next to the pad columns.
The oracle is the only expectation: minima as uint64, equal means equal; surfaces, where the operating point has them, in its format."""
import ctypes
import importlib

import numpy as np
import pytest

import me_cases as MC
from test_gpu_me import _valid

pytestmark = pytest.mark.gpu

A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
P = importlib.import_module("x265-yuuki-asuna_amd.pipeline")

SWITCHES = ("X265HIP_ME_BEST_VARIANT", "X265HIP_ME_Q2_FLAGS", "X265HIP_ME_KERNEL", "X265HIP_ME_SPLIT_GROUPS", "X265HIP_ME_W2", "X265HIP_ME_GENERIC", "X265HIP_ME_SPLIT",
            "X265HIP_ME_BEST_WAVES", "X265HIP_ME_XCD_OFF", "X265HIP_ME_CAND_VARIANT")
EINVAL = -2                                   # X265HIP_EINVAL


def _kernel_name(depth, rng):
    f = A.lib().x265hip_me_minima_kernel_name
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.c_int] * 2
    return f(depth, rng).decode()


def _select(op, monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for k, v in op.env.items():
        monkeypatch.setenv(k, v)
    A.lib().x265hip_me_env_refresh()          # the switches are read once per process (tests/conftest.py re-reads them after every test)


def _stage(case, dev):
    """(current picture, reference picture, the stage with the case's own tables)."""
    import torch
    op = case.op
    src, ref = MC.pictures(op.depth, case.content, *op.size, case.rng)
    cur, rf = P.DevicePicture(src, dev), P.DevicePicture(ref, dev)
    ms = P.MotionSearch(cur.w64, cur.h64, case.rng, op.depth, dev, want_surf=op.out != "best", want_best=op.out != "surf", packed=op.packed)
    cx, cy = MC.tables(case.table, case.rng)
    ms.cost_x = torch.from_numpy(cx.view(np.int16).copy()).to(dev)
    ms.cost_y = torch.from_numpy(cy.view(np.int16).copy()).to(dev)
    ms.cost_host = None                       # two tables: nothing may take one for both
    return cur, rf, ms


def _describe_best(got, want, nc):
    """Differing PUs per level and the first differing key as (cost, raster) on both sides."""
    got, want = got.reshape(-1, 85), want.reshape(-1, 85)
    per = [int(np.count_nonzero(got[:, b:b + n] != want[:, b:b + n])) for b, n in zip(MC.LEVEL_BASE, MC.LEVEL_PUS)]
    c, pu = [int(v[0]) for v in np.nonzero(got != want)]
    g, w = int(got[c, pu]), int(want[c, pu])
    return (f"differing PUs per level {per}; first: CTU {c} PU {pu}: device (cost {g >> 32}, raster {g & 0xffffffff} = mv index ({(g & 0xffffffff) % nc}, {(g & 0xffffffff) // nc})) "
            f"oracle (cost {w >> 32}, raster {w & 0xffffffff} = mv index ({(w & 0xffffffff) % nc}, {(w & 0xffffffff) // nc}))")


def _check_surf(ms, surf, label):
    e = _valid(surf, ms)
    if ms.packed:
        for level in range(4):
            b, n = P.LEVEL_BASE[level], P.LEVEL_PUS[level]
            g = ms.level_view(level)[0].cpu().numpy()
            x = e[:, :, b:b + n].reshape(-1, n)
            assert np.array_equal(g, x), f"{label}: surface level {level} differs ({np.count_nonzero(g != x)} of {x.size})"
    else:
        g = _valid(ms.surf.cpu().numpy(), ms)
        assert np.array_equal(g, e), f"{label}: SAD surface differs ({np.count_nonzero(g != e)} of {e.size})"


@pytest.mark.parametrize("case", MC.gpu_cases(), ids=lambda c: c.id)
def test_me_case(case, monkeypatch):
    import torch
    op = case.op
    _select(op, monkeypatch)
    name = _kernel_name(op.depth, case.rng)
    if op.route is not None:
        assert name == op.route, f"{case.id}: the launch table answers +-{case.rng} at {op.depth} bits with {name}, the case is listed for {op.route}"
    label = f"{case.id} [{op.kernel}; minima-only route {name}]"
    dev = torch.device("cuda:0")
    cur, rf, ms = _stage(case, dev)
    if op.centres:
        cen = MC.centres_of(ms.nctu)
        ms.run(cur, rf, centres=torch.from_numpy(cen).to(dev))
        surf, best = MC.expected_centred(op.depth, case.content, *op.size, case.rng, case.table, cen)
    else:
        ms.run(cur, rf)
        best = MC.expected_best(*MC.data_key(case)) if ms.best is not None else None
        surf = MC.expected_surf(op.depth, case.content, *op.size, case.rng) if ms.surf is not None else None
    torch.cuda.synchronize()
    if ms.best is not None:
        gb = ms.best.cpu().numpy().view(np.uint64)
        assert np.array_equal(gb, best), f"{label}: {_describe_best(gb, best, ms.nc)}"
    if ms.surf is not None:
        _check_surf(ms, surf, label)


@pytest.mark.parametrize("depth,rng,out", MC.REFUSED)
def test_me_first_range_beyond_the_16_bit_window_is_refused_and_writes_nothing(depth, rng, out):
    """+-76 is the widest window of 16-bit samples whose row fits the 512-byte LDS pitch (the fast paths at 10 bits, the generic kernel at 12, both among the
    cases); +-77 needs 1024 bytes a row and more LDS than a workgroup has: X265HIP_EINVAL, the minima still all-ones, the surface untouched."""
    import torch
    dev = torch.device("cuda:0")
    src, ref = MC.pictures(depth, "noise", 128, 64, rng)
    cur, rf = P.DevicePicture(src, dev), P.DevicePicture(ref, dev)
    ms = P.MotionSearch(cur.w64, cur.h64, rng, depth, dev, want_surf=out != "best", want_best=out != "surf")
    if ms.surf is not None:
        ms.surf.fill_(0x5a5a5a5a)
    A.lib().x265hip_me_fullsearch.restype = ctypes.c_int
    p = A.MEParams()
    p.depth, p.width, p.height, p.range = depth, cur.w64, cur.h64, rng
    p.fenc, p.fenc_stride = cur.t.data_ptr() + cur.org * 2, cur.stride
    p.fref, p.fref_stride = rf.t.data_ptr() + rf.org * 2, rf.stride
    p.surf, p.best = (ms.surf.data_ptr() if ms.surf is not None else None), (ms.best.data_ptr() if ms.best is not None else None)
    p.cost_x, p.cost_y = ms.cost_x.data_ptr(), ms.cost_y.data_ptr()
    p.surf_format = A.SURF_I32
    ms.reset()
    torch.cuda.synchronize()
    assert A.lib().x265hip_me_fullsearch(ctypes.byref(p), None) == EINVAL, A.lib().x265hip_last_error()
    assert b"LDS" in A.lib().x265hip_last_error()
    torch.cuda.synchronize()
    if ms.best is not None:
        assert bool((ms.best == -1).all())
    if ms.surf is not None:
        assert bool((ms.surf == 0x5a5a5a5a).all())


def test_me_cases_reach_every_kernel_of_the_launch_table(monkeypatch):
    """Every name x265hip_me_minima_kernel_name can return at 8, 10 and 12 bits with the default flag set - the two 8-bit column-group kernels, the
    record-per-lane kernel, the two 16-bit column-group kernels, the generic kernel at either sample size - is the route of some case, and the routes of the cases
    are what the launch table answers at their ranges."""
    names = set()
    for op in MC.OPS:
        _select(op, monkeypatch)
        for rng in op.ranges:
            name = _kernel_name(op.depth, rng)
            assert op.route is None or name == op.route, (op.name, rng, name)
            names.add(name)
    assert names == {"me_ctu_q2_kernel<256,13566>", "me_ctu_q_kernel<best>", "me_ctu_c_kernel (record per lane)", "me_ctu_kernel<u8,best>",
                     "me_ctu_w2_kernel", "me_ctu_w_kernel<best>", "me_ctu_kernel<u16,best>"}, names
    # the limits of the fast paths, from the launch table itself: the last range of each pitch and the first beyond it
    _select(MC.OPS[0], monkeypatch)
    assert not MC.OPS[0].env
    assert _kernel_name(8, 58).startswith("me_ctu_q2_kernel") and _kernel_name(8, 59) == "me_ctu_kernel<u8,best>"
    assert _kernel_name(10, 76) == "me_ctu_w2_kernel" and _kernel_name(10, 77) == "me_ctu_kernel<u16,best>"
