"""GPU parity of the 8-bit luma phase-plane kernels (csrc/phase_kernels.hip: the fixed-depth kernel that 8-bit luma takes by default, and the two older
kernels X265HIP_PHASE_KERNEL=1 / 2 select) against the oracle.

The oracle filters whole 8 x 8 blocks of planes whose row count is a multiple of 8, the product accepts any multiple of 4 from 16 rows on.  The filters are
position invariant, so a run over R rows is checked as a BAND of a taller plane: the product gets the plane from line BAND0 on and R rows, produces the band's
lines [4, R - 8) = the plane's lines [BAND0 + 4, BAND0 + R - 8), and EVERY one of them is compared with the oracle's plane, columns [8, stride - 8) (the
oracle leaves an 8-sample border undefined, the product's first and last tiles of a row read their neighbours' bytes)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_ROWS, BAND0 = 40, 4             # the tallest band, 28 rows, produces the plane's lines [8, 24): inside the oracle's [8, 32)

# luma taps (constants.cpp:250-259), index = quarter-sample phase; phase 0 is the copy
TAPS = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]])


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle_api
    return oracle_api


def _run_band(plane, rows, dst_shift=0):
    """The product on `rows` rows of `plane` [PLANE_ROWS, stride] from line BAND0 on -> [15, rows, stride]; dst_shift moves the destination off its 16-byte
    alignment."""
    import torch
    A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
    dev = torch.device("cuda:0")
    stride = plane.shape[1]
    d_src = torch.from_numpy(plane.reshape(-1).copy()).to(dev)
    d_dst = torch.zeros(dst_shift + 15 * rows * stride, dtype=torch.uint8, device=dev)
    assert d_dst.data_ptr() % 16 == 0
    A.phase_planes(8, d_src, BAND0 * stride, d_dst[dst_shift:], stride, rows)
    torch.cuda.synchronize()
    return d_dst[dst_shift:].cpu().numpy().reshape(15, rows, stride)


def _check(plane, rows, want=None, dst_shift=0):
    got = _run_band(plane, rows, dst_shift)
    if want is None:
        want = _oracle().phase_planes(8, plane, plane.shape[1], PLANE_ROWS)
    for ph in range(15):
        g, e = got[ph, 4:rows - 8, 8:-8], want[ph, BAND0 + 4:BAND0 + rows - 8, 8:-8]
        assert g.shape == e.shape and g.size == (rows - 12) * (plane.shape[1] - 16)
        assert np.array_equal(g, e), f"rows {rows} stride {plane.shape[1]} phase {ph + 1}: {np.count_nonzero(g != e)} of {g.size} samples differ"
    return got


def _random_plane(stride, seed):
    """Full-range noise with runs of 0 and 255 mixed in (rounding and both clips)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (PLANE_ROWS, stride), dtype=np.uint8)
    p[:, stride // 3:stride // 3 + 11] = 255
    p[9:14, :] = np.where(rng.integers(0, 2, (5, stride)) > 0, 255, 0)
    return p


_shared = {}


def _shared_case(tiles_w):
    """One plane and one oracle run per width, shared by the row counts; never modified."""
    if tiles_w not in _shared:
        p = _random_plane(4 * tiles_w, 500 + tiles_w)
        want = _oracle().phase_planes(8, p, 4 * tiles_w, PLANE_ROWS)
        p.setflags(write=False); want.setflags(write=False)
        _shared[tiles_w] = (p, want)
    return _shared[tiles_w]


# 18 tiles: not a multiple of 4 and a 72-byte pitch (narrow stores); 64: whole quads below one workgroup; 260: a second, partly empty workgroup in x
@pytest.mark.parametrize("tiles_w", [18, 64, 260])
# 1, 2, 3, 4 produced tile rows (for a kernel with 4x8 tiles: the remainder alone, one full tile, full + remainder, two full)
@pytest.mark.parametrize("rows", [16, 20, 24, 28])
def test_rows_and_widths(rows, tiles_w):
    plane, want = _shared_case(tiles_w)
    _check(plane, rows, want)


@pytest.mark.parametrize("rows", [20, 24])
def test_destination_off_16_bytes(rows):
    """Whole quads per row, but the destination (and so every plane and line of it) sits 4 bytes off a 16-byte boundary."""
    plane, want = _shared_case(64)
    _check(plane, rows, want, dst_shift=4)


@pytest.mark.parametrize("value", [0, 255])
def test_flat_planes(value):
    plane = np.full((PLANE_ROWS, 256), value, np.uint8)
    got = _check(plane, 24)
    assert np.all(got[:, 4:16, 8:-8] == value)           # the taps of every phase sum to 64


def test_random_plane():
    _check(_random_plane(256, 7), 24)


STAMP_LINE, STAMP_X0, STAMP_STEP = 12, 16, 16            # output line of every stamp's centre (source rows 9 .. 16, inside the 24-row band's 4 .. 27)


def _stamp_plane():
    """For every phase an 8x8 stamp with 255 where the product of the horizontal and the vertical tap is positive and 0 elsewhere, and its inverse, 16 columns
    apart on a zero plane.  The sample whose filter window is the stamp takes the largest (inverse: the smallest) sum the phase can produce."""
    plane = np.zeros((PLANE_ROWS, 4 * 132), np.uint8)
    where = {}
    for ph in range(1, 16):
        xf, yf = ph & 3, ph >> 2
        pos = np.outer(TAPS[yf], TAPS[xf]) > 0
        for inv in (0, 1):
            x = STAMP_X0 + STAMP_STEP * (2 * (ph - 1) + inv)
            plane[STAMP_LINE - 3:STAMP_LINE + 5, x:x + 8] = np.where(pos != bool(inv), 255, 0)
            where[ph, inv] = (STAMP_LINE, x + 3)
    return plane, where


def _unclipped(plane, y, x, xf, yf):
    """The two-stage sample before its clip, stage by stage (ipfilter.cpp:120-162 luma_hps at 8 bits, :241-282 luma_vsp)."""
    win = plane[y - 3:y + 5, x - 3:x + 5].astype(np.int64)
    inter = win @ TAPS[xf] - 8192
    assert inter.min() >= -14312 and inter.max() <= 14248
    return (int(TAPS[yf] @ inter) + 2048 + (8192 << 6)) >> 12, inter


def test_stamps_reach_the_range_ends():
    plane, where = _stamp_plane()
    want = _oracle().phase_planes(8, plane, plane.shape[1], PLANE_ROWS)
    # precondition, on the CPU alone: in every two-stage phase the stamp clips at 255 and its inverse at 0, from sums beyond the pixel range
    lo, hi = [], []
    for ph in range(1, 16):
        xf, yf = ph & 3, ph >> 2
        if not (xf and yf):
            continue
        (y, x), (yi, xi) = where[ph, 0], where[ph, 1]
        top, inter_top = _unclipped(plane, y, x, xf, yf)
        bottom, inter_bot = _unclipped(plane, yi, xi, xf, yf)
        assert top > 255 and want[ph - 1, y, x] == 255, (ph, top)
        assert bottom < 0 and want[ph - 1, yi, xi] == 0, (ph, bottom)
        hi.append(top); lo.append(bottom)
        if ph == 10:            # xf = yf = 2: the ends of all three ranges the kernel's missing int16 narrowing rests on
            assert (top, bottom) == (518, -263)
            assert max(inter_top.max(), inter_bot.max()) == 14248 and min(inter_top.min(), inter_bot.min()) == -14312
            assert (inter_top + 8192).max() == 22440 and (inter_bot + 8192).min() == -6120
    assert len(hi) == 9
    _check(plane, 24, want)


CHILD_ROWS, CHILD_TILES = 28, 64


def _child():
    """One small case in a process of its own (the library reads X265HIP_PHASE_KERNEL once): four tile rows, whole quads (=2 takes the wide stores)."""
    sys.path.insert(0, ROOT)
    plane = _random_plane(4 * CHILD_TILES, 321)
    _check(plane, CHILD_ROWS)
    print("phase kernel child ok", os.environ.get("X265HIP_PHASE_KERNEL"))


@pytest.mark.parametrize("force", [None, "1", "2", "3"])
def test_every_kernel_selection(force):
    env = dict(os.environ)
    env.pop("X265HIP_PHASE_KERNEL", None)
    if force is not None:
        env["X265HIP_PHASE_KERNEL"] = force
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "phase kernel child ok" in r.stdout, (force, r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    _child()
