"""CPU-only checks of x265hip_subpel_refine_levels: declared, exported, and the level mask refused with the other arguments before a
device is asked for."""
import ctypes
import importlib
import os
import re

import pytest

EINVAL, ENODEV = -2, -1


def _lib():
    A = importlib.import_module("x265-yuuki-asuna_amd.hipabi")
    try:
        return A, A.lib()
    except OSError as e:            # the way the other argument tests load it; no device is needed for that
        pytest.skip(f"libx265hip.so cannot be loaded here: {e}")


def _params(A):
    p = A.SubpelParams()
    p.depth, p.width, p.height, p.range, p.subme = 8, 128, 64, 8, 3
    p.fenc, p.fenc_stride, p.fref, p.fref_stride = 0x10000, 320, 0x20000, 320
    p.best_in, p.cost_q, p.qoff, p.out = 0x30000, 0x40000, 40, 0x50000
    return p


def _entry(L, A):
    f = L.x265hip_subpel_refine_levels
    f.argtypes = [ctypes.POINTER(A.SubpelParams), ctypes.POINTER(A.SubpelChroma), ctypes.c_uint, ctypes.c_void_p]
    f.restype = ctypes.c_int
    return f


def test_levels_entry_is_declared_and_exported(repo_root):
    A, L = _lib()
    hdr = open(os.path.join(repo_root, "include", "x265hip.h")).read()
    assert re.search(r"int x265hip_subpel_refine_levels\(const x265hip_subpel_params\* p, const x265hip_subpel_chroma\* c, unsigned level_mask, void\* stream\);", hdr)
    assert "x265hip_subpel_refine_levels" in A.exported_symbols() and hasattr(L, "x265hip_subpel_refine_levels")


@pytest.mark.parametrize("mask", [0, 16, 31, 0xffffffff])
def test_level_mask_out_of_range_is_refused_without_a_device(mask):
    """Masks 0 and 16 (and larger ones): X265HIP_EINVAL with an error text that names the mask - with or without a device in the machine,
    since every argument check runs before the device is asked for."""
    A, L = _lib()
    f = _entry(L, A)
    p = _params(A)
    L.x265hip_last_error.restype = ctypes.c_char_p
    assert f(ctypes.byref(p), None, mask, None) == EINVAL
    text = L.x265hip_last_error()
    assert b"level_mask" in text and str(mask).encode() in text, text


def test_other_arguments_are_checked_like_the_four_level_entry():
    import torch
    A, L = _lib()
    f = _entry(L, A)
    assert f(None, None, 15, None) == EINVAL
    for k, v in (("depth", 9), ("width", 100), ("subme", 8), ("fenc", None), ("out", None)):
        q = _params(A)
        setattr(q, k, v)
        assert f(ctypes.byref(q), None, 4, None) == EINVAL, k
    c = A.SubpelChroma()
    c.fenc_cb, c.fenc_cr, c.fenc_stride_c, c.fref_cb, c.fref_cr, c.fref_stride_c = 0x60000, 0x70000, 256, 0x80000, None, 256
    assert f(ctypes.byref(_params(A)), ctypes.byref(c), 4, None) == EINVAL
    if not torch.cuda.is_available():
        for mask in (1, 4, 11, 15):                       # a legal mask gets as far as the device
            assert f(ctypes.byref(_params(A)), None, mask, None) == ENODEV, mask


def test_python_mask_helper():
    A, _ = _lib()
    assert A.subpel_level_mask(4) == 4 and A.subpel_level_mask((2,)) == 4 and A.subpel_level_mask({0, 1, 3}) == 11 and A.subpel_level_mask(range(4)) == 15
    for bad in (0, 16, (), (4,), (-1,)):
        with pytest.raises(ValueError):
            A.subpel_level_mask(bad)
