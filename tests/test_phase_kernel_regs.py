"""Register budget of the 8-bit phase-plane kernel, read from the built library without a GPU (the reader of tests/test_kernel_regs.py).

profiles/phase_planes_8bit.txt: the kernel streams 11 source rows through a lane and keeps seven (row, row + 1) pairs per xf and column alive; it was measured at
162 registers = three wavefronts per SIMD and no scratch.  The form with 4x8 tiles lost at two wavefronts per SIMD, and capping the registers spills."""
from test_kernel_regs import _kernels


def test_phase_luma8_kernel_keeps_three_wavefronts_and_no_scratch():
    k = _kernels()["phase_luma8_kernel"]
    assert 512 // k["vgpr"] >= 3 and k["vspill"] == 0 and k["scratch"] == 0, k
