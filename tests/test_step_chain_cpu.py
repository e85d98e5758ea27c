"""tests/step_chain.py's pieces that the chain pin (tests/test_step_chains_cpu.py) does not reach: the SAO record the GPU step tests hand
to their steps, and the chroma geometry against frames.pad_chroma's own."""
import importlib

import numpy as np
import pytest

import step_chain as SC
import test_step_chains_cpu as PIN

F = importlib.import_module("x265-yuuki-asuna_amd.frames")
HT = importlib.import_module("x265-yuuki-asuna_amd.host_tables")


@pytest.mark.parametrize("depth", PIN.DEPTHS)
def test_sao_rdo_inputs_is_the_record_of_the_pin(depth):
    for slice_type in (HT.SLICE_B, HT.SLICE_P, HT.SLICE_I):
        got, want = SC.sao_rdo_inputs(depth, PIN._qp(depth), slice_type), PIN._record(depth, slice_type)
        assert sorted(got) == sorted(want) and all(np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in want)
    types = [SC.sao_rdo_inputs(depth, PIN._qp(depth), s)["ctx_type"] for s in (HT.SLICE_B, HT.SLICE_P, HT.SLICE_I)]
    assert len(set(types)) == 3, "the slice type does not reach the record"


@pytest.mark.parametrize("w64", [64, 128, 1920])
def test_chroma_geometry_is_pad_chroma_s(w64):
    _, stride, org = F.pad_chroma(np.zeros((32, w64 // 2), np.uint8), w64, 64)
    assert SC.chroma_geometry(w64) == (stride, org)
