"""The GRUUNet2 conv tiles on the host emulation of the kernel sources (no GPU needed): dn_cell_forward (live rows only, lane geometry from
compares) against dn_cell_forward_parent_tiles (the tiles as they were), bit for bit on `out` and `hx`; tests/celltile_cases.py holds the cases.
The emulator models v_mfma_f32_16x16x4_f32 as the k-ordered fmaf chain it is, so a VALU row that takes its K slots in another order, skips a pad
slot or starts from another bias entry shows here.  B = 1: the emulator runs a work-item per OS thread (about a second a forward).
tests/test_gpu_celltiles.py runs the same cases on the GPU."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import celltile_cases as cc  # noqa: E402
import model_abi  # noqa: E402


@pytest.fixture(scope="module")
def backend():
    return model_abi.Abi(emu.load())


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_live_row_tiles_against_the_parent_tiles_bit_for_bit(backend, case):
    cc.check(backend, case, 1)
