"""Any-length Griffin-Lim (dn_glg.hip: dn_griffinlim_general in its WHOLE and STEPS forms, dn_griffinlim_draw_phases_general, dn_server_mag) on the
host emulation of the kernel sources (no GPU needed).  tests/glg_cases.py holds the cases, the float64 references and the checks, and says what
each shape reaches; tests/test_gpu_glg.py runs the same checks on the MI355X at the larger shapes.  Batch 2 and T <= 5 on chip here: the
emulator runs a work-item per OS thread.

Bars are the project's waveform bars; the guard bands below are 10 x the worst value this tier measured in one run
(python tools/glg_margins.py --tier emu -> profiles/glg_parity_margins.txt), never above the bar.  Every check prints its figure first
(`glg-margin ...`, visible with -s).

Sensitivity, tried on a scratch copy of dn_glg.hip with one edit at a time: the docstring of each test names an edit it was seen to fail on.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import glg_cases as gc  # noqa: E402
import model_abi  # noqa: E402
import server_cases as sc  # noqa: E402

BATCH = 2
# stage -> guard band in the unit of its bar: 10 x the worst of the emulation tier in profiles/glg_parity_margins.txt (rounded up to two digits).
# `direction` has none: ten times its worst (3.32e-7) is above the bar of 8 ulp; hop_pair_* are held to the sum of two bands (glg_cases.py).
GUARD = {"whole_rms": 4.7e-4, "whole_max": 3.1e-3, "steps_rms": 2.4e-4, "steps_max": 9.9e-4, "normalize0": 4.6e-6, "normalize4_rms": 1.8e-5,
         "normalize4_max": 7.2e-5, "mag_rows": 2.4e-6, "glchain_rms": 1.6e-4, "glchain_max": 1.3e-3, "glchain_hx": 3.7e-6}
check = gc.Checker("emu", GUARD)


@pytest.fixture(scope="module")
def abi():
    return model_abi.Abi(emu.load())


@pytest.fixture(scope="module")
def plans(abi):
    p = sc.Plans(abi)
    yield p
    p.close()


@pytest.mark.parametrize("case", gc.parity_cases("emu"), ids=gc.case_id)
def test_parity_with_float64(abi, plans, case):
    """Fails (every case, both forms) when the right reflection `L - 2 - n0` of glg_segment becomes `L - 1 - n0`, and (asymmetric window)
    when WHOLE reads the envelope of a reflected sample mirrored."""
    gc.check_parity(abi, plans, check, case, BATCH)


@pytest.mark.parametrize("n_fft", gc.dc.N_FFTS)
def test_whole_and_steps_give_the_same_bits(abi, plans, n_fft):
    """Fails when WHOLE stores column t's first half to block t instead of t - 1, and when STEPS takes `mom` as torchaudio's momentum."""
    gc.check_forms_agree(abi, plans, n_fft, (3, 5), BATCH)


@pytest.mark.parametrize("n_fft", gc.dc.N_FFTS)
def test_zero_iterations_is_istft_general_of_init_times_mag(abi, plans, n_fft):
    gc.check_zero_iterations(abi, plans, n_fft, (3, 5, 9), BATCH)


@pytest.mark.parametrize("n_fft,name", [(n, w) for n in gc.dc.N_FFTS for w in gc.dc.WINDOWS])
def test_three_columns_agree_with_the_hop_chain(abi, plans, n_fft, name):
    gc.check_against_hop_chain(abi, plans, check, n_fft, name, BATCH)


@pytest.mark.parametrize("n_fft", gc.dc.N_FFTS)
def test_device_phases(abi, plans, n_fft):
    """Fails when glg_draw_kernel numbers its columns from 1."""
    gc.check_device_phases(abi, plans, n_fft, 4)


@pytest.mark.parametrize("n_fft", gc.dc.N_FFTS)
def test_init_normalize_takes_unit_phasors_of_a_spectrum(abi, plans, n_fft):
    """Fails when a bin below the smallest normal gets (0, 0) instead of (1, 0)."""
    gc.check_init_normalize(abi, plans, check, n_fft, BATCH)


@pytest.mark.parametrize("geometry", gc.MAG_GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in gc.MAG_GEOMETRIES])
def test_server_mag_against_float64_and_server_rows(abi, plans, geometry):
    gc.check_server_mag(abi, plans, check, geometry)


@pytest.mark.parametrize("geometry", sc.CHAIN_GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in sc.CHAIN_GEOMETRIES])
def test_three_requests_with_griffinlim_behind_the_model(abi, plans, geometry):
    """dn_stft_general, dn_cell_forward_ex, dn_server_mag, dn_griffinlim_general(DN_GL_INIT_NORMALIZE, n_iter 4; T = 10: STEPS) against the float64 chain."""
    plan = plans.get(*geometry, "asym")
    run, done = gc.abi_gl_chain_runner(abi, plan, 0.9, gc.CHAIN_N_ITER)
    try:
        gc.check_gl_chain(check, geometry, "asym", 0.9, plan.fb, run)
    finally:
        done()


def test_entry_points_refuse_bad_arguments_and_touch_nothing(abi, plans):
    gc.check_refusals(abi, plans)
