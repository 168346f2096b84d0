"""The server (any-length) kernels of dn_general.hip stage by stage against float64, on the host emulation of the kernel sources (no GPU
needed): dn_stft_general's spectrum AND log-mel, dn_server_rows on its own, dn_istft_general, the chain of the four ABI calls with
synthetic weights, and the refusals of the three entry points.  tests/server_cases.py holds the cases, the references (oracle/server_np64.py)
and the checks, and says what each shape reaches; tests/test_gpu_server.py runs the same checks on the MI355X.  Batch 2 here: the emulator
runs a work-item per OS thread.

Bars are the project's for the same stage (server_cases.py lists them); the guard bands below are 10 x the worst value this tier measured
in one run (python tools/server_margins.py --tier emu -> profiles/server_parity_margins.txt), never above the bar.  Every check prints its
figure first (`server-margin ...`, visible with -s).

Sensitivity, tried on a scratch copy of dn_general.hip with one edit at a time: the docstring of each test names the edits it fails on.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import model_abi  # noqa: E402
import server_cases as sc  # noqa: E402

BATCHES = (2,)
# stage -> guard band in the unit of its bar: 10 x the worst of the emulation tier in profiles/server_parity_margins.txt (rounded up to two
# digits).  The spectrum has no guard: ten times its worst (2.04e-7 of max|ref|) is 2.04e-6, above the bar of 2e-6 + 1e-6 / max|ref|
# (2.01e-6 .. 2.03e-6 here), so the bar stands alone there.
GUARD = {"logmel": 1.3e-5, "rows": 2.4e-6, "direction": 3.8e-7, "istft": 2.1e-6, "chain_rms": 5.0e-6, "chain_max": 3.5e-5, "chain_hx": 3.7e-6}
check = sc.Checker("emu", GUARD)


@pytest.fixture(scope="module")
def abi():
    return model_abi.Abi(emu.load())


@pytest.fixture(scope="module")
def plans(abi):
    p = sc.Plans(abi)
    yield p
    p.close()


@pytest.mark.parametrize("geometry,name", sc.STAGE_CASES, ids=sc.STAGE_IDS)
def test_stft_general_spectrum_and_logmel_against_float64(abi, plans, geometry, name):
    """Fails when the right reflection 2 L - 2 - i becomes 2 L - 1 - i (every case) and when the mel loop stops after its first 64 lanes
    (the 80- and 128-mel cases)."""
    sc.check_analysis(abi, plans, check, geometry, name, BATCHES)


@pytest.mark.parametrize("geometry", sc.GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in sc.GEOMETRIES])
def test_server_rows_against_float64_in_place_and_one_row(abi, plans, geometry):
    """Fails when `* 3.0f` is dropped and when the zero bin's phasor (1, 0) becomes (0, 0)."""
    sc.check_rows(abi, plans, check, geometry)


@pytest.mark.parametrize("n_fft,name", sc.ISTFT_CASES, ids=sc.ISTFT_IDS)
def test_istft_general_against_float64(abi, plans, n_fft, name):
    """Fails, under the asymmetric window only, when inv_env[n] is read mirrored, at hop - n (Hann's envelope is even).  Reading it at
    n + hop changes nothing and no test can see it: the plan's table 1 / (w[i]^2 + w[(i + hop) % n_fft]^2) has n_fft entries and is
    hop-periodic for every window, the two terms swapping."""
    sc.check_istft(abi, plans, check, n_fft, name, BATCHES)


@pytest.mark.parametrize("geometry,name,hx_decay", sc.CHAIN_CASES, ids=sc.CHAIN_IDS)
def test_three_requests_through_the_four_abi_calls_against_float64(abi, plans, geometry, name, hx_decay):
    """dn_stft_general, dn_cell_forward_ex(hx_decay), dn_server_rows in place, dn_istft_general with the synthetic hop blob: T = 10 through
    the cell, three requests with hx carried, waveform and hx of every request against server_np64.process_chunk64."""
    plan = plans.get(*geometry, name)
    run, done = sc.abi_chain_runner(abi, plan, hx_decay)
    try:
        sc.check_chain(check, geometry, name, hx_decay, plan.fb, run)
    finally:
        done()


def test_the_three_entry_points_refuse_bad_arguments_and_touch_nothing(abi, plans):
    sc.check_refusals(abi, plans)
