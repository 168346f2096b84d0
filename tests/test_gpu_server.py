"""The server (any-length) kernels of dn_general.hip stage by stage against float64 on the MI355X (``pytest -m gpu``): the checks of
tests/test_emu_server.py (tests/server_cases.py holds them, the cases and the float64 references of oracle/server_np64.py) at batches 1 and
3, the chain through ServerDenoiser.process with a window and an hx_decay passed in, and ServerDenoiser's own refusals.  The device's
expf / log1pf / hypotf and its FMA contraction are other code than the emulator's; the index arithmetic is the same.

Bars are the project's for the same stage (server_cases.py lists them); the guard bands below are 10 x the worst value measured in one run
on one MI355X (python tools/server_margins.py --tier gpu -> profiles/server_parity_margins.txt), never above the bar.  Every check prints
its figure first (`server-margin ...`, visible with -s).
"""
import numpy as np
import pytest
import torch

import dsp_cases as dc
import model_abi
import model_cases as mc
import server_cases as sc

pytestmark = pytest.mark.gpu

BATCHES = (1, 3)
# stage -> guard band in the unit of its bar: 10 x the worst of the gpu tier in profiles/server_parity_margins.txt (rounded up to two
# digits).  The spectrum's, 10 x 1.99e-7 of max|ref|, sits just under its bar of 2e-6 + 1e-6 / max|ref| (2.01e-6 .. 2.03e-6 here).
GUARD = {"spec": 2.0e-6, "logmel": 1.4e-5, "rows": 2.8e-6, "direction": 3.8e-7, "istft": 2.1e-6,
         "chain_rms": 4.9e-6, "chain_max": 4.0e-5, "chain_hx": 4.4e-6}
check = sc.Checker("gpu", GUARD)


@pytest.fixture(scope="module")
def abi():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return model_abi.GpuBackend()


@pytest.fixture(scope="module")
def plans(abi):
    p = sc.Plans(abi)
    yield p
    p.close()


@pytest.mark.parametrize("geometry,name", sc.STAGE_CASES, ids=sc.STAGE_IDS)
def test_stft_general_spectrum_and_logmel_against_float64(abi, plans, geometry, name):
    sc.check_analysis(abi, plans, check, geometry, name, BATCHES)


@pytest.mark.parametrize("geometry", sc.GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in sc.GEOMETRIES])
def test_server_rows_against_float64_in_place_and_one_row(abi, plans, geometry):
    sc.check_rows(abi, plans, check, geometry)


@pytest.mark.parametrize("n_fft,name", sc.ISTFT_CASES, ids=sc.ISTFT_IDS)
def test_istft_general_against_float64(abi, plans, n_fft, name):
    sc.check_istft(abi, plans, check, n_fft, name, BATCHES)


@pytest.mark.parametrize("geometry,name,hx_decay", sc.CHAIN_CASES, ids=sc.CHAIN_IDS)
def test_three_requests_through_server_denoiser_against_float64(abi, geometry, name, hx_decay):
    """ServerDenoiser(window=, hx_decay=).process with the synthetic hop blob: T = 10 through the cell, three requests with hx carried (the
    tensor process returns goes back in), the second request's x a non-contiguous view; waveform and hx of every request against
    server_np64.process_chunk64 on the filterbank the denoiser's plan holds."""
    from audio_denoising_amd.pipeline import ServerDenoiser
    n_fft, sr, n_mels = geometry
    sd = ServerDenoiser(abi.gruunet2(mc.hop_blob()), sr, n_fft, n_fft // 2, n_mels, hx_decay=hx_decay,
                        window=torch.from_numpy(dc.window(name, n_fft)))
    fb, _, win = sd.plan.tables()
    assert np.array_equal(win.numpy(), dc.window(name, n_fft))

    def run(c, x, hx):
        xd = abi.up(x)
        if c == 1:                                                   # every other sample of a twice-as-long row
            wide = torch.zeros(x.shape[0], 2 * x.shape[1], device=abi.device)
            wide[:, ::2] = xd
            xd = wide[:, ::2]
            assert not xd.is_contiguous()
        wave, hx1 = sd.process(xd, hx)
        return abi.down(wave), abi.down(hx1), hx1

    sc.check_chain(check, geometry, name, hx_decay, fb.numpy(), run)


def test_the_three_entry_points_refuse_bad_arguments_and_touch_nothing(abi, plans):
    sc.check_refusals(abi, plans)


def test_server_denoiser_refuses_other_tensors(abi):
    from audio_denoising_amd.pipeline import ServerDenoiser
    sd = ServerDenoiser(abi.gruunet2(mc.hop_blob()), 16000, 512, 256, 64)
    x = torch.from_numpy(dc.noise((2, 1000), 4100))
    for bad in (x, x.to(abi.device).double(), x[0].to(abi.device)):          # on the CPU, float64, 1-D
        with pytest.raises(ValueError, match="float32"):
            sd.process(bad)
    wave, hx = sd.process(x.to(abi.device))
    assert wave.shape == (2, 256 * (1000 // 256)) and hx.shape == (2, 17, 4) and torch.isfinite(wave).all()
