"""Any-length Griffin-Lim on the MI355X (``pytest -m gpu``): the checks of tests/test_emu_glg.py (tests/glg_cases.py holds them, the cases and
the float64 references) at batch 3 and at the shapes the emulator leaves out -- T = 8 on chip (512 threads, the whole LDS at n_fft 1536),
T = 9 and 19 in STEPS -- then ServerDenoiser(n_iter=...) and the torchaudio-style transforms at any length.  The device's rsq, its FMA
contraction and its LDS ordering are other code than the emulator's; the index arithmetic is the same.

Bars are the project's waveform bars; the guard bands below are 10 x the worst value measured in one run on one MI355X
(python tools/glg_margins.py --tier gpu -> profiles/glg_parity_margins.txt), never above the bar.  Every check prints its figure first
(`glg-margin ...`, visible with -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dsp_cases as dc
import glg_cases as gc
import model_abi
import model_cases as mc
import server_cases as sc
from oracle import dsp_np64, server_np64

pytestmark = pytest.mark.gpu

BATCH = gc.BATCH
# stage -> guard band in the unit of its bar: 10 x the worst of the gpu tier in profiles/glg_parity_margins.txt (rounded up to two digits).
# whole_rms (10 x 1.02e-4), direction (10 x 3.32e-7) and zero_iter_pair (10 x 2.37e-7) have none: ten times the worst is above the bar, which
# stands alone; hop_pair_* are held to the sum of two bands (glg_cases.py).
GUARD = {"whole_max": 7.9e-3, "steps_rms": 8.4e-4, "steps_max": 4.0e-3, "normalize0": 4.6e-6, "normalize4_rms": 5.8e-5, "normalize4_max": 2.9e-4,
         "mag_rows": 2.4e-6, "glchain_rms": 3.6e-5, "glchain_max": 3.2e-4, "glchain_hx": 4.4e-6, "t_spec": 1.5e-6, "t_istft": 1.9e-6,
         "t_gl_rms": 4.2e-4, "t_gl_max": 3.1e-3}
check = gc.Checker("gpu", GUARD)
ISTFT_GUARD = 2.1e-6            # test_gpu_server.py's guard band of dn_istft_general, relative to max|ref|


@pytest.fixture(scope="module")
def abi():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return model_abi.GpuBackend()


@pytest.fixture(scope="module")
def plans(abi):
    p = sc.Plans(abi)
    yield p
    p.close()


@pytest.mark.parametrize("case", gc.parity_cases("gpu"), ids=gc.case_id)
def test_parity_with_float64(abi, plans, case):
    gc.check_parity(abi, plans, check, case, BATCH)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_whole_and_steps_give_the_same_bits(abi, plans, n_fft):
    gc.check_forms_agree(abi, plans, n_fft, (3, 5, gc.WHOLE_MAX), BATCH)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_zero_iterations_is_istft_general_of_init_times_mag(abi, plans, n_fft):
    gc.check_zero_iterations(abi, plans, n_fft, (3, 5, gc.WHOLE_MAX, gc.WHOLE_MAX + 1), BATCH)


@pytest.mark.parametrize("n_fft,name", [(n, w) for n in dc.N_FFTS for w in dc.WINDOWS])
def test_three_columns_agree_with_the_hop_chain(abi, plans, n_fft, name):
    gc.check_against_hop_chain(abi, plans, check, n_fft, name, BATCH)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_device_phases(abi, plans, n_fft):
    gc.check_device_phases(abi, plans, n_fft, 4)
    gc.check_device_phases(abi, plans, n_fft, gc.WHOLE_MAX + 1)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_init_normalize_takes_unit_phasors_of_a_spectrum(abi, plans, n_fft):
    gc.check_init_normalize(abi, plans, check, n_fft, BATCH)


@pytest.mark.parametrize("geometry", gc.MAG_GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in gc.MAG_GEOMETRIES])
def test_server_mag_against_float64_and_server_rows(abi, plans, geometry):
    gc.check_server_mag(abi, plans, check, geometry)


def test_entry_points_refuse_bad_arguments_and_touch_nothing(abi, plans):
    gc.check_refusals(abi, plans)


# ------------------------------------------------------------------ ServerDenoiser
def _server(abi, geometry, name="asym", **kw):
    from audio_denoising_amd.pipeline import ServerDenoiser
    n_fft, sr, n_mels = geometry
    return ServerDenoiser(abi.gruunet2(mc.hop_blob()), sr, n_fft, n_fft // 2, n_mels, hx_decay=0.9, window=torch.from_numpy(dc.window(name, n_fft)), **kw)


@pytest.mark.parametrize("geometry", sc.CHAIN_GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in sc.CHAIN_GEOMETRIES])
def test_three_requests_through_server_denoiser_with_griffinlim(abi, geometry):
    """ServerDenoiser(n_iter=4, phase="input"): T = 10, three requests with hx carried, against the float64 chain
    (server_np64 stages, then dsp_np64.griffinlim from the unit phasors of the noisy spectrum)."""
    sd = _server(abi, geometry, n_iter=gc.CHAIN_N_ITER, phase="input")
    fb, _, _ = sd.plan.tables()

    def run(c, x, hx):
        wave, hx1 = sd.process(abi.up(x), hx)
        return abi.down(wave), abi.down(hx1), hx1

    gc.check_gl_chain(check, geometry, "asym", 0.9, fb.numpy(), run)
    assert sd.requests == sc.CHAIN_CHUNKS


@pytest.mark.parametrize("geometry", sc.CHAIN_GEOMETRIES, ids=[f"{g[0]}-{g[2]}mels" for g in sc.CHAIN_GEOMETRIES])
def test_server_denoiser_defaults_and_zero_iterations(abi, plans, geometry):
    """ServerDenoiser() with defaults gives the bits of the four ABI calls it made before; n_iter=0 from the input phases is the same
    reconstruction through another phasor arithmetic (one rsq instead of hypot and two divisions): within dn_istft_general's guard band."""
    x = sc.chain_chunks(geometry[0])[0]
    default, zero = _server(abi, geometry), _server(abi, geometry, n_iter=0, phase="input")
    w0, h0 = default.process(abi.up(x))
    run, done = sc.abi_chain_runner(abi, plans.get(*geometry, "asym"), 0.9)
    try:
        want, want_hx, _ = run(0, x, None)
    finally:
        done()
    assert np.array_equal(abi.down(w0), want) and np.array_equal(abi.down(h0), want_hx), "the default path changed its bits"
    w1, h1 = zero.process(abi.up(x))
    assert torch.equal(h1, h0)
    check("zero_iter_pair", float((w1 - w0).abs().max()) / float(w0.abs().max()), ISTFT_GUARD, n_fft=geometry[0])


def test_server_denoiser_random_phase_draws_from_seed_plus_request(abi, plans):
    geometry = sc.CHAIN_GEOMETRIES[0]
    x = abi.up(sc.chain_chunks(geometry[0])[0])
    sd, again, other = (_server(abi, geometry, n_iter=2, phase="random", seed=s) for s in (40, 40, 41))
    a0, _ = sd.process(x)
    a1, _ = sd.process(x)
    b0, _ = again.process(x)
    c0, _ = other.process(x)
    assert torch.equal(a0, b0) and torch.equal(a1, c0) and not torch.equal(a0, a1) and torch.isfinite(a1).all()
    with pytest.raises(ValueError):
        _server(abi, geometry, n_iter=2, phase="noisy")
    with pytest.raises(ValueError):
        _server(abi, geometry, n_iter=-1)
    with pytest.raises(ValueError):
        _server(abi, geometry, n_iter=2, momentum=1.0)


# ------------------------------------------------------------------ transforms
@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_transforms_take_any_length(abi, n_fft):
    from audio_denoising_amd import transforms as T
    dev, hop, name = abi.device, n_fft // 2, "hamming"
    w = dc.window(name, n_fft)
    kw = dict(n_fft=n_fft, win_length=n_fft, hop_length=hop, window_fn=torch.hamming_window)
    # Spectrogram at a ragged length
    L = 2 * n_fft + hop // 2 + 3
    x = dc.noise((2, L), 9100 + n_fft)
    S = T.Spectrogram(power=None, **kw).to(dev)
    spec = S(abi.up(x))
    ref = dsp_np64.stft(x, n_fft, hop, w)
    assert spec.shape == ref.shape == (2, n_fft // 2 + 1, 1 + L // hop)
    m = float(np.abs(ref).max())
    check("t_spec", float(np.abs(spec.cpu().numpy() - ref).max()) / m, sc.TOL_STFT_REL + sc.TOL_STFT_ABS / m, n_fft=n_fft)
    # InverseSpectrogram at T = 9
    z = sc.istft_spectrum(2, 9, n_fft, 9200 + n_fft)
    I = T.InverseSpectrogram(**kw).to(dev)
    wave = I(torch.from_numpy(z).to(dev).transpose(1, 2))
    ref = server_np64.synthesis(z, n_fft, hop, w)
    assert wave.shape == ref.shape
    check("t_istft", float(np.abs(wave.cpu().numpy() - ref).max()) / float(np.abs(ref).max()), sc.TOL_ISTFT, n_fft=n_fft)
    # GriffinLim at T = 9, injected phases
    key = (n_fft, name, 9, gc.N_ITER, gc.MOMENTUM)
    mag, init = gc.inputs(key)
    G = T.GriffinLim(n_iter=gc.N_ITER, power=1.0, momentum=gc.MOMENTUM, **kw).to(dev)
    got = G(torch.from_numpy(np.array(mag)).to(dev), init_angles=torch.from_numpy(np.array(init)).to(dev))
    ref = gc.case_reference(key)
    assert got.shape == ref.shape
    rms, mx, scale = dc.wave_errors(got.cpu().numpy(), ref)
    check("t_gl_rms", rms / scale, gc.TOL_WAVE_RMS, n_fft=n_fft)
    check("t_gl_max", mx / scale, gc.TOL_WAVE_MAX, n_fft=n_fft)
    torch.manual_seed(3)
    drawn = G(torch.from_numpy(np.array(mag)).to(dev))
    assert drawn.shape == got.shape and torch.isfinite(drawn).all() and not torch.equal(drawn, got)
    with pytest.raises(RuntimeError):
        G(torch.from_numpy(np.array(mag[:, :, :2])).to(dev))


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_three_column_transforms_keep_their_entry_points(abi, plans, n_fft):
    """(.., n_fft) frames, (.., K, 3) spectra and magnitudes reach dn_stft, dn_istft and dn_griffinlim as before: the bits of direct ABI calls."""
    from audio_denoising_amd import transforms as T
    dev, hop, lib = abi.device, n_fft // 2, abi.lib
    plan = gc.plan_of(plans, n_fft, "hann")
    kw = dict(n_fft=n_fft, win_length=n_fft, hop_length=hop)
    x = abi.up(dc.noise((2, n_fft), 9300 + n_fft))
    spec = T.Spectrogram(power=None, **kw).to(dev)(x)
    want = abi.nan(2, 3, plan.K, 2)
    lib.check(lib.dn_stft(plan.handle, abi.ptr(x), abi.ptr(want), 2, 0, None))
    assert torch.equal(torch.view_as_real(spec.transpose(1, 2).contiguous()), want)
    wave = T.InverseSpectrogram(**kw).to(dev)(spec)
    want_w = abi.nan(2, n_fft)
    lib.check(lib.dn_istft(plan.handle, abi.ptr(want), abi.ptr(want_w), 2, None))
    assert torch.equal(wave, want_w)
    mag, init = gc.magnitudes(2, n_fft, 3, 9400 + n_fft)
    got = T.GriffinLim(n_iter=3, power=1.0, **kw).to(dev)(abi.up(mag), init_angles=torch.from_numpy(init).to(dev))
    assert np.array_equal(got.cpu().numpy(), gc.run_hop_chain(abi, plan, mag, init, 3, 0.99))
