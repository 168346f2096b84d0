"""The pair-order hand-off of the real transforms through the wave's LDS tile (rfft_split_pairs / irfft_merge_pairs, dn_wavefft.hpp) on the GPU
(``pytest -m gpu``), where the tile really is shared memory and the wave's LDS operations really have to execute in order.

1.  dn_stft and dn_istft at n_fft 512 / 1024 / 1536, B = 2, on signals and spectra whose energy sits in one bin, against float64 numpy.fft
    (tests/handoff_cases.py: lane 0's bins, lane 32's, one ordinary pair), at the bars of tests/test_emu_windows.py.
2.  The short chain of tests/test_emu_handoff.py -- B = 3, three iterations -- as the wavefront-per-stream pipe (three hand-offs a direction
    through regions of the two exchange tiles) and as hop groups of two, against the one-hop pipe with a wavefront per column (the wave's own
    tile): frames, hx, emitted hops, ring and overlap-add line, torch.equal."""
import numpy as np
import pytest
import torch

import dsp_cases as dc
import handoff_cases as hc
from test_gpu_chain_loop import _check_frames, _check_stream, _per_stream, ctx, dev  # noqa: F401  (ctx, dev: fixtures)
from test_gpu_parity import TOL_WAVE_MAX, TOL_WAVE_RMS

pytestmark = pytest.mark.gpu

B_BIN = 2


@pytest.mark.parametrize("n_fft", hc.N_FFTS)
def test_stft_of_a_signal_in_one_bin(dev, n_fft):
    from audio_denoising_amd import transforms as T
    from oracle import dsp_np64
    hop, bad = n_fft // 2, []
    S = T.Spectrogram(power=None, n_fft=n_fft, win_length=n_fft, hop_length=hop).to(dev)
    w = torch.hann_window(n_fft).numpy()
    for k, who in hc.bins(n_fft):
        x = hc.signal(n_fft, k, B_BIN)
        got = S(torch.from_numpy(x).to(dev)).cpu().numpy().astype(np.complex128)
        ref = dsp_np64.stft(x, n_fft, hop, window=w)
        err = float(np.abs(got - ref).max())
        print(f"handoff stft n_fft={n_fft} bin={k} ({who}) err={err:.2e} bar={hc.stft_bar(ref):.2e}")
        assert np.abs(ref[:, k, 1]).min() > 0.1 * n_fft                                      # (the energy is where the case says)
        if err > hc.stft_bar(ref):
            bad.append(f"bin {k} ({who}): {err:.2e} > {hc.stft_bar(ref):.2e}; {dc.error_pattern(got, ref, n_fft)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n_fft", hc.N_FFTS)
def test_istft_of_a_spectrum_in_one_bin(dev, n_fft):
    from audio_denoising_amd import transforms as T
    from oracle import dsp_np64
    hop, bad = n_fft // 2, []
    I = T.InverseSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=hop).to(dev)
    w = torch.hann_window(n_fft).numpy()
    for k, who in hc.bins(n_fft):
        z = hc.spectrum(n_fft, k, B_BIN)
        got = I(torch.from_numpy(z).to(dev)).cpu().numpy()
        ref = dsp_np64.istft(z, n_fft, hop, window=w)
        rms, mx, scale = dc.wave_errors(got, ref)
        print(f"handoff istft n_fft={n_fft} bin={k} ({who}) rms={rms:.2e} max={mx:.2e} scale={scale:.2f}")
        assert np.sqrt(np.mean(ref ** 2)) > 0.1                                              # (real output, not a spectrum that cancels)
        if rms > TOL_WAVE_RMS * scale or mx > TOL_WAVE_MAX * scale:
            bad.append(f"bin {k} ({who}): rms {rms:.2e} max {mx:.2e} (scale {scale:.2f}); {dc.error_pattern(got, ref, n_fft)}")
    assert not bad, "\n".join(bad)


def test_wavefront_per_stream_chain_against_the_per_column_pipe(ctx):
    _check_frames(ctx, 3, 3, 2, _per_stream)
    _check_stream(ctx, 3, 3, _per_stream, 0)


def test_hop_group_of_two_against_the_per_column_pipe(ctx):
    _check_frames(ctx, 3, 3, 2, lambda pipe: None, H=2)
    _check_stream(ctx, 3, 3, lambda ps: None, 1, H=2)
