"""Float64 restatement of the socket server's request-loop body (server.py:207-216), STAGE BY STAGE, on oracle/dsp_np64.py
(TEST INFRASTRUCTURE; DSP stages PARITY UNPINNED like dsp_np64.py, which does the transforms).

    spec = T0(X); phase = angle; magn = abs; log_mel = M0T(magn).log1p()       server.py:207-210   analysis()
    out, hx = model(log_mel.T, hx); hx = hx * 0.9                              server.py:212, 214  process_chunk64()
    O = M0I(exp(log_mel - relu(out) * 3) - 1); polar(O, phase)                 server.py:213-216   rows()
    I0(.)                                                                      server.py:216       synthesis()

The three stage functions are what dn_stft_general, dn_server_rows and dn_istft_general compute, in the kernels' own layouts
(spec (B, T, K) complex, log-mel and model output (B, T, M)).  They take the fp32 tables the plan holds (dn_dsp_get_tables: filterbank,
pseudo-inverse, window) widened to float64, so that a stage test measures the kernel and not the table.  process_chunk64, the chain, does
NOT take the plan's pseudo-inverse: it solves the least-squares problem itself (dsp_np64.inverse_mel_scale), so that a wrong table cannot
hide end to end.
"""
from __future__ import annotations

import numpy as np

from . import dsp_np64


def analysis(x, n_fft, hop, window, fb):
    """x (B, L) -> spec (B, T, K) complex128, logmel (B, T, M); T = 1 + L // hop.  window (n_fft,) or None (Hann), fb (K, M)."""
    spec = dsp_np64.stft(x, n_fft, hop, window).transpose(0, 2, 1)
    return spec, np.log1p(np.abs(spec) @ np.asarray(fb, np.float64))


def mel_magnitude(logmel, model_out):
    """mm = exp(logmel - 3 relu(out)) - 1 (server.py:213, 215); negative where 3 relu(out) > logmel"""
    return np.exp(np.asarray(logmel, np.float64) - 3.0 * np.maximum(np.asarray(model_out, np.float64), 0.0)) - 1.0


def unit_phasor(z):
    """z / |z|, and (1, 0) where z == 0: torch.polar(., angle(z)) with angle(0) = 0"""
    z = np.asarray(z, np.complex128)
    a = np.abs(z)
    return np.where(a > 0.0, z / np.where(a > 0.0, a, 1.0), 1.0 + 0.0j)


def rows(logmel, model_out, spec_in, pinv):
    """logmel, model_out (..., M), spec_in (..., K) complex, pinv (K, M) -> spec_out (..., K) = relu(mm @ pinv^T) * u"""
    mag = np.maximum(mel_magnitude(logmel, model_out) @ np.asarray(pinv, np.float64).T, 0.0)
    return mag * unit_phasor(spec_in)


def synthesis(spec, n_fft, hop, window):
    """spec (B, T, K) complex, T >= 2 -> (B, hop (T - 1)): InverseSpectrogram with length=None"""
    return dsp_np64.istft(np.asarray(spec, np.complex128).transpose(0, 2, 1), n_fft, hop, window)


def process_chunk64(x, hx, model64, n_fft, hop, window, fb, hx_decay=0.9, zero_model_out=False):
    """One request: x (B, L), hx (B, 17, C); model64(x (B, T, M), hx) -> (out (B, T, M), hx) is the GRUUNet2 forward in float64.
    -> dict of float64 arrays: out (B, hop (T - 1)), hx (times hx_decay), spec, logmel, model_out, lin (B, T, K).
    zero_model_out: the waveform with model_out = 0 (the model stage switched off; what a test's liveness condition compares with)."""
    spec, logmel = analysis(x, n_fft, hop, window, fb)
    model_out, hx1 = model64(logmel, np.asarray(hx, np.float64))
    mm = mel_magnitude(logmel, np.zeros_like(model_out) if zero_model_out else model_out)
    lin = dsp_np64.inverse_mel_scale(mm.transpose(0, 2, 1), fb).transpose(0, 2, 1)             # lstsq, relu included
    wave = synthesis(lin * unit_phasor(spec), n_fft, hop, window)
    return dict(out=wave, hx=hx1 * hx_decay, spec=spec, logmel=logmel, model_out=model_out, lin=lin)
