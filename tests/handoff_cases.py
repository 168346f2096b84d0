"""Single-bin cases for the pair-order hand-off of the real transforms (rfft_split_pairs / irfft_merge_pairs, dn_wavefft.hpp), shared by
tests/test_emu_handoff.py and tests/test_gpu_handoff.py.

After the complex FFT of length NC = n_fft / 2 lane j holds Z[j + 64 t]; the split needs Z[NC - k] beside Z[k], which lane 64 - j holds, so the
values cross lanes once per direction.  Three kinds of lane exist, and a signal (a spectrum) whose energy sits in ONE bin says which of them
carried it wrong:
    lane 0    pairs with itself, one register further: bins 0, 64 t, NC / 2, NC - 64 t, NC
    lane 32   is its own partner, same register distance as everybody: bins 32 + 64 t
    others    one ordinary pair (5, NC - 5) as the control
The reference is float64 numpy.fft (oracle/dsp_np64.py); the bars are those tests/test_emu_windows.py holds the same entry points to: STFT
2e-6 max|ref| + 1e-6, waveform TOL_WAVE_RMS / TOL_WAVE_MAX at scale max(1, RMS of the float64 waveform).  Signals and spectra are scaled to
a waveform of RMS ~ 1, where a value handed to the wrong lane or register is an error of order 1."""
import numpy as np

N_FFTS = (512, 1024, 1536)


def bins(n_fft):
    """[(bin, which lane's hand-off it exercises)]"""
    nc = n_fft // 2
    np_ = nc // 128                                  # bin pairs a lane: NV / 2, NV = NC / 64
    lane0 = sorted({0, nc // 2, nc} | {64 * t for t in range(np_)} | {nc - 64 * t for t in range(np_)})
    lane32 = [32 + 64 * t for t in range(2 * np_)]
    return [(k, "lane 0") for k in lane0] + [(k, "lane 32") for k in lane32] + [(5, "control"), (nc - 5, "control")]


def signal(n_fft, k, rows):
    """(rows, n_fft) fp32: sqrt(2) cos(2 pi k n / n_fft + phase), one phase per row (never a multiple of pi / 2: DC and Nyquist stay non-zero)"""
    n = np.arange(n_fft, dtype=np.float64)
    ph = 0.3 + 0.9 * np.arange(rows, dtype=np.float64)[:, None]
    return (np.sqrt(2.0) * np.cos(2.0 * np.pi * k * n[None, :] / n_fft + ph)).astype(np.float32)


def spectrum(n_fft, k, rows):
    """(rows, K, 3) complex64, zero but for bin k of every column: complex values with non-zero imaginary parts (at DC and Nyquist too, where a
    C2R transform ignores them), scaled for a waveform of RMS ~ 1"""
    g = np.random.default_rng(1000 * n_fft + k)
    z = np.zeros((rows, n_fft // 2 + 1, 3), np.complex64)
    amp = 0.5 * n_fft * (1.0 + g.random((rows, 3)))
    z[:, k, :] = amp * np.exp(1j * (0.4 + 0.7 * g.random((rows, 3)))) * np.where(g.random((rows, 3)) < 0.5, -1.0, 1.0)
    assert (np.abs(z[:, k, :].imag) > 1.0).all()
    return z


def stft_bar(ref):
    return 2e-6 * float(np.abs(ref).max()) + 1e-6
