"""Shared cases of the window tests (tests/test_oracle_dsp.py, tests/test_emu_windows.py, tests/test_gpu_windows.py): the test windows, the
test signals, the float64 references built on oracle/dsp_np64.py and oracle/pipeline_np64.py, and the error-pattern report a failing
comparison prints.  TEST INFRASTRUCTURE; nothing here touches a kernel.

Why other windows than the periodic Hann (every test before these ran with it):
  * Hann is 0 at sample 0, so sample 0 of every STFT column -- one end of the left reflection: padded sample 0 of column 0 is x[H] -- is
    multiplied away.  Both test windows are nowhere zero.
  * The overlap-add envelope env[i] = w[i]^2 + w[(i + H) % N]^2 (H = N/2) is H-periodic for EVERY window (the two terms swap), and under Hann
    it is also even: env[-i] = env[i].  The kernels' "analysis window x 1/envelope of the column's source sample" tables read the envelope
    at H - n (column 0, reflected half), n (column 1) and 3H - 2 - n (column 2, reflected half).  With a periodic even envelope
    env[H - n] = env[n]: columns 0 and 1 hold the same table, and dropping column 0's reflection changes nothing -- no Hann test fails on
    that edit, in either schedule.  Column 2 reflects about the frame's LAST sample, not about its end: env[3H - 2 - n] = env[n + 2], a
    two-sample shift, so under Hann its table does differ from column 1's.  A host-built wave-per-stream table that gives column 2
    column 1's indices is therefore seen under Hann too, by the eight tests that hold that schedule bit-identical to wave-per-column
    (test_emu_kernels.py: one_wavefront_per_stream_is_bit_identical, deep_pipe_runs_the_chain_in_segments, hop_groups_run_whole_chains,
    streaming_hop_groups_emit_the_one_hop_pipes_samples_later[True]; test_emu_sessions.py: two_launch_schedule_emits_the_one_launch_samples).
    What no Hann test sees: an exchange of columns 0 and 1 or a dropped reflection in column 0 anywhere, and any error of column 2 that both
    schedules share.  W_ASYM's envelope is not even (asserted below): all three tables differ by more than 1e-2.
  * Hann is symmetric, w[n] = w[N - n]: a mirrored read of the window itself goes unnoticed.  W_ASYM is not.
W_HAMMING (symmetric, 0.08 at the edges) is what a caller would really pass through window_fn; Hann stays as the control.

The reference is always float64 on the fp32 window / filterbank values the kernels hold.
"""
import os

import numpy as np
import torch

from conftest import GOLDEN

N_FFTS = (512, 1024, 1536)
WINDOWS = ("asym", "hamming")            # the windows under test; "hann" is the control
# (sample rate, n_mels) of the fused-hop cases per n_fft: 64 mels = 4 compressed bins (weights_dari_tult.bin serves any count)
HOP_GEOMETRY = {512: (16000, 64), 1024: (16000, 64), 1536: (48000, 64)}
# Input level of the fused-hop cases.  The hop normalises by the frame's peak and multiplies it back (app3.py:181-217), and the model takes white
# noise down to 0.015 .. 0.06 of its level: noise of RMS 20 comes out with RMS 0.3 .. 1.2, so that the absolute waveform bars (scale
# max(1, RMS of the float64 waveform)) are about as tight relative to the signal as in the standalone Griffin-Lim cases.
HOP_LEVEL = 20.0


def column_sources(n_fft):
    """(3, n_fft) int: the index into the frame (= into the overlap-add envelope) that sample n of STFT column c reads -- reflect padding of
    n_fft/2 on both sides of an n_fft-sample frame, hop n_fft/2."""
    H = n_fft // 2
    n = np.arange(n_fft)
    return np.stack([np.where(n < H, H - n, n - H), n, np.where(n < H, n + H, 3 * H - 2 - n)])


def envelope(w):
    w = np.asarray(w, np.float64)
    return w * w + np.roll(w, -(w.size // 2)) ** 2


def window(name, n_fft):
    """fp32 (n_fft,) array built from n_fft alone."""
    n = np.arange(n_fft, dtype=np.float64)
    if name == "hann":
        return torch.hann_window(n_fft).numpy()
    if name == "hamming":
        return torch.hamming_window(n_fft).numpy()              # periodic
    assert name == "asym", name
    w = (0.3 + 0.7 * np.sin(np.pi * (n + 0.5) / n_fft) ** 2 * (1.0 + 0.5 * n / n_fft)).astype(np.float32)
    # conditions on the INPUT, not on any kernel: nowhere zero, not symmetric, and the three columns' tables really differ
    assert w.min() >= 0.3 and np.abs(w[1:] - w[:0:-1]).max() > 1e-2           # (w[n] against w[N - n])
    e = envelope(w)[column_sources(n_fft)]
    for a, b in ((0, 1), (1, 2), (0, 2)):
        assert np.abs(1.0 / e[a] - 1.0 / e[b]).max() > 1e-2 and np.abs(e[a] - e[b]).max() > 1e-2, (a, b)
    return w


def noise(shape, seed, rms=1.0):
    """fp32 white noise of the given RMS (the window tests' signals have RMS ~ 1)"""
    return (rms * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).numpy()


def magnitudes(B, n_fft, seed):
    """(B, K, 3) fp32 magnitudes and (B, K, 3) complex64 initial phases (real, imag ~ U[0, 1) as GriffinLim(rand_init=True) draws them); the
    magnitudes are scaled so that the reconstructed waveform has RMS ~ 1"""
    g = torch.Generator().manual_seed(seed)
    K = n_fft // 2 + 1
    mag = torch.rand(B, K, 3, generator=g) * (46.0 * np.sqrt(n_fft / 1024.0))
    init = torch.rand(B, K, 3, dtype=torch.complex64, generator=g)
    return mag.numpy(), init.numpy()


# Seeds of the 32-iteration Griffin-Lim cases at batch 67.  Thirty-two iterations amplify fp32-sized rounding by a factor that depends on the
# frame, with a heavy tail: perturbing the magnitudes of a batch of 67 random streams by 1e-7 (relative) moves the FLOAT64 result of one
# stream or another by 1e-3 .. 1.6e-2 RMS in most batches, which no fp32 implementation can be held to a 1e-3 bar on.  A batch is used when
# the float64 algorithm itself stays within 1e-4 RMS in every stream under two such perturbations (gl32_batch_is_well_conditioned below):
# the table holds, per (n_fft, window), the first k = 0, 1, 2 .. whose batch does (gl32_first_well_conditioned_k).  It is computed from the
# reference alone, not from any kernel's output; tests/test_oracle_dsp.py derives it again on the CPU, so it cannot go stale.
GL32_SEED_K = {(512, "asym"): 0, (512, "hamming"): 1, (512, "hann"): 2, (1024, "asym"): 6, (1024, "hamming"): 1, (1024, "hann"): 8,
               (1536, "asym"): 7, (1536, "hamming"): 1, (1536, "hann"): 0}
GL32_BATCH, GL32_N_ITER = 67, 32


def gl32_seed(n_fft, k):
    """the magnitudes() seed of the k-th candidate batch of the 32-iteration, batch-67 Griffin-Lim case"""
    return 400 + n_fft + GL32_N_ITER + GL32_BATCH + 1000 * k


def gl32_batch_is_well_conditioned(n_fft, name, k, trials=2, relative=1e-7, limit=1e-4):
    """True when float64 Griffin-Lim (oracle/dsp_np64.py) on candidate batch k moves no stream by more than `limit` RMS (at scale
    max(1, RMS of the stream)) when the magnitudes are perturbed by `relative` x N(0, 1), in each of `trials` draws"""
    from oracle import dsp_np64
    w = window(name, n_fft)
    mag, init = magnitudes(GL32_BATCH, n_fft, gl32_seed(n_fft, k))
    mag = mag.astype(np.float64)
    ref = dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=GL32_N_ITER, window=w)
    scale = np.maximum(1.0, np.sqrt(np.mean(ref ** 2, axis=1)))
    rg = np.random.default_rng(1)
    for _ in range(trials):
        y = dsp_np64.griffinlim(mag * (1.0 + relative * rg.standard_normal(mag.shape)), n_fft, n_fft // 2, init, n_iter=GL32_N_ITER, window=w)
        if (np.sqrt(np.mean((y - ref) ** 2, axis=1)) / scale).max() > limit:
            return False
    return True


def gl32_first_well_conditioned_k(n_fft, name, k_max=16):
    return next(k for k in range(k_max) if gl32_batch_is_well_conditioned(n_fft, name, k))


def ri(z):
    """(B, K, T) complex -> [B][T][K][2] float32, the kernels' storage"""
    z = np.asarray(z).transpose(0, 2, 1)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), dtype=np.float32)


def cplx(a):
    """[B][T][K][2] float32 -> (B, K, T) complex128"""
    a = np.asarray(a, np.float64)
    return (a[..., 0] + 1j * a[..., 1]).transpose(0, 2, 1)


def error_pattern(got, ref, n_fft):
    """Where a waveform (B, n_fft) or a spectrum (B, K, 3) is wrong: per column, per half of the frame, sample 0 alone -- what tells a swapped
    column table from a dropped reflection from an off-by-one at the window's first sample."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    H = n_fft // 2
    if err.ndim == 3 and err.shape[-1] == 3:
        return "max-abs error per column " + ", ".join(f"{err[:, :, c].max():.2e}" for c in range(3))
    if err.shape[-1] % H == 0 and err.shape[-1] >= n_fft:
        halves = ", ".join(f"{err[:, k * H:(k + 1) * H].max():.2e}" for k in range(err.shape[-1] // H))
        return (f"max-abs error per half-frame {halves}; sample 0 {err[:, 0].max():.2e}, sample 1 {err[:, 1].max():.2e}, "
                f"sample H {err[:, H].max():.2e}, last {err[:, -1].max():.2e}; worst at {np.unravel_index(err.argmax(), err.shape)}")
    return f"max-abs error {err.max():.2e} at {np.unravel_index(err.argmax(), err.shape)}"


def wave_errors(got, ref):
    """-> (RMS error, max-abs error, scale = max(1, RMS of the float64 waveform))"""
    ref = np.asarray(ref, np.float64)
    err = np.asarray(got, np.float64) - ref
    return float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max()), max(1.0, float(np.sqrt(np.mean(ref ** 2))))


# ------------------------------------------------------------------ the fused hop in float64
_SD64 = {}


def model64(short="dari_tult"):
    """GRUUNet2 forward in float64 (oracle/model_ref.forward on float64 weights) as process_frame64 wants it"""
    from oracle import model_ref
    if short not in _SD64:
        sd = model_ref.unflatten_weights(np.fromfile(os.path.join(GOLDEN, f"weights_{short}.bin"), dtype=np.float32))
        _SD64[short] = {k: v.double() for k, v in sd.items()}
    sd64 = _SD64[short]

    def run(x, hx):
        with torch.no_grad():
            o, h = model_ref.forward(sd64, torch.from_numpy(x), torch.from_numpy(hx))
        return o.numpy(), h.numpy()
    return run


def fbank(p):
    from oracle import dsp_ref
    return dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate).numpy()


def frames64(frames, inits, p, w, n_iter, momentum=0.99, hx0=None):
    """A chain of hops through oracle/pipeline_np64.process_frame64 with window w: frames, inits = lists of (B, n_fft) fp32 and (B, K, 3)
    complex64 arrays -> (list of float64 (B, n_fft) frames, float64 hx)"""
    from oracle import pipeline_np64
    B = frames[0].shape[0]
    hx = np.zeros((B, 17, p.num_compressed_bins)) if hx0 is None else hx0
    m64, fb, outs = model64(), fbank(p), []
    for f, ia in zip(frames, inits):
        r = pipeline_np64.process_frame64(f, hx, m64, w, fb, ia, p.n_fft, p.hop, n_iter=n_iter, momentum=momentum)
        hx = r["hx"]
        outs.append(r["out"])
    return outs, hx


def stream64(signal, inits, p, w, n_iter, momentum=0.99):
    """The streaming loop (app3.py:178-226) in float64: signal (B, n_fft + (F - 1) * hop), F = len(inits) frames -> emitted samples
    (B, F * hop) -- frame f's hop is the overlap-add line BEFORE frame f is added -- and hx."""
    B = signal.shape[0]
    F = len(inits)
    frames = [np.ascontiguousarray(signal[:, f * p.hop:f * p.hop + p.n_fft]) for f in range(F)]
    outs, hx = frames64(frames, inits, p, w, n_iter, momentum)
    ola = np.zeros((B, p.n_fft))
    emitted = []
    for y in outs:
        emitted.append(ola[:, :p.hop].copy())
        ola = np.concatenate([ola[:, p.hop:], np.zeros((B, p.hop))], axis=1) + y
    return np.concatenate(emitted, axis=1), hx
