#!/usr/bin/env python3
"""Fixtures of the long-stream tests (TEST INFRASTRUCTURE): tests/golden/long_stream_<n_fft>.npz for n_fft 512, 1024 and 1536.

Run once, on a CPU:  python oracle/make_long_golden.py [n_fft ...]

The signal is tests/long_cases.py's "conversation" (built from a seed, nothing is read from disk); the references are this repository's own
oracles: float64 numpy DSP on the fp32 tables with the model in float64 (oracle/pipeline_np64.py, tests/dsp_cases.model64) and the fp32 CPU
oracle (oracle/pipeline_ref.py, oracle/model_ref.py).  A fixture holds
  sha256      of the int16 signal (all five streams): a numpy that draws another signal is noticed, not silently compared
  cps, hx64   the checkpoints (frame indices, long_cases.checkpoints) and the float64 hx of the B_REF reference streams after each
  e_ref       (frames, B_REF) float32: the fp32 oracle's hx error against float64 after EVERY frame -- the yardstick and its conditioning
  win_*       per window of 8 hops (long_cases.windows): its first frame, the float64 hx and overlap-add line in front of it (the tests
              recompute the float64 waveform from them), the fp32 oracle's error over the window in input-phase mode with n_iter = 0 --
              per hop relative to the hop's own float64 peak (win_e_rel) and absolute (win_e_abs), the worst of either -- and the fp32
              oracle's own int16 samples (win_s16_ref32), which the 1 % cap of the int16 comparison is checked on
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def make(n_fft):
    import long_cases as lc
    t0 = time.time()
    F = lc.HOPS[n_fft]
    cps = np.array(lc.checkpoints(n_fft))
    hx64, hx32 = lc.chains(n_fft, F)
    e_ref = np.stack([lc.hx_error(hx32[f], hx64[f]) for f in range(F)]).astype(np.float32)
    wins = lc.windows(n_fft)
    w_hx, w_ola, w_rel, w_abs, w_s16 = [], [], [], [], []
    for label, f0 in wins:
        ola64 = lc.ola_in_front_of(lc.run64(n_fft), n_fft, f0, hx64, np.float64)
        ola32 = lc.ola_in_front_of(lc.run32(n_fft), n_fft, f0, hx32, np.float32)
        y64, _ = lc.window64(n_fft, f0, hx64[f0 - 1], ola64)
        y32, _ = lc.window32(n_fft, f0, hx32[f0 - 1], ola32)
        rel, err = lc.hop_errors(y32, y64)
        w_hx.append(hx64[f0 - 1])
        w_ola.append(ola64)
        w_rel.append(rel.max())
        w_abs.append(err.max())
        w_s16.append(lc.s16_of_f32(y32))
        print(f"  window {label!r} at frame {f0}: e_ref_wave rel {rel.max():.3e} abs {err.max():.3e}; float64 peak per hop "
              f"{np.abs(y64).max(axis=2).min():.2e} .. {np.abs(y64).max():.2e}; int16 of fp32 differs in "
              f"{(lc.s16_of_f32(y32) != lc.s16_of(y64)).mean():.4%}")
    out = os.path.join(REPO, "tests", "golden", f"long_stream_{n_fft}.npz")
    np.savez_compressed(out, sha256=np.array(lc.sha256(n_fft)), hops=np.array(F), cps=cps, hx64=hx64[cps], e_ref=e_ref,
                        win_f0=np.array([f0 for _, f0 in wins]), win_label=np.array([label for label, _ in wins]), win_hx64=np.stack(w_hx),
                        win_ola64=np.stack(w_ola), win_e_rel=np.array(w_rel), win_e_abs=np.array(w_abs), win_s16_ref32=np.stack(w_s16))
    run = lc.running_max(e_ref.max(axis=1))
    print(f"n_fft {n_fft}: {F} hops, {cps.size} checkpoints, {len(wins)} windows, {os.path.getsize(out)} bytes, {time.time() - t0:.0f} s; "
          f"e_ref max over the first {lc.PREFIX} hops {run[lc.PREFIX - 1]:.3e}, over the run {run[-1]:.3e} (x{run[-1] / run[lc.PREFIX - 1]:.2f}), "
          f"worst at hop {int(e_ref.max(axis=1).argmax())}, at the last hop {e_ref[-1].max():.3e}; max |hx| {np.abs(hx64).max():.3f}")


if __name__ == "__main__":
    for n in [int(a) for a in sys.argv[1:]] or (512, 1536, 1024):
        make(n)
