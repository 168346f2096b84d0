#!/usr/bin/env python3
"""Measured parity margins of the whole hop at n_fft 512 against the live oracle (what tests/test_gpu_nfft512.py asserts, printed): mel-residual
and hx max-abs error (bar 1e-4), waveform RMS / max-abs error with shared Griffin-Lim phases (bars 1e-3 / 2e-2), every stream of the batch
compared.  L16 = 16 kHz / 512 / 64 mels, L8 = 8 kHz / 512 / 48 mels; batches 12 and 67 (silent, sub-threshold and square-wave streams among them)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_nfft512 as t  # noqa: E402  (helpers only: the frames and the comparison the tests use)


def main():
    dev = torch.device("cuda", 0)
    worst = [0.0] * 4
    for tag in ("L16", "L8"):
        for B in (12, 67):
            e = t.hop_errors(dev, tag, B, 512 + B)
            worst = [max(a, b) for a, b in zip(worst, e[:4])]
            print(f"{tag} batch {B}: residual max-abs err {e[0]:.2e}, hx {e[1]:.2e}, waveform rms err {e[2]:.2e} (signal rms {e[4]:.2e}), max-abs err {e[3]:.2e}")
    print(f"worst: residual {worst[0]:.2e}, hx {worst[1]:.2e}, waveform rms {worst[2]:.2e}, max-abs {worst[3]:.2e}")


if __name__ == "__main__":
    main()
