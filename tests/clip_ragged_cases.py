"""The case tables of the ragged clip call (dn_clip_process_ragged), shared by tests/test_emu_clip_ragged.py (host emulation) and
tests/test_gpu_clip_ragged.py (MI355X).  No test in here.

  S   = 16 kHz, n_fft 1024, hop 512, 80 mels      R1 = 48 kHz, n_fft 1536, hop 768, 64 mels      L16 = 16 kHz, n_fft 512, hop 256, 64 mels

Stream b has run WARM[b] hops before the ragged call, so its overlap-add line and hx are non-zero and its frame0 differs from its neighbours':
a seed base shared by the streams fails every case."""
import numpy as np
import torch

DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM, DN_CONV_BF16, DN_PHASE_FROM_INPUT = 2, 4, 1, 8
DN_OK, DN_ERR_INVALID, DN_ERR_UNSUPPORTED = 0, -1, -2
MAX_FRAMES = 1 << 22          # frames a call carries at most
SEED, SID0 = 11, 2 ** 33 + 7
WARM = (2, 3, 2, 4, 3)        # hops stream b has run before the call = its frame0

# id -> (geometry, n_hops, flags, variant); variants: "plain", "s16" (int16 in and out), "init" (injected packed phases), "phin"
# (DN_PHASE_FROM_INPUT).  Host emulation: a work-item per OS thread, so at most 10 frames a call and four iterations.
#   (3, 0, 1, 2): N = 1, N = 2 and N >= 3 in the fold, a zero-length stream between live ones; per stream F = 6 fills one chain workgroup, partly
#   fills the next and puts a stream boundary inside a workgroup
EMU_N_ITER = 4
EMU_CASES = {
    "S-per-column": ("S", (3, 0, 1, 2), DN_CLIP_GL_PER_COLUMN, "plain"),
    "S-per-stream": ("S", (3, 0, 1, 2), DN_CLIP_GL_PER_STREAM, "plain"),
    "R1": ("R1", (2, 1, 3), 0, "plain"),
    "L16": ("L16", (2, 1, 3), 0, "plain"),
    "S-zero-first-and-last": ("S", (0, 2, 0), 0, "plain"),
    "L16-int16": ("L16", (2, 1, 3), 0, "s16"),
    "S-injected-phases": ("S", (2, 0, 1), DN_CLIP_GL_PER_STREAM, "init"),
    "S-phase-from-input": ("S", (2, 0, 1), 0, "phin"),
}
EMU_HOPS = 3                  # the yardstick's hops per stream behind the warm-up: the longest n_hops entry above

# MI355X: 32 iterations.  F = 15: four chain workgroups of the wavefront-per-frame form, the last partly filled, stream boundaries inside them
GPU_N_HOPS = (1, 0, 2, 9, 3)
GPU_CASES = {
    "S-per-column": ("S", DN_CLIP_GL_PER_COLUMN, "plain"),
    "S-per-stream": ("S", DN_CLIP_GL_PER_STREAM, "plain"),
    "S-auto": ("S", 0, "plain"),
    "R1": ("R1", 0, "plain"),
    "L16": ("L16", 0, "plain"),
    "S-int16": ("S", 0, "s16"),
    "S-bf16": ("S", 0, "bf16"),
    "S-phase-from-input": ("S", 0, "phin"),
}


def signal(n, length, seed):
    """n rows of a tone each, of different levels and pitches, in a little noise"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(length) / 16000.0
    tones = torch.stack([(0.05 + 0.2 * k) * torch.sin(2 * np.pi * (180.0 + 95.0 * k) * t) for k in range(n)])
    return (tones + 0.03 * torch.randn(n, length, generator=g)).float()


def offsets(n_hops):
    """off[b] = n_hops[0] + ... + n_hops[b - 1], off[B] = F"""
    return [int(v) for v in np.concatenate([[0], np.cumsum(n_hops)])]


def to_pcm(x):
    """float samples -> int16 PCM (numpy)"""
    return np.clip(np.asarray(x) * 32767.0, -32768, 32767).astype(np.int16)


def pcm_out(ref):
    """what the int16 output of float32 hops is: clip, scale, truncate (app3.py:244-245)"""
    return (np.clip(ref, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
