"""Shared cases of the input-phase tests (tests/test_emu_phase.py, tests/test_gpu_phase.py): DN_PHASE_FROM_INPUT, the Griffin-Lim chain started
from the unit phasors u = X / |X| of the hop's own analysis STFT.  TEST INFRASTRUCTURE; nothing here is product code.

Three parts:
  * the references: the analysis STFT X64 of the peak-normalised, pre-windowed frame in float64 (oracle/dsp_np64.py) on the fp32 window, its
    phasors, the fp32 torch restatement of both, and the fused hop from input phases in float64 (oracle/pipeline_np64.py) and in fp32 (the CPU
    oracle's own stages, oracle/pipeline_ref.py and oracle/dsp_ref.py, given phasors it computed itself);
  * Runner: every entry point of the C ABI that takes the flag, on host buffers (the emulated library) or on GPU buffers (model_abi.Abi), each
    run either WITH the flag or WITHOUT it and fed init_angles -- `identity` compares the two on everything the call writes;
  * the conditioning screen of the float64 cases and the seed table it gives (SEED_K), derived again by the CPU tier.

R, the allowed ratio of an error to the fp32 yardstick's error on the same case (e_ref), is set per family from the first GPU run
(profiles/phase_input_margins.txt: twice the largest measured ratio, rounded up to one digit)."""
import ctypes as C

import numpy as np
import torch

import dsp_cases as dc
from model_abi import Abi

DN_PEAK_NORMALIZE, DN_PRE_WINDOW, DN_CONV_BF16, DN_PHASE_FROM_INPUT = 1, 2, 1, 8
DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM = 2, 4
DN_ERR_INVALID = -1
N_FFTS = (512, 1024, 1536)
WINDOWS = ("hann", "asym")
FLT_MIN = float(np.finfo(np.float32).tiny)

# ratio bounds per family (module docstring), from the first run on an MI355X (profiles/phase_input_margins.txt holds every case's ratio).
# Phasors: a v_rsq_f32 (1 ulp) and two roundings per component on top of the fp32 transform, against torch's fp32 transform and a correctly rounded
# division.  Largest ratio 4.91 -- the constant frame under Hann, whose few low bins torch's transform gets almost exactly (its own error there is a
# seventh of its error on noise, ours 6e-8 = one rounding); on noise 0.8 .. 1.4.
R_PHASOR = 10.0
# The fused hop from input phases against the CPU oracle's fp32 stages: largest ratio 1.36 (process_frame) and 1.87 (the 12-hop stream).
R_FRAME = 3.0
R_STREAM = 4.0
BAR_RMS, BAR_MAX = 1e-3, 2e-2           # the project's waveform bars at scale max(1, RMS of the float64 waveform): R x e_ref must stay under them
RESID_BAR, HX_BAR = 1e-4, 1e-4          # the existing guard bands on the mel residual and hx (they do not depend on the phase source)
ULP_BAND = 4 * 2.0 ** -24               # | |u| - 1 |: v_rsq_f32 is 1 ulp, the two products half an ulp each


def geometry(n_fft):
    from oracle import pipeline_ref
    sr, n_mels = dc.HOP_GEOMETRY[n_fft]
    return pipeline_ref.Params(sr, n_fft, n_fft // 2, n_mels)


# ------------------------------------------------------------------ references
def prepared64(frames, w):
    """the frame as the STFT of the hop sees it, in float64 on the fp32 values: x / max|x| (when > 1e-6) x window -> (x, peak)"""
    x = np.asarray(frames, np.float64)
    peak = np.abs(x).max(axis=1)
    peak = np.where(peak > 1e-6, peak, 1.0)
    return x / peak[:, None] * np.asarray(w, np.float64), peak


def spectrum64(frames, n_fft, w):
    """X64 (B, K, 3) complex128: oracle/dsp_np64.stft of the normalised, pre-windowed frame"""
    from oracle import dsp_np64
    return dsp_np64.stft(prepared64(frames, w)[0], n_fft, n_fft // 2, w)


def phasors_of(X):
    """X / |X|, 1 where X == 0"""
    mag = np.abs(X)
    return np.where(mag > 0, X / np.where(mag > 0, mag, 1.0), 1.0 + 0.0j)


def phasors32(frames, n_fft, w):
    """the fp32 torch restatement: (B, K, 3) complex64 phasors of dsp_ref.spectrogram of the fp32 normalised, pre-windowed frame"""
    from oracle import dsp_ref
    f = torch.from_numpy(np.ascontiguousarray(frames, np.float32))
    wt = torch.from_numpy(np.ascontiguousarray(w, np.float32))
    peak = f.abs().amax(dim=1)
    peak = torch.where(peak > 1e-6, peak, torch.ones_like(peak))
    spec = dsp_ref.spectrogram(f / peak[:, None] * wt, n_fft, n_fft // 2, window=wt)
    mag = spec.abs()
    return torch.where(mag > 0, spec / torch.where(mag > 0, mag, torch.ones_like(mag)), torch.ones_like(spec)).numpy()


def weighted_error(u, X64):
    """max |u |X64| - X64| / max |X64|: a near-empty bin has an ill-conditioned phase, so the phasor is weighed by the bin's magnitude"""
    return float(np.abs(np.asarray(u, np.complex128) * np.abs(X64) - X64).max() / np.abs(X64).max())


def frame64(frames, hx0, p, w, n_iter):
    """the fused hop from input phases in float64 -> oracle/pipeline_np64.process_frame64's dict"""
    from oracle import pipeline_np64
    u = phasors_of(spectrum64(frames, p.n_fft, w))
    return pipeline_np64.process_frame64(frames, hx0, dc.model64(), w, dc.fbank(p), u, p.n_fft, p.hop, n_iter=n_iter)


def frame32(frames, hx0, p, n_iter):
    """the fp32 yardstick: the CPU oracle's own stages (Hann, as oracle/pipeline_ref.py builds it) given fp32 phasors it computed itself from
    dsp_ref.spectrogram.  pipeline_ref.process_frame has no n_iter argument: its body is spelled out with the one of dsp_ref.griffinlim."""
    from oracle import dsp_ref, model_ref, pipeline_ref
    sd = model_ref.unflatten_weights(np.fromfile(dc.os.path.join(dc.GOLDEN, "weights_dari_tult.bin"), dtype=np.float32))
    fb = dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate)
    f = torch.from_numpy(np.ascontiguousarray(frames, np.float32))
    u = torch.from_numpy(phasors32(frames, p.n_fft, torch.hann_window(p.n_fft).numpy()))
    with torch.no_grad():
        model_input, peak = pipeline_ref.analysis(f, p, fb)
        diff, hx = model_ref.forward(sd, model_input, torch.from_numpy(np.ascontiguousarray(hx0, np.float32)))
        lin = torch.clamp(dsp_ref.inverse_mel_scale(pipeline_ref.residual_to_mel_mag(model_input, diff), fb), min=0)
        y = dsp_ref.griffinlim(lin, p.n_fft, p.hop, n_iter=n_iter, init_angles=u)
    return dict(out=(y * peak[:, None]).numpy(), hx=hx.numpy(), predicted_diff=diff.numpy())


def stream_of(run_frame, signal, p, F):
    """the streaming loop (app3.py:178-226) around a per-frame function (frames, hx) -> dict(out, hx): F frames of signal (B, n_fft + (F - 1) hop)
    -> (emitted (B, F hop): frame f's hop is the overlap-add line BEFORE frame f is added, hx), in the dtype run_frame computes in"""
    B = signal.shape[0]
    hx, ola, emitted = None, None, []
    for f in range(F):
        r = run_frame(np.ascontiguousarray(signal[:, f * p.hop:f * p.hop + p.n_fft]), hx)
        hx = r["hx"]
        y = r["out"]
        if ola is None:
            ola = np.zeros((B, p.n_fft), y.dtype)
        emitted.append(ola[:, :p.hop].copy())
        ola = np.concatenate([ola[:, p.hop:], np.zeros((B, p.hop), y.dtype)], axis=1) + y
    return np.concatenate(emitted, axis=1), hx


def stream64(signal, p, w, n_iter, F):
    z = np.zeros((signal.shape[0], 17, p.num_compressed_bins))
    return stream_of(lambda fr, hx: frame64(fr, z if hx is None else hx, p, w, n_iter), signal, p, F)


def stream32(signal, p, n_iter, F):
    z = np.zeros((signal.shape[0], 17, p.num_compressed_bins), np.float32)
    return stream_of(lambda fr, hx: frame32(fr, z if hx is None else hx, p, n_iter), signal, p, F)


# ------------------------------------------------------------------ the float64 cases and their conditioning screen
FRAME_B, STREAM_B, STREAM_F = 6, 3, 12
E2E_N_ITERS = (0, 2, 6)
# (family, n_fft) -> k of the first candidate batch (noise seed 1300 + n_fft + 100 k) whose float64 result, at n_iter 2 AND 6, moves no stream by
# more than 1e-4 relative RMS under two 1e-7 relative perturbations of the signal.  n_iter 0 is one istft: it needs no screen and shares the batch.
# From the reference alone (first_well_conditioned_k); tests/test_emu_phase.py derives it again.
SEED_K = {("frame", 512): 0, ("frame", 1024): 0, ("frame", 1536): 0, ("stream", 512): 0, ("stream", 1024): 0, ("stream", 1536): 0}


def e2e_input(family, n_fft, k=None):
    """the noise of a float64 case at dsp_cases.HOP_LEVEL: frames (FRAME_B, n_fft) or a signal (STREAM_B, n_fft + (STREAM_F - 1) hop)"""
    k = SEED_K[(family, n_fft)] if k is None else k
    shape = (FRAME_B, n_fft) if family == "frame" else (STREAM_B, n_fft + (STREAM_F - 1) * (n_fft // 2))
    return dc.noise(shape, 1300 + n_fft + 100 * k + (7 if family == "stream" else 0), dc.HOP_LEVEL)


def e2e_ref64(family, n_fft, n_iter, x):
    """the float64 waveform of a case (Hann, the window the fp32 yardstick is built on): (B, n_fft) or the emitted (B, F hop), and hx"""
    p = geometry(n_fft)
    w = dc.window("hann", n_fft)
    if family == "frame":
        r = frame64(x, np.zeros((x.shape[0], 17, p.num_compressed_bins)), p, w, n_iter)
        return r["out"], r["hx"], r["predicted_diff"]
    y, hx = stream64(x, p, w, n_iter, STREAM_F)
    return y, hx, None


def conditioning(family, n_fft, k, n_iter, trials=2, relative=1e-7):
    """worst move of a stream of the float64 waveform, in RMS at scale max(1, RMS of the stream), when the signal is perturbed by
    `relative` x N(0, 1), over `trials` draws"""
    x = e2e_input(family, n_fft, k)
    ref = e2e_ref64(family, n_fft, n_iter, x)[0]
    scale = np.maximum(1.0, np.sqrt(np.mean(ref ** 2, axis=1)))
    rg = np.random.default_rng(1)
    worst = 0.0
    for _ in range(trials):
        y = e2e_ref64(family, n_fft, n_iter, x.astype(np.float64) * (1.0 + relative * rg.standard_normal(x.shape)))[0]
        worst = max(worst, float((np.sqrt(np.mean((y - ref) ** 2, axis=1)) / scale).max()))
    return worst


def first_well_conditioned_k(family, n_fft, k_max=8, limit=1e-4):
    return next(k for k in range(k_max) if all(conditioning(family, n_fft, k, it) <= limit for it in E2E_N_ITERS if it > 0))


# ------------------------------------------------------------------ every entry point, with the flag or with injected phases
def pack(u):
    """(B, K, 3) complex -> [B][3][K][2] float32"""
    return dc.ri(u)


class Runner(Abi):
    """The entry points that take DN_PHASE_FROM_INPUT.  Every run_* takes `inits`: None = the call carries the flag; else the call does NOT carry
    it and is fed these init_angles, one [B][3][K][2] array per frame.  Each returns a dict of host arrays: everything the call writes.
    Workspaces are handed over full of NaNs."""

    def __init__(self, lib, device=None, weights="dari_tult"):
        super().__init__(lib, device)
        self.blob = np.fromfile(dc.os.path.join(dc.GOLDEN, f"weights_{weights}.bin"), dtype=np.float32)
        self.plans = {}

    def plan(self, n_fft, window="hann"):
        from audio_denoising_amd._lib import DspCfg
        key = (n_fft, window)
        if key not in self.plans:
            p = geometry(n_fft)
            fb, w = np.ascontiguousarray(dc.fbank(p), np.float32), np.ascontiguousarray(dc.window(window, n_fft), np.float32)
            d = C.c_void_p()
            self.lib.check(self.lib.dn_dsp_create(C.byref(DspCfg(p.sample_rate, p.n_fft, p.hop, p.n_mels)), fb.ctypes.data_as(C.c_void_p), None,
                                                  w.ctypes.data_as(C.c_void_p), C.byref(d)))
            self.plans[key] = (p, d, self.model(self.blob, p.num_compressed_bins), w)
        return self.plans[key]

    def close(self):
        for _, d, m, _ in self.plans.values():
            self.lib.dn_dsp_destroy(d)
            self.lib.dn_model_destroy(m)
        self.plans = {}

    def flags(self, inits, extra=0):
        return extra | (DN_PHASE_FROM_INPUT if inits is None else 0)

    def phasors(self, plan, frames, flags=DN_PEAK_NORMALIZE | DN_PRE_WINDOW):
        """dn_stft_phasors -> [B][3][K][2] float32 on the host"""
        p, d = plan[0], plan[1]
        B = frames.shape[0]
        fr, out = self.up(frames), self.nan(B, 3, p.n_stft, 2)
        self.lib.check(self.lib.dn_stft_phasors(d, self.ptr(fr), self.ptr(out), B, flags, None))
        return self.down(out)

    def nan_bytes(self, n):
        assert n > 0 and n % 256 == 0, n
        return self.nan(n // 4)

    # -- dn_process_frame
    def run_frame(self, plan, frames, hx0, n_iter, inits=None, conv=0, ws=None):
        p, d, m, _ = plan
        lib, B = self.lib, frames.shape[0]
        fl = self.flags(inits, conv)
        ws = self.nan_bytes(lib.dn_workspace_bytes_ex(d, B, fl)) if ws is None else ws
        fr, hx, out, resid = self.up(frames), self.up(hx0), self.nan(B, p.n_fft), self.nan(B, 3, p.n_mels)
        ia = None if inits is None else self.up(inits[0])
        lib.check(lib.dn_process_frame(m, d, self.ptr(fr), self.ptr(hx), self.ptr(out), self.ptr(resid), self.ptr(ia), 11, 3, n_iter, 0.99,
                                       self.ptr(ws), B, fl, None))
        return dict(out=self.down(out), hx=self.down(hx), resid=self.down(resid))

    # -- dn_stream_step: the ring primed with the signal's first hop, then `hops` steps; frame h is signal[:, h hop : h hop + n_fft]
    def run_steps(self, plan, signal, hops, n_iter, inits=None):
        p, d, m, _ = plan
        lib, B = self.lib, signal.shape[0]
        fl = self.flags(inits)
        ring = np.zeros((B, p.n_fft), np.float32)
        ring[:, p.hop:] = signal[:, :p.hop]
        ring, ola, hx = self.up(ring), self.up(np.zeros((B, p.n_fft))), self.up(np.zeros((B, 17, p.num_compressed_bins)))
        ws = self.nan_bytes(lib.dn_workspace_bytes_ex(d, B, fl))
        outs = []
        for h in range(hops):
            hin, out = self.up(signal[:, (h + 1) * p.hop:(h + 2) * p.hop]), self.nan(B, p.hop)
            ia = None if inits is None else self.up(inits[h])
            lib.check(lib.dn_stream_step(m, d, self.ptr(hin), self.ptr(ring), self.ptr(ola), self.ptr(hx), self.ptr(out), self.ptr(ia), 11 + h, 3,
                                         n_iter, 0.99, self.ptr(ws), B, fl, None))
            outs.append(self.down(out))
        return dict(out=np.concatenate(outs, axis=1), ring=self.down(ring), ola=self.down(ola), hx=self.down(hx))

    # -- dn_clip_process: the same stream, all N hops in one call; signal float32 or int16
    def run_clip(self, plan, signal, N, n_iter, inits=None, gl=0, ws=None):
        p, d, m, _ = plan
        lib, B = self.lib, signal.shape[0]
        s16 = signal.dtype == np.int16
        fl = self.flags(inits, gl)
        first = as_float(signal[:, :p.hop])
        ring = np.zeros((B, p.n_fft), np.float32)
        ring[:, p.hop:] = first
        ring, ola, hx = self.up(ring), self.up(np.zeros((B, p.n_fft))), self.up(np.zeros((B, 17, p.num_compressed_bins)))
        ws = self.nan_bytes(lib.dn_clip_workspace_bytes_ex(d, B, N, fl)) if ws is None else ws
        hin = self.up(signal[:, p.hop:(N + 1) * p.hop], signal.dtype)
        out = self.up(np.full((B, N * p.hop), 7, signal.dtype), signal.dtype)
        ia = None if inits is None else self.up(np.stack(inits[:N], axis=1))          # [B][N][3][K][2]
        lib.check(lib.dn_clip_process(m, d, self.ptr(hin), int(s16), self.ptr(ring), self.ptr(ola), self.ptr(hx), self.ptr(out), int(s16),
                                      self.ptr(ia), 11, 3, n_iter, 0.99, self.ptr(ws), B, N, fl, None))
        return dict(out=self.down(out), ring=self.down(ring), ola=self.down(ola), hx=self.down(hx))

    # -- dn_pipe_*: a pipe in one of MODES
    def _pipe(self, plan, B, inits, streaming, mode):
        lib = self.lib
        pipe = C.c_void_p()
        create = lib.dn_pipe_stream_create if streaming else lib.dn_pipe_create
        lib.check(create(plan[2], plan[1], B, self.flags(inits), C.byref(pipe)))
        try:
            if "head" in mode:
                lib.check(lib.dn_pipe_set_head_start(pipe, mode["head"]))
            if mode.get("per_stream"):
                lib.check(lib.dn_pipe_set_gl_schedule(pipe, 2))
            if "depth" in mode:
                lib.check(lib.dn_pipe_set_depth(pipe, mode["depth"]))
            if mode.get("split"):
                lib.check(lib.dn_pipe_set_head_start(pipe, 0))
                lib.check(lib.dn_pipe_set_gl_schedule(pipe, 2))
                lib.check(lib.dn_pipe_set_split(pipe, 1))
            if "group" in mode:
                lib.check(lib.dn_pipe_set_group(pipe, mode["group"]))
        except Exception:
            lib.dn_pipe_destroy(pipe)
            raise
        return pipe

    def run_pipe_frames(self, plan, frames, n_iter, mode, inits=None):
        """frame mode: the frames (F, B, n_fft) submitted in order (a group pipe: in groups), one flush -> out (F, B, n_fft), hx"""
        p = plan[0]
        lib, (F, B) = self.lib, frames.shape[:2]
        pipe = self._pipe(plan, B, inits, False, mode)
        fr, out, hx = self.up(frames), self.nan(F, B, p.n_fft), self.up(np.zeros((B, 17, p.num_compressed_bins)))
        ia = None if inits is None else self.up(np.stack(inits[:F]))                  # [F][B][3][K][2]
        line, irow = B * p.n_fft, B * 3 * p.n_stft * 2
        try:
            H = mode.get("group", 0)
            if H:
                for f0 in range(0, F, H):
                    k = min(H, F - f0)
                    lib.check(lib.dn_pipe_submit_group(pipe, self.ptr(fr[f0:]), line, self.ptr(hx), self.ptr(out[f0:]), line,
                                                       None if ia is None else self.ptr(ia[f0:]), irow, 11, 3, k, n_iter, 0.99, None))
            else:
                for f in range(F):
                    lib.check(lib.dn_pipe_submit(pipe, self.ptr(fr[f]), self.ptr(hx), self.ptr(out[f]), None if ia is None else self.ptr(ia[f]),
                                                 11, 3, n_iter, 0.99, None))
            lib.check(lib.dn_pipe_flush(pipe, n_iter, 0.99, None))
            return dict(out=self.down(out), hx=self.down(hx))
        finally:
            lib.dn_pipe_destroy(pipe)

    def run_pipe_stream(self, plan, signal, pushes, n_iter, mode, inits=None):
        """streaming: `pushes` hops of the signal pushed (a group pipe: H at a time), then drained; push k >= 1 delivers frame k - 1.
        -> every emitted hop in order, and the state the pipe is left with"""
        p = plan[0]
        lib, B = self.lib, signal.shape[0]
        pipe = self._pipe(plan, B, inits, True, mode)
        zero = np.zeros((B, 3, p.n_stft, 2), np.float32)
        per_push = None if inits is None else [zero] + list(inits)                    # (push 0 primes the ring: its phases are not read)
        H, depth = mode.get("group", 0), mode.get("depth", 1)
        hop = lambda k: signal[:, k * p.hop:(k + 1) * p.hop]  # noqa: E731
        outs = []
        try:
            if H:
                assert pushes % H == 0
                for k0 in range(0, pushes, H):
                    hin, out = self.up(np.stack([hop(k) for k in range(k0, k0 + H)])), self.nan(H, B, p.hop)
                    ia = None if inits is None else self.up(np.stack(per_push[k0:k0 + H]))
                    lib.check(lib.dn_pipe_stream_push_group(pipe, self.ptr(hin), B * p.hop, 0, self.ptr(out), B * p.hop, 0, self.ptr(ia),
                                                            B * 3 * p.n_stft * 2, 11, 3, n_iter, 0.99, None))
                    outs += list(self.down(out))
                out, valid = self.nan(H, B, p.hop), C.c_int32(-1)
                lib.check(lib.dn_pipe_stream_flush_group(pipe, self.ptr(out), B * p.hop, 0, C.byref(valid), None))
                outs += list(self.down(out))
            else:
                for k in range(pushes):
                    hin, out = self.up(hop(k)), self.nan(B, p.hop)
                    ia = None if inits is None else self.up(per_push[k])
                    lib.check(lib.dn_pipe_stream_push(pipe, self.ptr(hin), 0, self.ptr(out), 0, self.ptr(ia), 11, 3, n_iter, 0.99, None))
                    outs.append(self.down(out))
                for _ in range(depth):
                    out = self.nan(B, p.hop)
                    lib.check(lib.dn_pipe_stream_flush(pipe, self.ptr(out), 0, n_iter, 0.99, None))
                    outs.append(self.down(out))
            ring, ola, hx = self.nan(B, p.n_fft), self.nan(B, p.n_fft), self.nan(B, 17, p.num_compressed_bins)
            lib.check(lib.dn_pipe_stream_get_state(pipe, self.ptr(ring), self.ptr(ola), self.ptr(hx), None))
            frames = C.c_uint64()
            lib.check(lib.dn_pipe_get_counters(pipe, None, C.byref(frames), None, None))
            return dict(out=np.stack(outs), ring=self.down(ring), ola=self.down(ola), hx=self.down(hx), frames=np.array(frames.value))
        finally:
            lib.dn_pipe_destroy(pipe)

    # -- dn_sessions_*: the streams on slots B .. 1 of a pool of B + 1, every push lists all of them
    def run_sessions(self, plan, signal, pushes, n_iter, schedule, inits=None):
        p = plan[0]
        lib, B = self.lib, signal.shape[0]
        pool = C.c_void_p()
        lib.check(lib.dn_sessions_create(plan[2], plan[1], B + 1, self.flags(inits), C.byref(pool)))
        try:
            lib.check(lib.dn_sessions_set_schedule(pool, schedule))
            ids = np.ascontiguousarray(np.arange(B, 0, -1), np.int32)
            idp = ids.ctypes.data_as(C.c_void_p)
            lib.check(lib.dn_sessions_open(pool, idp, B, None, None))
            outs = []
            for k in range(pushes):
                hin, out = self.up(signal[:, k * p.hop:(k + 1) * p.hop]), self.nan(B, p.hop)
                ia = None if inits is None or k == 0 else self.up(inits[k - 1])
                lib.check(lib.dn_sessions_push(pool, idp, B, self.ptr(hin), 0, self.ptr(out), 0, self.ptr(ia), 11, n_iter, 0.99, None))
                outs.append(self.down(out))
            rec = self.up(np.zeros((B, int(lib.dn_sessions_record_bytes(pool))), np.uint8), np.uint8)
            lib.check(lib.dn_sessions_export(pool, idp, B, self.ptr(rec), None))
            return dict(out=np.stack(outs), records=self.down(rec))
        finally:
            lib.dn_sessions_destroy(pool)


def as_float(x):
    """int16 PCM -> float32 as the kernels convert it (app3.py:172: x / 32767); float32 stays"""
    x = np.asarray(x)
    return x.astype(np.float32) / np.float32(32767.0) if x.dtype == np.int16 else x.astype(np.float32)


def stream_frames(signal, p, F):
    """frame f of a stream = samples [f hop, f hop + n_fft) of its signal (int16 converted as the kernels do)"""
    s = as_float(signal)
    return [np.ascontiguousarray(s[:, f * p.hop:f * p.hop + p.n_fft]) for f in range(F)]


def identity(runner, plan, frames_per_hop, run):
    """`run(inits)` with the flag (inits None) must equal `run` without it fed dn_stft_phasors of every frame, on everything it returns.
    -> the flagged run's results"""
    a = run(None)
    b = run([runner.phasors(plan, f) for f in frames_per_hop])
    assert a.keys() == b.keys()
    for key in a:
        assert np.isfinite(np.asarray(a[key], np.float64)).all() or a[key].dtype == np.uint8, f"{key}: not finite"
        assert np.array_equal(a[key], b[key]), f"{key}: the flag and the injected phasors differ ({int((a[key] != b[key]).sum())} of {a[key].size} values)"
    return a


# the pipe modes of the bit-identity family; those n_fft 512 and 1536 support are the first two
MODES = {"one_hop": {"head": 0}, "head_start": {"head": 2}, "per_stream": {"head": 0, "per_stream": True}, "depth2": {"depth": 2},
         "split": {"split": True}, "group2": {"group": 2}, "group4": {"group": 4}}
MODES_ANY_NFFT = ("one_hop", "head_start")


def stream_signal(B, n_fft, hops, seed=77):
    """B streams of noise, (hops + 1) hop samples: hop 0 primes"""
    return dc.noise((B, (hops + 1) * (n_fft // 2)), seed + n_fft, dc.HOP_LEVEL)


def to_s16(sig):
    return np.clip(np.rint(sig * (3000.0 / dc.HOP_LEVEL)), -32767, 32767).astype(np.int16)
