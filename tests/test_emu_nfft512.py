"""n_fft 512 (the 256-point one-wave FFT, 256 = 4*4*4*4) on the host emulation of the kernel sources: the transform against the oracle on
signals that hit DC, the self-paired mid bin 128 and bin 256 exactly; the whole hop, the stream, the one-hop pipe and a session pool at
the two geometries the size is for; the schedules that are not built at this size are refused.

  L16 = 16 kHz, n_fft 512, hop 256, 64 mels   (half the window / hop latency of the 1024 path)
  L8  =  8 kHz, n_fft 512, hop 256, 48 mels   (the 64 ms window / 32 ms hop of the checkpoints, at 8 kHz)

Tolerances are those of tests/test_gpu_parity.py (TOL_RESIDUAL, TOL_HX_STREAM, _wave_close), imported from there.  The oracle is called
live.  Small shapes: the emulator runs a work-item per OS thread."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
from audio_denoising_amd._lib import (DN_GL_AUTO, DN_GL_WAVE_PER_COLUMN, DN_GL_WAVE_PER_STREAM, DN_SESS_AUTO, DN_SESS_ONE_LAUNCH,  # noqa: E402
                                      DN_SESS_TWO_LAUNCHES, DN_SPLIT_AUTO, DN_SPLIT_OFF, DN_SPLIT_ON, DspCfg, ModelCfg)
from audio_denoising_amd.sessions import record_layout  # noqa: E402
from oracle import dsp_ref, model_ref, pipeline_ref  # noqa: E402
from test_gpu_parity import TOL_HX_STREAM, TOL_RESIDUAL, _wave_close  # noqa: E402

L16 = pipeline_ref.Params(16000, 512, 256, 64)
L8 = pipeline_ref.Params(8000, 512, 256, 48)
GEOS = {"L16": L16, "L8": L8}
DN_ERR_INVALID, DN_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def sd():
    return model_ref.unflatten_weights(np.fromfile(os.path.join(GOLDEN, "weights_dari_tult.bin"), dtype=np.float32))


def _dsp(lib, p, fb=True):
    f = emu.f32(dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate).numpy()) if fb and p.n_mels else None
    h = C.c_void_p()
    lib.check(lib.dn_dsp_create(C.byref(DspCfg(p.sample_rate, p.n_fft, p.hop, p.n_mels)), emu.ptr(f), None,
                                emu.ptr(emu.f32(torch.hann_window(p.n_fft).numpy())), C.byref(h)))
    return h


def _model(lib, Cb):
    w = np.fromfile(os.path.join(GOLDEN, "weights_dari_tult.bin"), dtype=np.float32)
    h = C.c_void_p()
    lib.check(lib.dn_model_create(emu.ptr(w), w.size, C.byref(ModelCfg(Cb, 1, 4, 17, 3, 2, 1, 6)), C.byref(h)))
    return h


@pytest.fixture(scope="module")
def plans(lib):
    """tag -> (params, plan, model) for the two geometries"""
    d = {t: (p, _dsp(lib, p), _model(lib, p.num_compressed_bins)) for t, p in GEOS.items()}
    yield d
    for _, h, m in d.values():
        lib.dn_dsp_destroy(h)
        lib.dn_model_destroy(m)


def _ri(z):
    """(B, K, 3) complex -> [B][3][K] interleaved re, im"""
    z = np.asarray(z).transpose(0, 2, 1)
    return emu.f32(np.stack([z.real, z.imag], axis=-1))


def _signal(n, length, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(length) / 16000.0
    tones = torch.stack([0.05 * torch.sin(2 * np.pi * (180.0 + 95.0 * k) * t) for k in range(n)])
    return (tones + 0.03 * torch.randn(n, length, generator=g)).float()


# ------------------------------------------------------------------ the transform
def test_spectrogram_of_five_frames_hits_dc_mid_and_last_bin_and_inverts(lib):
    p = L16
    h = _dsp(lib, pipeline_ref.Params(16000, 512, 256, 0))
    x = torch.zeros(5, p.n_fft)
    x[0, 0] = 1.0                                               # impulse at sample 0
    x[1, 511] = 1.0                                             # impulse at the last sample
    x[2, :] = 1.0                                               # constant: DC
    x[3, :] = torch.tensor([1.0, -1.0]).repeat(256)             # Nyquist rate: bin 256
    x[4, :] = torch.randn(p.n_fft, generator=torch.Generator().manual_seed(3)) + torch.cos(np.pi * torch.arange(512) / 2)   # noise + bin 128
    spec = np.zeros((5, 3, p.n_stft, 2), np.float32)
    lib.check(lib.dn_stft(h, emu.ptr(emu.f32(x.numpy())), emu.ptr(spec), 5, 0, None))
    ref = dsp_ref.spectrogram(x, p.n_fft, p.hop).numpy()
    got = (spec[..., 0] + 1j * spec[..., 1]).transpose(0, 2, 1)
    for i in range(5):              # per frame: an impulse's spectrum (|X| <= 1) is not checked at the scale of the constant frame's (256)
        assert np.abs(got[i] - ref[i]).max() <= 2e-6 * np.abs(ref[i]).max() + 1e-6, i
    # the bins the Hermitian split treats on their own are where the signals put their energy
    assert abs(ref[2, 0, 1]) > 100 and abs(ref[3, 256, 1]) > 100 and abs(ref[4, 128, 1]) > 50
    wave = np.zeros((5, p.n_fft), np.float32)
    lib.check(lib.dn_istft(h, emu.ptr(spec), emu.ptr(wave), 5, None))
    assert np.abs(wave - x.numpy()).max() <= 2e-5
    lib.dn_dsp_destroy(h)


# ------------------------------------------------------------------ the whole hop
@pytest.mark.parametrize("tag", ["L16", "L8"])
def test_process_frame_matches_the_oracle_at_batches_1_3_5(lib, plans, sd, tag):
    p, dsp, m = plans[tag]
    Cb = p.num_compressed_bins
    fb = dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate)
    g = torch.Generator().manual_seed(512 + p.sample_rate)
    frames_all = 0.1 * torch.randn(5, p.n_fft, generator=g)
    init_all = torch.rand(5, p.n_stft, 3, dtype=torch.complex64, generator=g)
    with torch.no_grad():
        ref = pipeline_ref.process_frame(sd, frames_all, torch.zeros(5, 17, Cb), p, fb, init_angles=init_all)
    assert torch.isfinite(ref["out"]).all()
    for B in (1, 3, 5):
        ws = np.zeros(lib.dn_workspace_bytes(dsp, B) // 4 + 16, np.float32)
        hx = np.zeros((B, 17, Cb), np.float32)
        out = np.zeros((B, p.n_fft), np.float32)
        resid = np.zeros((B, 3, p.n_mels), np.float32)
        lib.check(lib.dn_process_frame(m, dsp, emu.ptr(emu.f32(frames_all[:B].numpy())), emu.ptr(hx), emu.ptr(out), emu.ptr(resid),
                                       emu.ptr(_ri(init_all[:B].numpy())), 0, 0, 32, 0.99, emu.ptr(ws), B, 0, None))
        assert np.abs(resid - ref["predicted_diff"][:B].numpy()).max() <= TOL_RESIDUAL, B
        assert np.abs(hx - ref["hx"][:B].numpy()).max() <= TOL_RESIDUAL, B
        _wave_close(out, ref["out"][:B].numpy())


# ------------------------------------------------------------------ streams and the one-hop pipe
def test_six_hop_stream_matches_streamref_and_the_pipe_equals_it_one_hop_late(lib, plans, sd):
    p, dsp, m = plans["L16"]
    B, n_hops, Cb = 3, 6, p.num_compressed_bins
    sig = _signal(B, (n_hops + 1) * p.hop, 21)
    g = torch.Generator().manual_seed(22)
    inits = [torch.rand(B, p.n_stft, 3, dtype=torch.complex64, generator=g) for _ in range(n_hops)]
    with torch.no_grad():
        oracle = pipeline_ref.StreamRef(sd, p, B)
        ref = oracle.push(sig, inits).numpy()
    assert ref.shape == (B, n_hops * p.hop)
    # serial: dn_stream_step, the first hop in the ring already
    ws = np.zeros(lib.dn_workspace_bytes(dsp, B) // 4 + 16, np.float32)
    ring = np.zeros((B, p.n_fft), np.float32)
    ring[:, p.hop:] = sig[:, :p.hop].numpy()
    ola = np.zeros((B, p.n_fft), np.float32)
    hx = np.zeros((B, 17, Cb), np.float32)
    serial = []
    for k in range(n_hops):
        hop_in = emu.f32(sig[:, (k + 1) * p.hop:(k + 2) * p.hop].numpy())
        out = np.zeros((B, p.hop), np.float32)
        lib.check(lib.dn_stream_step(m, dsp, emu.ptr(hop_in), emu.ptr(ring), emu.ptr(ola), emu.ptr(hx), emu.ptr(out),
                                     emu.ptr(_ri(inits[k].numpy())), 0, 0, 32, 0.99, emu.ptr(ws), B, 0, None))
        serial.append(out)
    assert np.abs(hx - oracle.hx.numpy()).max() <= TOL_HX_STREAM
    _wave_close(np.concatenate(serial, axis=1), ref)
    assert np.abs(ref[:, p.hop:]).max() > 1e-3
    # the pipe of depth 1: push 0 primes the ring, push k + 1 fronts frame k, whose hop comes out of push k + 2 (the flush for the last)
    pipe = C.c_void_p()
    lib.check(lib.dn_pipe_stream_create(m, dsp, B, 0, C.byref(pipe)))
    piped, keep = [], []
    for k in range(n_hops + 1):
        hop_in = emu.f32(sig[:, k * p.hop:(k + 1) * p.hop].numpy())
        ia = _ri(inits[k - 1].numpy()) if k >= 1 else None
        keep.append((hop_in, ia))
        out = np.full((B, p.hop), 7.0, np.float32)
        lib.check(lib.dn_pipe_stream_push(pipe, emu.ptr(hop_in), 0, emu.ptr(out), 0, emu.ptr(ia), 0, 0, 32, 0.99, None))
        piped.append(out)
    last = np.zeros((B, p.hop), np.float32)
    lib.check(lib.dn_pipe_stream_flush(pipe, emu.ptr(last), 0, 32, 0.99, None))
    piped.append(last)
    lib.dn_pipe_destroy(pipe)
    assert not piped[0].any() and not piped[1].any()
    for k in range(n_hops):
        assert np.array_equal(piped[k + 2], serial[k]), k


# ------------------------------------------------------------------ a session pool
class _Pool:
    def __init__(self, lib, m, dsp, p, cap):
        self.lib, self.p = lib, p
        self.h = C.c_void_p()
        lib.check(lib.dn_sessions_create(m, dsp, cap, 0, C.byref(self.h)))
        self.stride = int(lib.dn_sessions_record_bytes(self.h))

    def open(self, ids, sids):
        i, s = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(sids, dtype=np.uint64)
        self.lib.check(self.lib.dn_sessions_open(self.h, emu.ptr(i), i.size, emu.ptr(s), None))

    def push(self, ids, hops, seed, n_iter):
        i = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.full((i.size, self.p.hop), 7, np.float32)
        self.lib.check(self.lib.dn_sessions_push(self.h, emu.ptr(i), i.size, emu.ptr(emu.f32(hops)), 0, emu.ptr(out), 0, None, seed, n_iter,
                                                 0.99, None))
        return out

    def export(self, ids):
        i = np.ascontiguousarray(ids, dtype=np.int32)
        rec = np.full((i.size, self.stride), 0xA5, np.uint8)
        self.lib.check(self.lib.dn_sessions_export(self.h, emu.ptr(i), i.size, emu.ptr(rec), None))
        return rec

    def import_(self, ids, rec):
        i = np.ascontiguousarray(ids, dtype=np.int32)
        self.lib.check(self.lib.dn_sessions_import(self.h, emu.ptr(i), i.size, emu.ptr(np.ascontiguousarray(rec)), None, None))

    def destroy(self):
        self.lib.dn_sessions_destroy(self.h)


class _Step:
    """one session as dn_stream_step at B = 1: the first hop fills ring[hop:], hop k >= 1 runs frame k - 1 under (seed + k - 1, stream id)"""

    def __init__(self, lib, m, dsp, p, sid, seed, n_iter):
        self.lib, self.m, self.dsp, self.p, self.sid, self.seed, self.n_iter = lib, m, dsp, p, sid, seed, n_iter
        self.ring, self.ola = np.zeros((1, p.n_fft), np.float32), np.zeros((1, p.n_fft), np.float32)
        self.hx = np.zeros((1, 17, p.num_compressed_bins), np.float32)
        self.ws = np.zeros(lib.dn_workspace_bytes(dsp, 1) // 4 + 16, np.float32)
        self.hops = 0

    def push(self, hop):
        if self.hops == 0:
            self.ring[0, self.p.hop:] = hop
            self.hops = 1
            return None
        out = np.zeros((1, self.p.hop), np.float32)
        self.lib.check(self.lib.dn_stream_step(self.m, self.dsp, emu.ptr(emu.f32(hop[None])), emu.ptr(self.ring), emu.ptr(self.ola),
                                               emu.ptr(self.hx), emu.ptr(out), None, self.seed + self.hops - 1, self.sid, self.n_iter, 0.99,
                                               emu.ptr(self.ws), 1, 0, None))
        self.hops += 1
        return out[0]


def test_session_pool_on_scattered_slots_equals_stream_step_and_moves_bit_for_bit(lib, plans):
    p, dsp, m = plans["L16"]
    seed, n_iter = 9, 4
    sig = _signal(2, 7 * p.hop, 31).numpy()
    a, b = _Pool(lib, m, dsp, p, 8), _Pool(lib, m, dsp, p, 8)
    assert a.stride == record_layout(512, p.num_compressed_bins)["stride"] == 4608
    # session 0 lives in slot 6 from tick 0 on, session 1 in slot 1 from tick 2 on; after tick 3 both move to pool b, slots 0 and 7
    slot_a, slot_b, sids, born = [6, 1], [0, 7], [77, 2 ** 33 + 5], [0, 2]
    refs = [_Step(lib, m, dsp, p, sids[k], seed, n_iter) for k in range(2)]
    n_pushed = [0, 0]
    compared = 0
    for t in range(6):
        pool, slots = (a, slot_a) if t < 4 else (b, slot_b)
        if t == 4:
            b.import_(slot_b[::-1], a.export(slot_a[::-1]))
        live = [k for k in range(2) if born[k] <= t]
        for k in live:
            if born[k] == t:
                a.open([slot_a[k]], [sids[k]])
        order = live[::-1] if t % 2 else live
        hops = np.stack([sig[k, n_pushed[k] * p.hop:(n_pushed[k] + 1) * p.hop] for k in order])
        got = pool.push([slots[k] for k in order], hops, seed, n_iter)
        for r, k in enumerate(order):
            want = refs[k].push(hops[r])
            n_pushed[k] += 1
            if want is None:
                assert not got[r].any()
            else:
                assert np.array_equal(got[r], want), (t, k)
                compared += int(t >= 4 and np.abs(want).max() > 0)
    assert compared >= 3                  # hops emitted after the move
    a.destroy()
    b.destroy()


# ------------------------------------------------------------------ what is not built at this size
def test_schedules_built_for_1024_are_refused_and_the_auto_modes_resolve(lib, plans):
    p, dsp, m = plans["L16"]
    B = 2
    pipe, twin = C.c_void_p(), C.c_void_p()           # `twin` is never touched by a setter: what `pipe` has to go on computing
    lib.check(lib.dn_pipe_create(m, dsp, B, 0, C.byref(pipe)))
    lib.check(lib.dn_pipe_create(m, dsp, B, 0, C.byref(twin)))
    frames = emu.f32(0.1 * torch.randn(B, p.n_fft, generator=torch.Generator().manual_seed(4)).numpy())

    def run(h):
        hx, out = np.zeros((B, 17, p.num_compressed_bins), np.float32), np.zeros((B, p.n_fft), np.float32)
        lib.check(lib.dn_pipe_submit(h, emu.ptr(frames), emu.ptr(hx), emu.ptr(out), None, 5, 0, 4, 0.99, None))
        lib.check(lib.dn_pipe_flush(h, 4, 0.99, None))
        return out

    def same():
        a, b = run(pipe), run(twin)
        return np.abs(a).max() > 0 and np.array_equal(a, b)
    assert same()
    for call in (lambda: lib.dn_pipe_set_depth(pipe, 2), lambda: lib.dn_pipe_set_group(pipe, 2),
                 lambda: lib.dn_pipe_set_gl_schedule(pipe, DN_GL_WAVE_PER_STREAM), lambda: lib.dn_pipe_set_split(pipe, DN_SPLIT_ON)):
        assert call() == DN_ERR_UNSUPPORTED
        assert b"512" in lib.dn_last_error() and b"1024" in lib.dn_last_error()
        assert same()                                           # the pipe runs on as it was
    for mode in (DN_GL_AUTO, DN_GL_WAVE_PER_COLUMN):
        lib.check(lib.dn_pipe_set_gl_schedule(pipe, mode))
    for mode in (DN_SPLIT_AUTO, DN_SPLIT_OFF):
        lib.check(lib.dn_pipe_set_split(pipe, mode))
    lib.check(lib.dn_pipe_set_depth(pipe, 1))
    lib.check(lib.dn_pipe_set_group(pipe, 0))
    assert same()
    lib.dn_pipe_destroy(pipe)
    lib.dn_pipe_destroy(twin)

    pool = _Pool(lib, m, dsp, p, 2)
    assert lib.dn_sessions_set_schedule(pool.h, DN_SESS_TWO_LAUNCHES) == DN_ERR_UNSUPPORTED
    assert b"512" in lib.dn_last_error() and b"1024" in lib.dn_last_error()
    for mode in (DN_SESS_AUTO, DN_SESS_ONE_LAUNCH):
        lib.check(lib.dn_sessions_set_schedule(pool.h, mode))
    pool.destroy()


def test_plan_refusals_at_and_around_512(lib):
    h = C.c_void_p()
    # 80 HTK filters over 257 bins at 16 kHz leave filters without a bin of their own: the plan cannot build the pseudo-inverse
    assert lib.dn_dsp_create(C.byref(DspCfg(16000, 512, 256, 80)), None, None, None, C.byref(h)) == DN_ERR_INVALID
    assert b"rank deficient" in lib.dn_last_error() and not h.value
    # hop != n_fft / 2 and the sizes that are not built stay refused, with the built sizes named
    for cfg in (DspCfg(16000, 512, 128, 64), DspCfg(16000, 256, 128, 16), DspCfg(48000, 2048, 1024, 64)):
        assert lib.dn_dsp_create(C.byref(cfg), None, None, None, C.byref(h)) == DN_ERR_UNSUPPORTED
        msg = lib.dn_last_error()
        assert b"512" in msg and b"1024" in msg and b"1536" in msg and not h.value
