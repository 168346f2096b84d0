"""A streaming dn_pipe that changes mode while it carries a stream, on the host emulator (tests/test_emu_kernels.py has the tier's how and
why): single pushes, hop groups and single pushes again on ONE pipe against the never-reconfigured one-hop pipe, every emitted hop placed by
the model of tests/pipe_cases.py.  The gpu tier (tests/test_gpu_pipe_switch.py) runs every other switch, at batch 5 and 3 over 21 hops."""
import ctypes as C

import numpy as np
import pytest

import pipe_cases as pc
from conftest import load_golden
from test_emu_kernels import P, _run_pipe, dsp, emu, lib, make_model  # noqa: F401  (lib, dsp: the module's fixtures)
from audio_denoising_amd._lib import DnError


class EmuStream:
    """pipe_cases.run_script's driver on the C ABI: device-RNG phases, seed 11, stream id 3 as _run_pipe"""

    def __init__(self, lib, dsp, m, B, signal, n_iter):
        self.lib, self.B, self.sig, self.n_iter = lib, B, signal, n_iter
        self.pipe = C.c_void_p()
        lib.check(lib.dn_pipe_stream_create(m, dsp, B, 0, C.byref(self.pipe)))
        self.depth, self.group = 1, 0

    def close(self):
        self.lib.dn_pipe_destroy(self.pipe)

    def _hops(self, idx):
        return emu.f32(np.stack([self.sig[:self.B, h * P.hop:(h + 1) * P.hop] for h in idx]))

    def push(self, h):
        x, o = self._hops([h])[0], np.zeros((self.B, P.hop), np.float32)
        self.lib.check(self.lib.dn_pipe_stream_push(self.pipe, emu.ptr(x), 0, emu.ptr(o), 0, None, 11, 3, self.n_iter, 0.99, None))
        return [o]

    def flush(self):
        outs = []
        for _ in range(self.depth):
            o = np.zeros((self.B, P.hop), np.float32)
            self.lib.check(self.lib.dn_pipe_stream_flush(self.pipe, emu.ptr(o), 0, self.n_iter, 0.99, None))
            outs.append(o)
        return outs

    def push_group(self, idx):
        x, o = self._hops(idx), np.zeros((self.group, self.B, P.hop), np.float32)
        self.lib.check(self.lib.dn_pipe_stream_push_group(self.pipe, emu.ptr(x), self.B * P.hop, 0, emu.ptr(o), self.B * P.hop, 0, None, 0, 11, 3,
                                                          self.n_iter, 0.99, None))
        return list(o)

    def flush_group(self):
        o, valid = np.full((self.group, self.B, P.hop), np.nan, np.float32), C.c_int32(-1)
        self.lib.check(self.lib.dn_pipe_stream_flush_group(self.pipe, emu.ptr(o), self.B * P.hop, 0, C.byref(valid), None))
        return list(o), valid.value

    def set_depth(self, depth):
        self.lib.check(self.lib.dn_pipe_set_depth(self.pipe, depth))
        self.depth = depth

    def set_group(self, hops):
        self.lib.check(self.lib.dn_pipe_set_group(self.pipe, hops))
        self.group = hops

    def refuse(self, setter, value):
        with pytest.raises(DnError):
            self.lib.check(getattr(self.lib, "dn_pipe_" + setter)(self.pipe, value))

    def state(self):
        ring, ola = np.zeros((self.B, P.n_fft), np.float32), np.zeros((self.B, P.n_fft), np.float32)
        hx, frames = np.zeros((self.B, 17, P.num_compressed_bins), np.float32), C.c_uint64()
        self.lib.check(self.lib.dn_pipe_stream_get_state(self.pipe, emu.ptr(ring), emu.ptr(ola), emu.ptr(hx), None))
        self.lib.check(self.lib.dn_pipe_get_counters(self.pipe, None, C.byref(frames), None, None))
        return ring, ola, hx, frames.value


def test_single_pushes_then_groups_then_single_pushes_on_one_pipe(lib, dsp):
    """Three single pushes and a flush; set_group(2): a group and its flush, then two groups and their flush -- *hops_valid is 2 both times, the
    ring was primed by the single pushes; the refused wave-per-column schedule leaves the stream alone; set_group(0), two pushes, a flush.
    Eleven hops = frames 0 .. 9: every hop the never-reconfigured one-hop pipe's bit for bit or an exact zero where the header says so, every
    frame once, the same ring, overlap-add line, hx and frame count at the end.
    (The flush directly behind the FIRST group is where the host's count of primed hops shows: behind a second group it no longer matters.  No
    depth-2 segment: without one this test already takes 18.9 s where the longest pipe test of test_emu_kernels.py, the deep pipe at depth 2,
    takes 13.2 s on the same machine; depth 3 after single pushes runs in the gpu tier.)"""
    from audio_denoising_amd._lib import DN_GL_WAVE_PER_COLUMN
    sig = load_golden("stream_S.npz")["signal"]
    B, n_iter, F = 2, 3, 10
    assert sig.shape[1] == (F + 1) * P.hop
    m = make_model(lib, 5)
    a = _run_pipe(lib, dsp, m, DN_GL_WAVE_PER_COLUMN, B, F, {"signal": sig}, stream=True, n_iter=n_iter)          # F + 1 pushes, one flush, the state
    E = [a[f + 2] for f in range(F)]
    assert not a[0].any() and not a[1].any() and not E[0].any() and all(e.any() for e in E[1:])
    script = [("push",), ("push",), ("push",), ("flush",),
              ("set_group", 2), ("push_group",), ("flush_group", 2),
              ("refuse", "set_gl_schedule", DN_GL_WAVE_PER_COLUMN), ("push_group",), ("push_group",), ("flush_group", 2),
              ("set_group", 0), ("push",), ("push",), ("flush",), ("state", "end")]
    s = EmuStream(lib, dsp, m, B, sig, n_iter)
    try:
        labels, hops, kept = pc.run_script(script, s, pc.EmitModel(P.n_fft // P.hop - 1))
    finally:
        s.close()
        lib.dn_model_destroy(m)
    pc.check_emitted(labels, hops, E, range(F))
    (ring, ola, hx, frames), delivered = kept["end"]
    assert delivered == F + 1 and frames == F
    for x, y in zip(a[-3:], (ring, ola, hx)):
        assert np.array_equal(x, y)
