"""The ragged clip call (dn_clip_process_ragged: n_hops[b] hops of stream b, clips of different lengths in one call) on the host emulation of the
kernel sources.  For every stream with hops the call is defined as "n_hops[b] calls of dn_stream_step with B = 1, bit for bit", so the yardstick is
the emulated dn_stream_step run on that stream's rows alone with stream_id0 + b and the seeds SEED + frame0[b] + i, and every comparison is
np.array_equal on the hops out, ring, ola and hx -- no tolerance.  Cases and geometries: tests/clip_ragged_cases.py.

Every workspace is handed over full of NaNs and exactly dn_clip_ragged_workspace_bytes long, with a canary region behind it; one spare hop of
canary sits behind hops_out.  Both must come back untouched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import clip_ragged_cases as cases  # noqa: E402
from audio_denoising_amd._lib import DspCfg, ModelCfg  # noqa: E402
from clip_ragged_cases import (DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM, DN_ERR_INVALID, DN_ERR_UNSUPPORTED, DN_OK, DN_PHASE_FROM_INPUT,  # noqa: E402
                               EMU_CASES, EMU_HOPS, SEED, SID0, WARM)
from oracle import dsp_ref, pipeline_ref  # noqa: E402

GEOS = {"S": pipeline_ref.PARAMS_S, "R1": pipeline_ref.PARAMS_R1, "L16": pipeline_ref.Params(16000, 512, 256, 64)}
N_ITER = cases.EMU_N_ITER
CANARY = np.float32(-12345.0)
CANARY_FLOATS = 256


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def plans(lib):
    d = {}
    w = np.fromfile(os.path.join(GOLDEN, "weights_dari_tult.bin"), dtype=np.float32)
    for tag, p in GEOS.items():
        dsp, m = C.c_void_p(), C.c_void_p()
        fb = emu.f32(dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate).numpy())
        lib.check(lib.dn_dsp_create(C.byref(DspCfg(p.sample_rate, p.n_fft, p.hop, p.n_mels)), emu.ptr(fb), None,
                                    emu.ptr(emu.f32(torch.hann_window(p.n_fft).numpy())), C.byref(dsp)))
        lib.check(lib.dn_model_create(emu.ptr(w), w.size, C.byref(ModelCfg(p.num_compressed_bins, 1, 4, 17, 3, 2, 1, 6)), C.byref(m)))
        d[tag] = (p, dsp, m)
    yield d
    for _, dsp, m in d.values():
        lib.dn_dsp_destroy(dsp)
        lib.dn_model_destroy(m)


class _State:
    """ring, ola, hx of some streams"""

    def __init__(self, ring, ola, hx):
        self.ring, self.ola, self.hx = ring, ola, hx

    @staticmethod
    def stack(rows):
        return _State(*(np.ascontiguousarray(np.concatenate([getattr(r, k) for r in rows])) for k in ("ring", "ola", "hx")))

    def copy(self):
        return _State(self.ring.copy(), self.ola.copy(), self.hx.copy())

    def row(self, b):
        return _State(self.ring[b:b + 1], self.ola[b:b + 1], self.hx[b:b + 1])

    def same(self, o):
        return np.array_equal(self.ring, o.ring) and np.array_equal(self.ola, o.ola) and np.array_equal(self.hx, o.hx)


def _step(lib, plan, st, hop_in, seed, sid, flags=0, init=None):
    """one dn_stream_step with B = 1 on `st`"""
    p, dsp, m = plan
    ws = np.zeros(lib.dn_workspace_bytes_ex(dsp, 1, flags) // 4 + 16, np.float32)
    out = np.full((1, p.hop), 7.0, np.float32)
    lib.check(lib.dn_stream_step(m, dsp, emu.ptr(emu.f32(hop_in)), emu.ptr(st.ring), emu.ptr(st.ola), emu.ptr(st.hx), emu.ptr(out), emu.ptr(init),
                                 seed, sid, N_ITER, 0.99, emu.ptr(ws), 1, flags, None))
    return out


@pytest.fixture(scope="module")
def warmed(lib, plans):
    """(tag, b) -> (the stream's signal (1, (1 + WARM[b] + EMU_HOPS) hop), its state after the priming hop and WARM[b] hops): computed once"""
    cache = {}

    def get(tag, b):
        if (tag, b) not in cache:
            plan = plans[tag]
            p = plan[0]
            sig = cases.signal(b + 1, (1 + WARM[b] + EMU_HOPS) * p.hop, 300 + p.n_fft + b)[b:b + 1].numpy()
            st = _State(np.zeros((1, p.n_fft), np.float32), np.zeros((1, p.n_fft), np.float32), np.zeros((1, 17, p.num_compressed_bins), np.float32))
            st.ring[:, p.hop:] = sig[:, :p.hop]
            for k in range(WARM[b]):
                _step(lib, plan, st, sig[:, (1 + k) * p.hop:(2 + k) * p.hop], SEED + k, SID0 + b)
            assert np.abs(st.ola).max() > 1e-3 and np.abs(st.hx).max() > 1e-3
            cache[tag, b] = (sig, st)
        return cache[tag, b]
    return get


def _inits(p, F):
    """packed injected phases [F][3][K] re, im"""
    z = torch.rand(F, 3, p.n_stft, dtype=torch.complex64, generator=torch.Generator().manual_seed(42))
    return emu.f32(torch.view_as_real(z).numpy())


@pytest.fixture(scope="module")
def yard(lib, plans, warmed):
    """(tag, b, variant, first frame of the stream in the call) -> (the stream's hops in (1, EMU_HOPS hop) float32 or int16, [(state, hops out so far)
    after 1 .. EMU_HOPS steps of dn_stream_step from the warmed state]): the yardstick, computed once per key and only read"""
    cache = {}

    def get(tag, b, variant="plain", off=0, F=0):
        key = (tag, b, variant, off if variant == "init" else 0)
        if key not in cache:
            plan = plans[tag]
            p = plan[0]
            sig, st = warmed(tag, b)
            st = st.copy()
            hops = sig[:, (1 + WARM[b]) * p.hop:]
            fed = hops
            if variant == "s16":
                hops = cases.to_pcm(hops)
                fed = hops.astype(np.float32) / np.float32(32767.0)                    # app3.py:172
            flags = DN_PHASE_FROM_INPUT if variant == "phin" else 0
            packed = _inits(p, F) if variant == "init" else None
            after, outs = [], []
            for i in range(EMU_HOPS):
                init = np.ascontiguousarray(packed[off + i:off + i + 1]) if packed is not None and off + i < F else None
                outs.append(_step(lib, plan, st, fed[:, i * p.hop:(i + 1) * p.hop], SEED + WARM[b] + i, SID0 + b, flags, init))
                ref = np.concatenate(outs, axis=1)
                after.append((st.copy(), cases.pcm_out(ref) if variant == "s16" else ref))
            cache[key] = (hops, after)
        return cache[key]
    return get


def _ragged(lib, plan, st, packed_in, n_hops, frame0, flags=0, init=None, seed=SEED, sid0=SID0):
    """dn_clip_process_ragged on `st` (B rows); returns (rc, hops out, workspace): the workspace exactly as long as the library asks, full of NaNs,
    canaries behind it and behind the hops out"""
    p, dsp, m = plan
    B, F = len(n_hops), int(sum(n_hops))
    need = lib.dn_clip_ragged_workspace_bytes(dsp, B, F, flags)
    assert need > 0 and need % 256 == 0
    ws = np.full(need // 4 + CANARY_FLOATS, np.nan, np.float32)
    ws[need // 4:] = CANARY
    s16 = packed_in.dtype == np.int16
    out = np.full((F + 1) * p.hop, 7, packed_in.dtype)
    rc = lib.dn_clip_process_ragged(m, dsp, emu.ptr(packed_in), int(s16), emu.ptr(st.ring), emu.ptr(st.ola), emu.ptr(st.hx), emu.ptr(out), int(s16),
                                    emu.ptr(init), seed, sid0, (C.c_int32 * B)(*n_hops), None if frame0 is None else (C.c_uint64 * B)(*frame0),
                                    N_ITER, 0.99, emu.ptr(ws), B, flags, None)
    assert (ws[need // 4:] == CANARY).all(), "the call wrote behind its workspace"
    assert (out[F * p.hop:] == 7).all(), "the call wrote behind hops_out"
    return rc, out[:F * p.hop], ws[:need // 4]


@pytest.mark.parametrize("case", sorted(EMU_CASES))
def test_ragged_call_equals_stream_steps_per_stream(lib, plans, warmed, yard, case):
    tag, n_hops, flags, variant = EMU_CASES[case]
    plan = plans[tag]
    p = plan[0]
    B, F, off = len(n_hops), sum(n_hops), cases.offsets(n_hops)
    assert F <= 10 and max(n_hops) <= EMU_HOPS
    start = _State.stack([warmed(tag, b)[1] for b in range(B)])
    refs = [yard(tag, b, variant, off[b], F) if n_hops[b] else None for b in range(B)]
    packed = np.concatenate([refs[b][0][0, :n_hops[b] * p.hop] for b in range(B) if n_hops[b]])
    st = start.copy()
    if variant == "phin":
        flags |= DN_PHASE_FROM_INPUT
        plain = lib.dn_clip_ragged_workspace_bytes(plan[1], B, F, 0)
        rows = lib.dn_clip_workspace_bytes_ex(plan[1], 1, F, DN_PHASE_FROM_INPUT) - lib.dn_clip_workspace_bytes(plan[1], 1, F)
        assert rows >= F * 3 * p.n_stft * 8 and lib.dn_clip_ragged_workspace_bytes(plan[1], B, F, flags) == plain + rows
    rc, out, _ = _ragged(lib, plan, st, packed, n_hops, WARM[:B], flags, _inits(p, F) if variant == "init" else None)
    assert rc == DN_OK, lib.dn_last_error()
    assert out.dtype == packed.dtype
    for b in range(B):
        if n_hops[b] == 0:          # left exactly as it was
            assert st.row(b).same(start.row(b)), b
            continue
        want, want_out = refs[b][1][n_hops[b] - 1]
        assert np.array_equal(out[off[b] * p.hop:off[b + 1] * p.hop], want_out[0]), b
        assert st.row(b).same(want), b
        assert np.abs(want_out.astype(np.float32)).max() > (30 if variant == "s16" else 1e-3)


def test_a_shared_seed_base_would_fail(lib, plans, warmed, yard):
    """the case table's claim: with frame0 left out (zeros) the streams draw other phases than their yardsticks"""
    plan = plans["L16"]
    p = plan[0]
    n_hops = (2, 1, 3)
    start = _State.stack([warmed("L16", b)[1] for b in range(3)])
    packed = np.concatenate([yard("L16", b)[0][0, :n_hops[b] * p.hop] for b in range(3)])
    rc, out, _ = _ragged(lib, plan, start.copy(), packed, n_hops, None)
    assert rc == DN_OK
    assert not np.array_equal(out[3 * p.hop:], yard("L16", 2)[1][2][1][0])          # (a stream's first hop out is its old line alone: take three)


def test_equal_lengths_give_the_uniform_call(lib, plans, warmed, yard):
    plan = plans["L16"]
    p, dsp, m = plan
    B, N = 3, 2
    start = _State.stack([warmed("L16", b)[1] for b in range(B)])
    hops_in = np.ascontiguousarray(np.concatenate([yard("L16", b)[0][:, :N * p.hop] for b in range(B)]))
    want = start.copy()
    ws = np.full(lib.dn_clip_workspace_bytes(dsp, B, N) // 4, np.nan, np.float32)
    want_out = np.zeros((B, N * p.hop), np.float32)
    lib.check(lib.dn_clip_process(m, dsp, emu.ptr(hops_in), 0, emu.ptr(want.ring), emu.ptr(want.ola), emu.ptr(want.hx), emu.ptr(want_out), 0, None,
                                  SEED + 5, SID0, N_ITER, 0.99, emu.ptr(ws), B, N, 0, None))
    st = start.copy()
    rc, out, _ = _ragged(lib, plan, st, hops_in.reshape(-1), (N,) * B, (5,) * B)
    assert rc == DN_OK
    assert np.array_equal(out, want_out.reshape(-1)) and st.same(want)


def test_no_hops_at_all_is_ok_and_writes_nothing(lib, plans, warmed):
    p, dsp, m = plans["S"]
    start = _State.stack([warmed("S", b)[1] for b in range(2)])
    st = start.copy()
    n = (C.c_int32 * 2)(0, 0)
    assert lib.dn_clip_process_ragged(m, dsp, None, 0, emu.ptr(st.ring), emu.ptr(st.ola), emu.ptr(st.hx), None, 0, None, SEED, SID0, n, None, N_ITER,
                                      0.99, None, 2, 0, None) == DN_OK
    assert st.same(start)
    assert lib.dn_clip_ragged_workspace_bytes(dsp, 2, 0, 0) == 0


def test_workspace_size(lib, plans):
    p, dsp, m = plans["S"]
    for B, F in ((1, 1), (4, 6), (63, 6), (64, 6), (1000, 10)):
        table = (((4 * (B + 1) + 7) // 8 * 8 + 8 * B) + 255) // 256 * 256          # off [B + 1] int32 to 8 bytes, frame0 [B] uint64, to 256 bytes
        assert lib.dn_clip_ragged_workspace_bytes(dsp, B, F, 0) == table + lib.dn_clip_workspace_bytes(dsp, 1, F), (B, F)
    assert lib.dn_clip_ragged_workspace_bytes(dsp, 3, cases.MAX_FRAMES, 0) > 0
    for kw in (dict(d=None), dict(B=0), dict(B=-1), dict(F=0), dict(F=-1), dict(F=cases.MAX_FRAMES + 1), dict(F=2 ** 40), dict(flags=64)):
        a = dict(d=dsp, B=2, F=5, flags=0)
        a.update(kw)
        assert lib.dn_clip_ragged_workspace_bytes(a["d"], a["B"], a["F"], a["flags"]) == 0, kw


def test_refusals_leave_everything_untouched(lib, plans, warmed, yard):
    plan = plans["S"]
    p, dsp, m = plan
    n_ok = (2, 0, 1)
    B, F = 3, 3
    start = _State.stack([warmed("S", b)[1] for b in range(B)])
    st = start.copy()
    hops_in = np.concatenate([yard("S", b)[0][0, :n_ok[b] * p.hop] for b in range(B) if n_ok[b]])
    out = np.zeros(F * p.hop, np.float32)
    need = lib.dn_clip_ragged_workspace_bytes(dsp, B, F, DN_PHASE_FROM_INPUT)
    ws = np.full(need // 4, np.nan, np.float32)
    init = _inits(p, F)

    def call(n_hops=n_ok, B=B, flags=0, ws_=ws, ring=st.ring, hops=hops_in, out_=out, init_=None, handles=(dsp, m), n_null=False):
        n = None if n_null else (C.c_int32 * len(n_hops))(*n_hops)
        return lib.dn_clip_process_ragged(handles[1], handles[0], emu.ptr(hops), 0, emu.ptr(ring), emu.ptr(st.ola), emu.ptr(st.hx), emu.ptr(out_), 0,
                                          emu.ptr(init_), SEED, SID0, n, (C.c_uint64 * 3)(*WARM[:3]), N_ITER, 0.99, emu.ptr(ws_), B, flags, None)
    refused = (dict(B=0), dict(B=-2), dict(n_null=True), dict(n_hops=(2, -1, 1)), dict(n_hops=(cases.MAX_FRAMES, 1, 0)),
               dict(n_hops=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), dict(flags=DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM), dict(flags=64),
               dict(flags=DN_PHASE_FROM_INPUT, init_=init), dict(ws_=None), dict(ring=None), dict(hops=None), dict(out_=None),
               dict(handles=(None, m)), dict(handles=(dsp, None)))
    for kw in refused:
        assert call(**kw) == DN_ERR_INVALID, kw
        assert lib.dn_last_error(), kw
        assert st.same(start) and not out.any() and np.isnan(ws).all(), kw
    # the wavefront-per-stream chains are built for n_fft 1024: refused at 512 and 1536, the message names the size
    for tag in ("L16", "R1"):
        q, dsp_q, m_q = plans[tag]
        start2 = _State.stack([warmed(tag, b)[1] for b in range(2)])
        st2 = start2.copy()
        h2, o2 = np.zeros(2 * q.hop, np.float32), np.zeros(2 * q.hop, np.float32)
        w2 = np.full(lib.dn_clip_ragged_workspace_bytes(dsp_q, 2, 2, 0) // 4, np.nan, np.float32)
        rc = lib.dn_clip_process_ragged(m_q, dsp_q, emu.ptr(h2), 0, emu.ptr(st2.ring), emu.ptr(st2.ola), emu.ptr(st2.hx), emu.ptr(o2), 0, None, SEED, SID0,
                                        (C.c_int32 * 2)(1, 1), None, N_ITER, 0.99, emu.ptr(w2), 2, DN_CLIP_GL_PER_STREAM, None)
        assert rc == DN_ERR_UNSUPPORTED and b"1024" in lib.dn_last_error()
        assert st2.same(start2) and not o2.any() and np.isnan(w2).all()
    assert call() == DN_OK and out.any() and not st.same(start)          # the same arguments, valid: the call goes through
