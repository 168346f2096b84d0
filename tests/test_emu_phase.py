"""Input-phase mode (DN_PHASE_FROM_INPUT) on the host emulation of the kernel sources (tests/test_emu_kernels.py has the tier's how and why), and
the parts of it that need no kernel at all.  tests/phase_cases.py holds the references, the runner of every entry point and the bounds.

  1. dn_stft_phasors against float64, weighted by magnitude, at every n_fft and two windows; unit modulus; zero, constant and impulse frames.
  2. The flag equals injected phasors, bit for bit, at every entry point: a call with the flag against the same call without it fed
     init_angles = dn_stft_phasors(frame).  The emulator runs a work-item per OS thread: B = 2, two iterations, two or three frames.
  4. Flag plus init_angles is refused with nothing changed; the _ex sizes; NaN workspaces (every run hands one over); default-mode bits after an
     input-mode call on the same workspace.
  (3., the fused hop against float64 through the Python front ends, is the gpu tier's; its seed table is derived again here.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import dsp_cases as dc  # noqa: E402
import phase_cases as pcs  # noqa: E402

B, N_ITER = 2, 2


@pytest.fixture(scope="module")
def run():
    r = pcs.Runner(emu.load())
    yield r
    r.close()


# ------------------------------------------------------------------ 1. phasors alone
@pytest.mark.parametrize("window", pcs.WINDOWS)
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_phasors_match_float64(run, n_fft, window):
    plan = run.plan(n_fft, window)
    w = plan[3]
    special = np.zeros((3, n_fft), np.float32)            # an all-zero frame, a constant frame, a one-sample impulse
    special[1] = 0.37
    special[2, n_fft // 3] = -2.5
    for name, frames in (("noise", dc.noise((3, n_fft), 500 + n_fft)), ("special", special)):
        u = dc.cplx(run.phasors(plan, frames))
        X64 = pcs.spectrum64(frames, n_fft, w)
        assert np.abs(np.abs(u) - 1.0).max() <= pcs.ULP_BAND, name
        rows = range(3) if name == "noise" else (1, 2)
        for b in rows:
            e, e_ref = pcs.weighted_error(u[b], X64[b]), pcs.weighted_error(pcs.phasors32(frames, n_fft, w)[b], X64[b])
            print(f"phasors n_fft {n_fft} {window} {name}[{b}]: weighted error {e:.3e}, fp32 torch {e_ref:.3e}, ratio {e / e_ref:.2f}")
            assert e <= pcs.R_PHASOR * e_ref, (name, b, e, e_ref)
        if name == "special":
            assert np.array_equal(u[0], np.ones_like(u[0])), "an all-zero frame gives exactly (1, 0) everywhere"


def test_phasors_without_the_analysis_flags(run):
    """flags as dn_stft: 0 = the STFT of the raw frame"""
    plan = run.plan(1024, "asym")
    frames = dc.noise((2, 1024), 77)
    from oracle import dsp_np64
    X64 = dsp_np64.stft(frames, 1024, 512, plan[3])
    u = dc.cplx(run.phasors(plan, frames, flags=0))
    assert pcs.weighted_error(u, X64) <= 1e-5


# ------------------------------------------------------------------ 2. the flag equals injected phasors
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_process_frame_and_stream_steps(run, n_fft):
    plan = run.plan(n_fft, "asym")
    p = plan[0]
    sig = pcs.stream_signal(B, n_fft, 4)
    frames = pcs.stream_frames(sig, p, 4)
    hx0 = 0.1 * dc.noise((B, 17, p.num_compressed_bins), 9)
    for n_iter in (0, N_ITER):
        pcs.identity(run, plan, frames[:1], lambda inits: run.run_frame(plan, frames[0], hx0, n_iter, inits))
    a = pcs.identity(run, plan, frames[:3], lambda inits: run.run_steps(plan, sig, 3, N_ITER, inits))
    assert np.abs(a["out"][:, p.hop:]).max() > 1e-3


@pytest.mark.parametrize("gl", [pcs.DN_CLIP_GL_PER_COLUMN, pcs.DN_CLIP_GL_PER_STREAM])
@pytest.mark.parametrize("N", [1, 2, 4])
def test_clip_1024(run, N, gl):
    plan = run.plan(1024)
    sig = pcs.stream_signal(B if N < 4 else 1, 1024, N)
    if N == 2:
        sig = pcs.to_s16(sig)                             # int16 in and out
    frames = pcs.stream_frames(sig, plan[0], N)
    a = pcs.identity(run, plan, frames, lambda inits: run.run_clip(plan, sig, N, N_ITER, inits, gl))
    steps = run.run_steps(plan, pcs.as_float(sig), N, N_ITER)
    if sig.dtype != np.int16:
        assert all(np.array_equal(a[k], steps[k]) for k in a), "dn_clip_process is N calls of dn_stream_step in input-phase mode too"


@pytest.mark.parametrize("n_fft", [512, 1536])
def test_clip_other_sizes(run, n_fft):
    plan = run.plan(n_fft, "asym")
    sig = pcs.stream_signal(1, n_fft, 2)
    pcs.identity(run, plan, pcs.stream_frames(sig, plan[0], 2), lambda inits: run.run_clip(plan, sig, 2, N_ITER, inits))


@pytest.mark.parametrize("mode", list(pcs.MODES))
def test_frame_pipe_1024(run, mode):
    plan = run.plan(1024)
    F = 3
    frames = np.stack(pcs.stream_frames(pcs.stream_signal(B, 1024, F, seed=5), plan[0], F))
    a = pcs.identity(run, plan, list(frames), lambda inits: run.run_pipe_frames(plan, frames, N_ITER, pcs.MODES[mode], inits))
    hx = np.zeros((B, 17, plan[0].num_compressed_bins), np.float32)
    first = run.run_frame(plan, frames[0], hx, N_ITER)
    assert np.array_equal(a["out"][0], first["out"]), "the pipe's first frame is dn_process_frame's"


@pytest.mark.parametrize("mode", list(pcs.MODES))
def test_stream_pipe_1024(run, mode):
    plan = run.plan(1024)
    pushes = 4
    sig = pcs.stream_signal(B, 1024, pushes - 1, seed=6)
    a = pcs.identity(run, plan, pcs.stream_frames(sig, plan[0], pushes - 1),
                     lambda inits: run.run_pipe_stream(plan, sig, pushes, N_ITER, pcs.MODES[mode], inits))
    assert int(a["frames"]) == pushes - 1
    # the samples are dn_stream_step's, later: every hop the steps emit appears among the pipe's, in order
    steps = run.run_steps(plan, sig, pushes - 1, N_ITER)["out"].reshape(B, pushes - 1, -1)
    live = [h for h in a["out"] if h.any()]
    assert len(live) >= pushes - 2 and all(np.array_equal(h, steps[:, 1 + i]) for i, h in enumerate(live[:pushes - 2]))


@pytest.mark.parametrize("n_fft", [512, 1536])
@pytest.mark.parametrize("mode", pcs.MODES_ANY_NFFT)
def test_pipes_other_sizes(run, n_fft, mode):
    plan = run.plan(n_fft, "asym")
    sig = pcs.stream_signal(B, n_fft, 2, seed=8)
    frames = pcs.stream_frames(sig, plan[0], 2)
    pcs.identity(run, plan, frames, lambda inits: run.run_pipe_frames(plan, np.stack(frames), N_ITER, pcs.MODES[mode], inits))
    pcs.identity(run, plan, frames, lambda inits: run.run_pipe_stream(plan, sig, 3, N_ITER, pcs.MODES[mode], inits))


@pytest.mark.parametrize("n_fft,schedule", [(1024, 1), (1024, 2), (512, 1), (1536, 1)])
def test_session_pool(run, n_fft, schedule):
    plan = run.plan(n_fft)
    sig = pcs.stream_signal(B, n_fft, 3, seed=9)
    a = pcs.identity(run, plan, pcs.stream_frames(sig, plan[0], 3), lambda inits: run.run_sessions(plan, sig, 4, N_ITER, schedule, inits))
    steps = run.run_steps(plan, sig, 3, N_ITER)["out"].reshape(B, 3, -1)
    assert not a["out"][0].any() and all(np.array_equal(a["out"][1 + h], steps[:, h]) for h in range(3)), "a session's samples are dn_stream_step's"


def test_session_records_cross_the_two_modes(run):
    """a record exported from a pool in either mode imports into a pool in the other"""
    lib = run.lib
    plan = run.plan(1024)
    p = plan[0]
    sig = pcs.stream_signal(1, 1024, 2, seed=10)
    ids = np.zeros(1, np.int32)
    idp = ids.ctypes.data_as(C.c_void_p)

    def pool(flags):
        h = C.c_void_p()
        lib.check(lib.dn_sessions_create(plan[2], plan[1], 1, flags, C.byref(h)))
        return h

    def push(h, k):
        hin, out = emu.f32(sig[:, k * p.hop:(k + 1) * p.hop]), np.zeros((1, p.hop), np.float32)
        lib.check(lib.dn_sessions_push(h, idp, 1, emu.ptr(hin), 0, emu.ptr(out), 0, None, 11, N_ITER, 0.99, None))
        return out

    a, b = pool(pcs.DN_PHASE_FROM_INPUT), pool(0)
    try:
        assert lib.dn_sessions_record_bytes(a) == lib.dn_sessions_record_bytes(b)
        lib.check(lib.dn_sessions_open(a, idp, 1, None, None))
        push(a, 0), push(a, 1)
        rec = np.zeros(lib.dn_sessions_record_bytes(a), np.uint8)
        lib.check(lib.dn_sessions_export(a, idp, 1, emu.ptr(rec), None))
        lib.check(lib.dn_sessions_import(b, idp, 1, emu.ptr(rec), None, None))
        rec_b = np.zeros_like(rec)
        lib.check(lib.dn_sessions_export(b, idp, 1, emu.ptr(rec_b), None))
        assert np.array_equal(rec, rec_b)
        out_b = push(b, 2)                                # the default-mode pool goes on from the input-mode pool's state
        assert np.array_equal(out_b, push(a, 2)), "the emitted hop is the overlap-add line: it does not depend on the mode of the push that emits it"
        lib.check(lib.dn_sessions_export(b, idp, 1, emu.ptr(rec_b), None))
        lib.check(lib.dn_sessions_import(a, idp, 1, emu.ptr(rec_b), None, None))          # ... and back
    finally:
        lib.dn_sessions_destroy(a)
        lib.dn_sessions_destroy(b)


# ------------------------------------------------------------------ 4. errors and sizes
def test_ex_sizes(run):
    lib = run.lib
    for n_fft in pcs.N_FFTS:
        d = run.plan(n_fft)[1]
        K = n_fft // 2 + 1
        for Bn in (1, 3, 67):
            base = lib.dn_workspace_bytes(d, Bn)
            assert lib.dn_workspace_bytes_ex(d, Bn, 0) == base == lib.dn_workspace_bytes_ex(d, Bn, pcs.DN_CONV_BF16)
            with_flag = lib.dn_workspace_bytes_ex(d, Bn, pcs.DN_PHASE_FROM_INPUT)
            assert with_flag >= base + Bn * 3 * K * 8 and with_flag % 256 == 0 and with_flag < base + Bn * 3 * K * 8 + 256
            for N in (1, 4):
                cbase = lib.dn_clip_workspace_bytes(d, Bn, N)
                assert lib.dn_clip_workspace_bytes_ex(d, Bn, N, 0) == cbase == lib.dn_clip_workspace_bytes_ex(d, Bn, N, pcs.DN_CLIP_GL_PER_STREAM)
                cflag = lib.dn_clip_workspace_bytes_ex(d, Bn, N, pcs.DN_PHASE_FROM_INPUT | pcs.DN_CLIP_GL_PER_COLUMN)
                assert cflag >= cbase + Bn * N * 3 * K * 8 and cflag % 256 == 0
        assert lib.dn_workspace_bytes_ex(d, 0, pcs.DN_PHASE_FROM_INPUT) == 0 and lib.dn_workspace_bytes_ex(None, 2, 0) == 0
        assert lib.dn_workspace_bytes_ex(d, 2, 64) == 0 and lib.dn_clip_workspace_bytes_ex(d, 2, 2, 64) == 0


def test_flag_plus_init_angles_is_refused_and_changes_nothing(run):
    lib = run.lib
    plan = run.plan(1024)
    p, d, m, _ = plan
    FL = pcs.DN_PHASE_FROM_INPUT
    sig = pcs.stream_signal(B, 1024, 3, seed=12)
    init = np.ones((B, 4, 3, p.n_stft, 2), np.float32)
    ip = emu.ptr(init)
    seven = lambda *s: np.full(s, 7.0, np.float32)  # noqa: E731
    fr, hx, out = emu.f32(sig[:, :p.n_fft]), seven(B, 17, p.num_compressed_bins), seven(B, p.n_fft)
    ring, ola, hop_out = seven(B, p.n_fft), seven(B, p.n_fft), seven(B, 4 * p.hop)
    ws = seven(lib.dn_clip_workspace_bytes_ex(d, B, 4, FL) // 4)
    state = (hx, out, ring, ola, hop_out, ws)

    def refused(rc):
        assert rc == pcs.DN_ERR_INVALID and b"init_angles" in lib.dn_last_error()
        assert all((a == 7.0).all() for a in state)

    refused(lib.dn_process_frame(m, d, emu.ptr(fr), emu.ptr(hx), emu.ptr(out), None, ip, 11, 3, N_ITER, 0.99, emu.ptr(ws), B, FL, None))
    refused(lib.dn_stream_step(m, d, emu.ptr(fr), emu.ptr(ring), emu.ptr(ola), emu.ptr(hx), emu.ptr(hop_out), ip, 11, 3, N_ITER, 0.99,
                               emu.ptr(ws), B, FL, None))
    refused(lib.dn_clip_process(m, d, emu.ptr(fr), 0, emu.ptr(ring), emu.ptr(ola), emu.ptr(hx), emu.ptr(hop_out), 0, ip, 11, 3, N_ITER, 0.99,
                                emu.ptr(ws), B, 2, FL | pcs.DN_CLIP_GL_PER_COLUMN, None))
    # unknown bits stay refused beside the new one
    assert lib.dn_process_frame(m, d, emu.ptr(fr), emu.ptr(hx), emu.ptr(out), None, None, 11, 3, N_ITER, 0.99, emu.ptr(ws), B, FL | 64, None) \
        == pcs.DN_ERR_INVALID
    pipe = C.c_void_p()
    assert lib.dn_pipe_create(m, d, B, FL | 64, C.byref(pipe)) == pcs.DN_ERR_INVALID
    assert lib.dn_sessions_create(m, d, B, 16, C.byref(pipe)) == pcs.DN_ERR_INVALID

    def counters(h):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_int32()
        lib.check(lib.dn_pipe_get_counters(h, C.byref(a), C.byref(b), C.byref(c), None))
        return a.value, b.value, c.value

    # a pipe carries the flag from create: frame mode, single hops and groups
    lib.check(lib.dn_pipe_create(m, d, B, FL, C.byref(pipe)))
    try:
        refused(lib.dn_pipe_submit(pipe, emu.ptr(fr), emu.ptr(hx), emu.ptr(out), ip, 11, 3, N_ITER, 0.99, None))
        lib.check(lib.dn_pipe_set_group(pipe, 2))
        refused(lib.dn_pipe_submit_group(pipe, emu.ptr(fr), 0, emu.ptr(hx), emu.ptr(out), 0, ip, 0, 11, 3, 1, N_ITER, 0.99, None))
        assert counters(pipe) == (0, 0, 0)
    finally:
        lib.dn_pipe_destroy(pipe)
    # ... and streaming
    lib.check(lib.dn_pipe_stream_create(m, d, B, FL, C.byref(pipe)))
    try:
        hin = emu.f32(sig[:, :2 * p.hop])
        refused(lib.dn_pipe_stream_push(pipe, emu.ptr(hin), 0, emu.ptr(hop_out), 0, ip, 11, 3, N_ITER, 0.99, None))
        lib.check(lib.dn_pipe_set_group(pipe, 2))
        refused(lib.dn_pipe_stream_push_group(pipe, emu.ptr(hin), B * p.hop, 0, emu.ptr(hop_out), B * p.hop, 0, ip, 0, 11, 3, N_ITER, 0.99, None))
        assert counters(pipe) == (0, 0, 0)
        got = [np.ones((B, p.n_fft), np.float32), np.ones((B, p.n_fft), np.float32), np.ones((B, 17, p.num_compressed_bins), np.float32)]
        lib.check(lib.dn_pipe_stream_get_state(pipe, emu.ptr(got[0]), emu.ptr(got[1]), emu.ptr(got[2]), None))
        assert not any(g.any() for g in got)
    finally:
        lib.dn_pipe_destroy(pipe)
    # a session pool likewise
    pool = C.c_void_p()
    lib.check(lib.dn_sessions_create(m, d, B, FL, C.byref(pool)))
    try:
        ids = np.arange(B, dtype=np.int32)
        idp = ids.ctypes.data_as(C.c_void_p)
        lib.check(lib.dn_sessions_open(pool, idp, B, None, None))
        refused(lib.dn_sessions_push(pool, idp, B, emu.ptr(emu.f32(sig[:, :p.hop])), 0, emu.ptr(hop_out), 0, ip, 11, N_ITER, 0.99, None))
        f, n = C.c_uint64(9), C.c_int32(9)
        lib.check(lib.dn_sessions_get_counters(pool, 0, C.byref(f), C.byref(n), None))
        assert (f.value, n.value) == (0, 0)
    finally:
        lib.dn_sessions_destroy(pool)


def test_default_mode_bits_after_an_input_mode_call_on_the_same_workspace(run):
    lib = run.lib
    plan = run.plan(1024)
    p, d = plan[0], plan[1]
    frames = dc.noise((B, 1024), 31, dc.HOP_LEVEL)
    hx0 = np.zeros((B, 17, p.num_compressed_bins), np.float32)
    inj = [np.ascontiguousarray(pcs.pack(np.exp(1j * dc.noise((B, p.n_stft, 3), 32))))]
    ws = np.full(lib.dn_workspace_bytes_ex(d, B, pcs.DN_PHASE_FROM_INPUT) // 4, np.nan, np.float32)
    before = run.run_frame(plan, frames, hx0, N_ITER, inj, ws=ws)
    flagged = run.run_frame(plan, frames, hx0, N_ITER, None, ws=ws)
    after = run.run_frame(plan, frames, hx0, N_ITER, inj, ws=ws)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert not np.array_equal(before["out"], flagged["out"]) and np.array_equal(before["resid"], flagged["resid"])
    assert np.array_equal(before["hx"], flagged["hx"]), "the phase source reaches neither the mel residual nor hx"
    # the same for a clip workspace, the device generator's phases in default mode
    sig = pcs.stream_signal(1, 1024, 2, seed=33)
    cws = np.full(lib.dn_clip_workspace_bytes_ex(d, 1, 2, pcs.DN_PHASE_FROM_INPUT) // 4, np.nan, np.float32)
    plain = lambda: _clip_default(run, plan, sig, cws)  # noqa: E731
    a = plain()
    run.run_clip(plan, sig, 2, N_ITER, None, ws=cws)
    b = plain()
    assert all(np.array_equal(a[k], b[k]) for k in a)


def _clip_default(run, plan, sig, ws):
    """dn_clip_process in default mode with the device generator's phases (flags 0, init_angles NULL) on a given workspace"""
    p, d, m, _ = plan
    lib = run.lib
    ring = np.zeros((1, p.n_fft), np.float32)
    ring[:, p.hop:] = sig[:, :p.hop]
    ola, hx, out = np.zeros((1, p.n_fft), np.float32), np.zeros((1, 17, p.num_compressed_bins), np.float32), np.zeros((1, 2 * p.hop), np.float32)
    hin = emu.f32(sig[:, p.hop:3 * p.hop])
    lib.check(lib.dn_clip_process(m, d, emu.ptr(hin), 0, emu.ptr(ring), emu.ptr(ola), emu.ptr(hx), emu.ptr(out), 0, None, 11, 3, N_ITER, 0.99,
                                  emu.ptr(ws), 1, 2, 0, None))
    assert np.isfinite(out).all()
    return dict(out=out, ring=ring, ola=ola, hx=hx)


# ------------------------------------------------------------------ the seed table of the gpu tier's float64 cases
@pytest.mark.parametrize("family,n_fft", sorted(pcs.SEED_K))
def test_seed_table_is_what_the_screen_gives(family, n_fft):
    assert pcs.first_well_conditioned_k(family, n_fft) == pcs.SEED_K[(family, n_fft)]
