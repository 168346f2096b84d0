"""Input-phase mode (DN_PHASE_FROM_INPUT; ``Denoiser(phase="input")``) on the MI355X (``pytest -m gpu``).  tests/phase_cases.py holds the
references, the runner of every entry point and the bounds; tests/test_emu_phase.py is the CPU tier of the same families.

  1. dn_stft_phasors against float64, weighted by magnitude, B = 5, every n_fft, two windows; unit modulus; zero, constant and impulse frames.
  2. The flag equals injected phasors, bit for bit (np.array_equal / torch.equal on everything a call writes): every entry point of the C ABI and
     every mode of a pipe at B = 5 (a chain workgroup of four partly filled) and 3, n_iter 0 and 2, every n_fft for the modes it has; then the
     Python front ends against each other.
  3. The Python front ends against float64 end to end, noise at dsp_cases.HOP_LEVEL: process_frame at B = 6 and a 12-hop DenoiserStream at B = 3,
     n_iter 0, 2 and 6, bound R x e_ref (e_ref: the CPU oracle's fp32 stages on the same case), mel residual and hx at their guard bands.
Every figure is printed before it is asserted (profiles/phase_input_margins.txt is that output)."""
import numpy as np
import pytest
import torch

import dsp_cases as dc
import phase_cases as pcs
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def run(dev):
    from audio_denoising_amd import _lib
    r = pcs.Runner(_lib.get_lib(), dev)
    yield r
    torch.cuda.synchronize()
    r.close()


@pytest.fixture(scope="module")
def denoisers(dev):
    from audio_denoising_amd.pipeline import Denoiser
    cache = {}

    def get(n_fft, phase, n_iter):
        if (n_fft, phase, n_iter) not in cache:
            p = pcs.geometry(n_fft)
            cache[n_fft, phase, n_iter] = Denoiser(_model(dev, p.num_compressed_bins), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter,
                                                   phase=phase)
        return cache[n_fft, phase, n_iter]
    return get


# ------------------------------------------------------------------ 1. phasors alone
@pytest.mark.parametrize("window", pcs.WINDOWS)
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_phasors_match_float64(run, n_fft, window):
    plan = run.plan(n_fft, window)
    w = plan[3]
    special = np.zeros((3, n_fft), np.float32)            # an all-zero frame, a constant frame, a one-sample impulse
    special[1] = 0.37
    special[2, n_fft // 3] = -2.5
    for name, frames in (("noise", dc.noise((5, n_fft), 500 + n_fft)), ("special", special)):
        u = dc.cplx(run.phasors(plan, frames))
        X64 = pcs.spectrum64(frames, n_fft, w)
        u32 = pcs.phasors32(frames, n_fft, w)
        assert np.abs(np.abs(u) - 1.0).max() <= pcs.ULP_BAND, name
        for b in (range(5) if name == "noise" else (1, 2)):
            e, e_ref = pcs.weighted_error(u[b], X64[b]), pcs.weighted_error(u32[b], X64[b])
            print(f"MARGIN phasors n_fft {n_fft} {window} {name}[{b}]: weighted error {e:.3e}, fp32 torch {e_ref:.3e}, ratio {e / e_ref:.2f}")
            assert e <= pcs.R_PHASOR * e_ref, (name, b, e, e_ref)
        if name == "special":
            assert np.array_equal(u[0], np.ones_like(u[0])), "an all-zero frame gives exactly (1, 0) everywhere"


# ------------------------------------------------------------------ 2. the flag equals injected phasors: the C ABI
CASES = [(n_fft, B, n_iter) for n_fft in pcs.N_FFTS for B in (5, 3) for n_iter in (0, 2)]
HOPS = 3


def _modes(n_fft):
    return list(pcs.MODES) if n_fft == 1024 else list(pcs.MODES_ANY_NFFT)


@pytest.mark.parametrize("n_fft,B,n_iter", CASES)
def test_process_frame_and_stream_steps(run, n_fft, B, n_iter):
    plan = run.plan(n_fft, "asym")
    p = plan[0]
    sig = pcs.stream_signal(B, n_fft, HOPS + 1)
    frames = pcs.stream_frames(sig, p, HOPS + 1)
    hx0 = 0.1 * dc.noise((B, 17, p.num_compressed_bins), 9)
    pcs.identity(run, plan, frames[:1], lambda inits: run.run_frame(plan, frames[0], hx0, n_iter, inits))
    pcs.identity(run, plan, frames[:1], lambda inits: run.run_frame(plan, frames[0], hx0, n_iter, inits, conv=pcs.DN_CONV_BF16))
    a = pcs.identity(run, plan, frames[:HOPS], lambda inits: run.run_steps(plan, sig, HOPS, n_iter, inits))
    assert np.abs(a["out"][:, p.hop:]).max() > 1e-3


@pytest.mark.parametrize("n_fft,B,n_iter", CASES)
def test_clip(run, n_fft, B, n_iter):
    plan = run.plan(n_fft, "asym")
    layouts = (pcs.DN_CLIP_GL_PER_COLUMN, pcs.DN_CLIP_GL_PER_STREAM) if n_fft == 1024 else (0,)
    for N in (1, 2, 4):
        sig = pcs.stream_signal(B, n_fft, N, seed=20 + N)
        steps = run.run_steps(plan, sig, N, n_iter)
        for s in (sig, pcs.to_s16(sig)):
            frames = pcs.stream_frames(s, plan[0], N)
            for gl in layouts:
                a = pcs.identity(run, plan, frames, lambda inits: run.run_clip(plan, s, N, n_iter, inits, gl))
                if s.dtype != np.int16:
                    assert all(np.array_equal(a[k], steps[k]) for k in a), "dn_clip_process is N calls of dn_stream_step in input-phase mode too"


@pytest.mark.parametrize("n_fft,B,n_iter", CASES)
def test_frame_pipe_every_mode(run, n_fft, B, n_iter):
    plan = run.plan(n_fft, "asym")
    F = 5
    frames = np.stack(pcs.stream_frames(pcs.stream_signal(B, n_fft, F, seed=5), plan[0], F))
    first = run.run_frame(plan, frames[0], np.zeros((B, 17, plan[0].num_compressed_bins), np.float32), n_iter)
    ref = None
    for mode in _modes(n_fft):
        a = pcs.identity(run, plan, list(frames), lambda inits: run.run_pipe_frames(plan, frames, n_iter, pcs.MODES[mode], inits))
        assert np.array_equal(a["out"][0], first["out"]), (mode, "the pipe's first frame is dn_process_frame's")
        ref = a if ref is None else ref
        assert all(np.array_equal(a[k], ref[k]) for k in a), (mode, "every mode of a pipe gives the one-hop pipe's bits")


@pytest.mark.parametrize("n_fft,B,n_iter", CASES)
def test_stream_pipe_every_mode(run, n_fft, B, n_iter):
    plan = run.plan(n_fft, "asym")
    p = plan[0]
    pushes = 8                                            # a multiple of both group sizes; frames 0 .. 6
    sig = pcs.stream_signal(B, n_fft, pushes - 1, seed=6)
    frames = pcs.stream_frames(sig, p, pushes - 1)
    steps = run.run_steps(plan, sig, pushes - 1, n_iter)
    hops = steps["out"].reshape(B, pushes - 1, p.hop)
    for mode in _modes(n_fft):
        a = pcs.identity(run, plan, frames, lambda inits: run.run_pipe_stream(plan, sig, pushes, n_iter, pcs.MODES[mode], inits))
        assert int(a["frames"]) == pushes - 1, mode
        # the samples are dn_stream_step's, later: frame f's hop (the overlap-add line before frame f is added; zeros for f = 0) comes out once
        # frame f - 1 is done, behind zero hops; the state the pipe is left with is the steps'
        live = [h for h in a["out"] if h.any()]
        assert len(live) == pushes - 2 and all(np.array_equal(h, hops[:, 1 + i]) for i, h in enumerate(live)), mode
        assert np.array_equal(a["ring"], steps["ring"]) and np.array_equal(a["hx"], steps["hx"]) and np.array_equal(a["ola"], steps["ola"]), mode


@pytest.mark.parametrize("n_fft,B,n_iter", CASES)
def test_session_pool_both_schedules(run, n_fft, B, n_iter):
    plan = run.plan(n_fft, "asym")
    sig = pcs.stream_signal(B, n_fft, HOPS, seed=9)
    steps = run.run_steps(plan, sig, HOPS, n_iter)["out"].reshape(B, HOPS, -1)
    ref = None
    for schedule in ((1, 2) if n_fft == 1024 else (1,)):
        a = pcs.identity(run, plan, pcs.stream_frames(sig, plan[0], HOPS), lambda inits: run.run_sessions(plan, sig, HOPS + 1, n_iter, schedule, inits))
        assert not a["out"][0].any() and all(np.array_equal(a["out"][1 + h], steps[:, h]) for h in range(HOPS)), "a session's samples are dn_stream_step's"
        ref = a if ref is None else ref
        assert all(np.array_equal(a[k], ref[k]) for k in a)


# ------------------------------------------------------------------ 2. the Python front ends
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_denoiser_phase_input_equals_injected_input_phases(dev, denoisers, n_fft):
    dn_in, dn_rand = denoisers(n_fft, "input", 2), denoisers(n_fft, "random", 2)
    frames = torch.from_numpy(dc.noise((5, n_fft), 61, dc.HOP_LEVEL)).to(dev)
    u = dn_rand.input_phases(frames)
    assert u.shape == (5, n_fft // 2 + 1, 3) and u.dtype == torch.complex64 and torch.equal(u, dn_in.input_phases(frames))
    a = dn_in.process_frame(frames, None, return_residual=True)
    b = dn_rand.process_frame(frames, None, init_angles=u, return_residual=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.isfinite(a[0]).all()
    c = dn_in.process_frame(frames, None, seed=12345, stream_id0=9)
    assert torch.equal(c[0], a[0]), "seed and stream_id0 are ignored for the phases"
    out, hx = torch.empty_like(frames), dn_in.init_hx(5)
    dn_in.process_frame_(frames, hx, out)
    assert torch.equal(out, a[0]) and torch.equal(hx, a[1])
    with pytest.raises(ValueError, match="init_angles"):
        dn_in.process_frame(frames, None, init_angles=u)
    with pytest.raises(ValueError):
        from audio_denoising_amd.pipeline import Denoiser
        Denoiser(dn_in.model, dn_in.sample_rate, n_fft, n_fft // 2, dn_in.n_mels, phase="noisy")


@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_streaming_front_ends_agree(dev, denoisers, n_fft):
    """DenoiserStream.push against push_many against PipelinedStream (delayed by its hop) against SessionPool, and a captured graph_step
    replayed four times against eager pushes"""
    from audio_denoising_amd.pipeline import DenoiserStream, PipelinedStream
    from audio_denoising_amd.sessions import SessionPool
    dn = denoisers(n_fft, "input", 2)
    B, hops = 3, 6
    sig = torch.from_numpy(pcs.stream_signal(B, n_fft, hops, seed=62)).to(dev)                # (B, (hops + 1) hop): hop 0 primes
    a = DenoiserStream(dn, B)
    ref = torch.cat([a.push(sig[:, k * dn.hop:(k + 1) * dn.hop].contiguous()) for k in range(hops + 1)], dim=1)
    assert ref.shape == (B, hops * dn.hop) and ref[:, dn.hop:].abs().max() > 1e-3
    b = DenoiserStream(dn, B)
    many = b.push_many(sig)
    assert torch.equal(many, ref) and torch.equal(a.ola, b.ola) and torch.equal(a.hx, b.hx) and torch.equal(a.ring, b.ring)
    with pytest.raises(ValueError, match="init_angles"):
        b.push(sig[:, :dn.hop].contiguous(), init_angles_per_hop=[dn.input_phases(sig[:, :n_fft].contiguous())])
    # the pipe emits frame f's hop one push later: push k + 1 of the pipe = hop k of the stream (push 0 primes, push 1 emits zeros)
    pipe = PipelinedStream(dn, B)
    piped = [pipe.push(sig[:, k * dn.hop:(k + 1) * dn.hop].contiguous()) for k in range(hops + 1)] + [pipe.flush()]
    assert not piped[0].any() and not piped[1].any()
    assert torch.equal(torch.cat(piped[2:], dim=1), ref)
    # a captured push replayed four times against the eager pushes above
    gpipe = PipelinedStream(dn, B)
    hop_buf, out_buf = torch.zeros(B, dn.hop, device=dev), torch.zeros(B, dn.hop, device=dev)
    for k in range(2):
        gpipe.push_(sig[:, k * dn.hop:(k + 1) * dn.hop].contiguous(), out_buf)
    g = gpipe.graph_step(hop_buf, out_buf)
    for k in range(2, 6):
        hop_buf.copy_(sig[:, k * dn.hop:(k + 1) * dn.hop])
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_buf, piped[k]), k
    # a session per stream
    pool = SessionPool(dn, B + 1)
    slots = [pool.open() for _ in range(B)]
    outs = [pool.push(slots, sig[:, k * dn.hop:(k + 1) * dn.hop].contiguous()) for k in range(hops + 1)]
    assert not outs[0].any() and torch.equal(torch.cat(outs[1:], dim=1), ref)


# ------------------------------------------------------------------ 3. against float64, end to end
_REF = {}


def _reference(family, n_fft, n_iter):
    """the case's input, its float64 result and the fp32 yardstick's, computed once"""
    key = (family, n_fft, n_iter)
    if key not in _REF:
        x = pcs.e2e_input(family, n_fft)
        p = pcs.geometry(n_fft)
        y64, hx64, resid64 = pcs.e2e_ref64(family, n_fft, n_iter, x)
        if family == "frame":
            y32 = pcs.frame32(x, np.zeros((x.shape[0], 17, p.num_compressed_bins), np.float32), p, n_iter)["out"]
        else:
            y32 = pcs.stream32(x, p, n_iter, pcs.STREAM_F)[0]
        _REF[key] = (x, y64, hx64, resid64, y32)
    return _REF[key]


def _check_wave(tag, got, y64, y32, R):
    rms, mx, scale = dc.wave_errors(got, y64)
    ref_rms, ref_mx, _ = dc.wave_errors(y32, y64)
    print(f"MARGIN {tag}: RMS {rms:.3e} (e_ref {ref_rms:.3e}, ratio {rms / ref_rms:.2f}), max-abs {mx:.3e} (e_ref {ref_mx:.3e}, ratio {mx / ref_mx:.2f}), "
          f"scale {scale:.3f}")
    assert R * ref_rms <= pcs.BAR_RMS * scale and R * ref_mx <= pcs.BAR_MAX * scale, "R x e_ref must stay under the project's bars"
    assert rms <= R * ref_rms and mx <= R * ref_mx, (tag, rms, ref_rms, mx, ref_mx)


@pytest.mark.parametrize("n_iter", pcs.E2E_N_ITERS)
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_process_frame_against_float64(dev, denoisers, n_fft, n_iter):
    x, y64, hx64, resid64, y32 = _reference("frame", n_fft, n_iter)
    out, hx, resid = denoisers(n_fft, "input", n_iter).process_frame(torch.from_numpy(x).to(dev), None, return_residual=True)
    e_res, e_hx = float(np.abs(resid.cpu().numpy() - resid64).max()), float(np.abs(hx.cpu().numpy() - hx64).max())
    print(f"MARGIN frame n_fft {n_fft} n_iter {n_iter}: mel residual max-abs {e_res:.3e}, hx max-abs {e_hx:.3e}")
    assert e_res <= pcs.RESID_BAR and e_hx <= pcs.HX_BAR
    _check_wave(f"frame n_fft {n_fft} n_iter {n_iter}", out.cpu().numpy(), y64, y32, pcs.R_FRAME)


@pytest.mark.parametrize("n_iter", pcs.E2E_N_ITERS)
@pytest.mark.parametrize("n_fft", pcs.N_FFTS)
def test_stream_against_float64(dev, denoisers, n_fft, n_iter):
    from audio_denoising_amd.pipeline import DenoiserStream
    x, y64, hx64, _, y32 = _reference("stream", n_fft, n_iter)
    s = DenoiserStream(denoisers(n_fft, "input", n_iter), pcs.STREAM_B)
    got = s.push(torch.from_numpy(x).to(dev))
    assert got.shape == y64.shape
    e_hx = float(np.abs(s.hx.cpu().numpy() - hx64).max())
    print(f"MARGIN stream n_fft {n_fft} n_iter {n_iter}: hx max-abs {e_hx:.3e}")
    assert e_hx <= pcs.HX_BAR
    _check_wave(f"stream n_fft {n_fft} n_iter {n_iter}", got.cpu().numpy(), y64, y32, pcs.R_STREAM)
