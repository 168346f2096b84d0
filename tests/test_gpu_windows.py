"""Caller-supplied windows and the other never-varied parameters of the DSP primitives on the MI355X (``pytest -m gpu``), against float64
(oracle/dsp_np64.py, oracle/pipeline_np64.py on the fp32 window / filterbank values the kernels hold).  The windows and why the periodic
Hann of every other test cannot stand in for them: tests/dsp_cases.py.  Same cases as tests/test_emu_windows.py at the batches that reach the
ragged paths -- 1 / 3 / 67 for the standalone kernels, 7 for the hop and the pipe, 5 for the forced wave-per-stream schedule and hop groups
(four streams a workgroup and a tail), a pool of 8 with three staggered sessions -- plus GriffinLim(power, rand_init, momentum),
MelScale / InverseMelScale(f_min, f_max), dn_mel_scale / dn_invmel at T != 3, and a filterbank with three filters a bin.

Bars are the project's for the same stage (tests/test_gpu_parity.py, imported where they have a name there): STFT 2e-6 max|ref| + 1e-6,
log-mel 2e-5, inverse mel 2e-5 max(1, max|ref|), istft round trip 2e-5, residual / hx TOL_RESIDUAL, waveform TOL_WAVE_RMS / TOL_WAVE_MAX at
scale max(1, RMS of the float64 waveform).  dn_mel_scale has no log: it is held to the log-mel bar on log1p of both sides
(d log1p(m) = dm / (1 + m): the same bar the fused analysis meets on the same sums).  Every stream is compared.

Guard bands (GUARD) sit beside the bars at 10x the worst value measured on one MI355X over all n_fft, windows and batches of a stage
(python tools/window_margins.py -> profiles/window_parity_margins.txt), never above the bar.  Every check prints its figure first
(`window-margin ...`, visible with -s).
"""
import numpy as np
import pytest
import torch

import dsp_cases as dc
from test_gpu_parity import TOL_RESIDUAL, TOL_WAVE_MAX, TOL_WAVE_RMS, _model

pytestmark = pytest.mark.gpu

TOL_STFT_REL, TOL_STFT_ABS = 2e-6, 1e-6
TOL_LOGMEL = 2e-5
TOL_INVMEL = 2e-5
TOL_ROUND_TRIP = 2e-5
BATCHES = (1, 3, 67)
CASES = [(n, w) for n in dc.N_FFTS for w in dc.WINDOWS]
IDS = [f"{n}-{w}" for n, w in CASES]

# stage -> guard band in the unit of its bar (10x the worst measured; see profiles/window_parity_margins.txt).  A stage without an entry
# is held to its bar alone.
GUARD = {
    "stft": 1.7e-6, "stft_general": 1.8e-6, "round_trip": 1.2e-5, "istft_general": 9.7e-6, "istft_rms": 9.0e-7, "istft_max": 1.2e-5,
    "hop_residual": 2.6e-5, "hop_hx": 3.4e-6, "mel_scale": 7.2e-6, "inverse_mel": 4.0e-6,
    "pipe_rms": 2.4e-4, "pipe_max": 1.3e-3, "groups_rms": 2.2e-4, "groups_max": 1.1e-3, "sessions_rms": 5.7e-4, "sessions_max": 2.0e-3,
    # gl_few, gl32, hop and stream waveforms have no guard: ten times the worst measured is above the bar in RMS and in max-abs for each
    # (gl_few 5.1e-3 / 1.2e-1, gl32 6.8e-3 / 1.5e-1, hop 4.1e-3 / 2.6e-2, stream 5.5e-3 / 2.5e-2 against 1e-3 / 2e-2) -- the Griffin-Lim
    # chain's amplification has a heavy tail over streams already at five or six iterations.  The bars stand alone there.
}


def check(stage, value, bar, **where):
    """print the figure, then hold it to min(guard band, bar)"""
    print(f"window-margin {stage:<18} " + " ".join(f"{k}={v}" for k, v in where.items()) + f" value={value:.2e} bar={bar:.2e}")
    limit = min(GUARD.get(stage, bar), bar)
    assert value <= limit, (stage, where, value, limit)


def check_stft(stage, got, ref, pattern="", **where):
    m = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    try:
        check(stage, err / m, TOL_STFT_REL + TOL_STFT_ABS / m, **where)
    except AssertionError as e:
        raise AssertionError(f"{e}; {pattern() if callable(pattern) else pattern}") from None


def check_wave(stage, got, ref, frame, **where):
    """waveform RMS and max-abs at scale max(1, RMS of the float64 waveform); a failure says where the error sits"""
    rms, mx, scale = dc.wave_errors(got, ref)
    try:
        check(stage + "_rms", rms / scale, TOL_WAVE_RMS, **where)
        check(stage + "_max", mx / scale, TOL_WAVE_MAX, **where)
    except AssertionError as e:
        raise AssertionError(f"{e}; scale {scale:.2f}; {dc.error_pattern(got, ref, frame)}") from None


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


def window_fn(name):
    return lambda n: torch.from_numpy(dc.window(name, n))


def geometry(n_fft):
    from oracle import pipeline_ref
    sr, n_mels = dc.HOP_GEOMETRY[n_fft]
    return pipeline_ref.Params(sr, n_fft, n_fft // 2, n_mels)


def denoiser(dev, n_fft, name, n_iter):
    from audio_denoising_amd.pipeline import Denoiser
    p = geometry(n_fft)
    return Denoiser(_model(dev, p.num_compressed_bins), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter,
                    window=torch.from_numpy(dc.window(name, n_fft)))


def bkt(t):
    """(B, K, T) complex tensor -> numpy complex128"""
    return t.cpu().numpy().astype(np.complex128)


# ------------------------------------------------------------------ the transforms
@pytest.mark.parametrize("n_fft,name", CASES, ids=IDS)
def test_spectrogram_and_inverse_spectrogram_with_the_window(dev, n_fft, name):
    """Spectrogram(window_fn=) of noise frames, InverseSpectrogram(window_fn=) of a NON-consistent spectrogram, and the round trip."""
    from audio_denoising_amd import transforms as T
    from oracle import dsp_np64
    hop, w = n_fft // 2, dc.window(name, n_fft)
    S = T.Spectrogram(power=None, n_fft=n_fft, win_length=n_fft, hop_length=hop, window_fn=window_fn(name)).to(dev)
    I = T.InverseSpectrogram(n_fft=n_fft, win_length=n_fft, hop_length=hop, window_fn=window_fn(name)).to(dev)
    for B in BATCHES:
        x = dc.noise((B, n_fft), 100 + n_fft + B)
        spec = S(torch.from_numpy(x).to(dev))
        ref = dsp_np64.stft(x, n_fft, hop, window=w)
        check_stft("stft", bkt(spec), ref, lambda: dc.error_pattern(bkt(spec), ref, n_fft), n_fft=n_fft, window=name, B=B)
        back = I(spec.contiguous()).cpu().numpy()
        check("round_trip", float(np.abs(back - x).max()), TOL_ROUND_TRIP, n_fft=n_fft, window=name, B=B)
        mag, ang = dc.magnitudes(B, n_fft, 200 + n_fft + B)
        z = (ang * mag).astype(np.complex64)
        wave = I(torch.from_numpy(z).to(dev)).cpu().numpy()
        check_wave("istft", wave, dsp_np64.istft(z, n_fft, hop, window=w), n_fft, n_fft=n_fft, window=name, B=B)


@pytest.mark.parametrize("n_fft,name", CASES, ids=IDS)
def test_general_length_stft_and_istft_with_the_window(dev, n_fft, name):
    """dn_stft_general / dn_istft_general (inv_env[n] per output hop): a ragged length (T = 4) and the minimum (L = hop + 1, T = 2)."""
    from audio_denoising_amd.transforms import DspPlan
    from oracle import dsp_np64
    hop, w = n_fft // 2, dc.window(name, n_fft)
    plan = DspPlan(dev, 0, n_fft, hop, 0, window=torch.from_numpy(w))
    for L in (3 * hop + 37, hop + 1):
        T = 1 + L // hop
        for B in BATCHES:
            x = dc.noise((B, L), 300 + L + B)
            xd = torch.from_numpy(x).to(dev)
            spec = torch.empty(B, T, hop + 1, 2, device=dev)
            plan.lib.check(plan.lib.dn_stft_general(plan.handle, xd.data_ptr(), spec.data_ptr(), None, B, L, None))
            torch.cuda.synchronize()
            ref = dsp_np64.stft(x, n_fft, hop, window=w)
            got = dc.cplx(spec.cpu().numpy())
            err = np.abs(got - ref)
            check_stft("stft_general", got, ref, "max-abs error per column " + ", ".join(f"{err[:, :, t].max():.2e}" for t in range(T)),
                       n_fft=n_fft, window=name, L=L, B=B)
            ref32 = dc.ri(ref)                           # the inverse of the REFERENCE spectrum: the two kernels are checked apart
            wave = torch.empty(B, hop * (T - 1), device=dev)
            sd = torch.from_numpy(ref32).to(dev)
            plan.lib.check(plan.lib.dn_istft_general(plan.handle, sd.data_ptr(), wave.data_ptr(), B, T, None))
            torch.cuda.synchronize()
            want = dsp_np64.istft(dc.cplx(ref32), n_fft, hop, window=w)
            _, mx, scale = dc.wave_errors(wave.cpu().numpy(), want)
            check("istft_general", mx / scale, TOL_ROUND_TRIP, n_fft=n_fft, window=name, L=L, B=B)


# ------------------------------------------------------------------ Griffin-Lim
def _gl(dev, n_fft, name, **kw):
    from audio_denoising_amd import transforms as T
    return T.GriffinLim(n_fft=n_fft, win_length=n_fft, hop_length=n_fft // 2, window_fn=window_fn(name), **kw).to(dev)


@pytest.mark.parametrize("name", dc.WINDOWS + ("hann",))
@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_griffinlim_with_the_window_at_other_iteration_counts_and_momenta(dev, n_fft, name):
    """GriffinLim(window_fn=, n_iter=, momentum=) with injected phases: n_iter 0 (istft of the phased magnitudes), 1 (the first re-STFT),
    momentum 0.5 and 0, and the 32 iterations of the app.  Hann is the control: a failure that it does not share is about the window."""
    from oracle import dsp_np64
    w = dc.window(name, n_fft)
    for n_iter, momentum in ((0, 0.99), (1, 0.99), (5, 0.5), (6, 0.0), (32, 0.99)):
        GL = _gl(dev, n_fft, name, n_iter=n_iter, momentum=momentum, power=1.0)
        for B in BATCHES:
            if (n_iter, B) == (dc.GL32_N_ITER, dc.GL32_BATCH):
                seed = dc.gl32_seed(n_fft, dc.GL32_SEED_K[(n_fft, name)])          # (a well-conditioned batch: tests/dsp_cases.py)
            else:
                seed = 400 + n_fft + n_iter + B
            mag, init = dc.magnitudes(B, n_fft, seed)
            y = GL(torch.from_numpy(mag).to(dev), init_angles=torch.from_numpy(init).to(dev)).cpu().numpy()
            ref = dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=n_iter, momentum=momentum, window=w)
            check_wave("gl32" if n_iter == 32 else "gl_few", y, ref, n_fft, n_fft=n_fft, window=name, n_iter=n_iter, momentum=momentum, B=B)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_griffinlim_power_rand_init_and_zero_momentum(dev, n_fft):
    """power=2.0 on squared magnitudes against power=1.0 on magnitudes: only torch's pow(0.5) on the device differs, so where that returns the
    magnitudes bit for bit (checked first, on the device) the waveforms must be equal bit for bit; where it does not, the kernel is given
    other numbers and both results are held to float64 instead.  rand_init=False starts from unit phases; momentum=0.0 over 32 iterations."""
    from oracle import dsp_np64
    name, B = "asym", 3
    w = dc.window(name, n_fft)
    mag, init = dc.magnitudes(B, n_fft, 900 + n_fft)
    md, idv = torch.from_numpy(mag).to(dev), torch.from_numpy(init).to(dev)
    y1 = _gl(dev, n_fft, name, n_iter=4, power=1.0)(md, init_angles=idv).cpu().numpy()
    y2 = _gl(dev, n_fft, name, n_iter=4, power=2.0)(md * md, init_angles=idv).cpu().numpy()
    ref = dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=4, window=w)
    exact = torch.equal((md * md).pow(0.5), md)
    print(f"window-margin power2 n_fft={n_fft} pow(m*m, 0.5)==m bit for bit on the device: {exact}; max |power2 - power1| {np.abs(y1 - y2).max():.2e}")
    check_wave("gl_few", y1, ref, n_fft, n_fft=n_fft, window=name, case="power1")
    check_wave("gl_few", y2, ref, n_fft, n_fft=n_fft, window=name, case="power2")
    if exact:
        assert np.array_equal(y1, y2)
    ones = np.ones((B, n_fft // 2 + 1, 3), np.complex64)
    y = _gl(dev, n_fft, name, n_iter=4, power=1.0, rand_init=False)(md).cpu().numpy()
    check_wave("gl_few", y, dsp_np64.griffinlim(mag, n_fft, n_fft // 2, ones, n_iter=4, window=w), n_fft, n_fft=n_fft, window=name,
               case="rand_init=False")
    y = _gl(dev, n_fft, name, n_iter=32, power=1.0, momentum=0.0)(md, init_angles=idv).cpu().numpy()
    check_wave("gl32", y, dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=32, momentum=0.0, window=w), n_fft, n_fft=n_fft,
               window=name, case="momentum=0")


# ------------------------------------------------------------------ the fused hop and the stream
N_ITER = 6


def _inits(rg, n, B, K):
    return [(rg.random((B, K, 3)) + 1j * rg.random((B, K, 3))).astype(np.complex64) for _ in range(n)]


@pytest.mark.parametrize("n_fft,name", CASES, ids=IDS)
def test_process_frame_and_stream_with_the_window(dev, n_fft, name):
    """Denoiser(window=).process_frame and DenoiserStream over two frames (ragged arrival) at batch 7 against process_frame64."""
    from audio_denoising_amd.pipeline import DenoiserStream
    p, w, B = geometry(n_fft), dc.window(name, n_fft), 7
    dn = denoiser(dev, n_fft, name, N_ITER)
    sig = dc.noise((B, n_fft + p.hop), 500 + n_fft, dc.HOP_LEVEL)
    inits = _inits(np.random.default_rng(600 + n_fft), 2, B, p.n_stft)
    frames = [np.ascontiguousarray(sig[:, f * p.hop:f * p.hop + n_fft]) for f in range(2)]
    from oracle import pipeline_np64
    r0 = pipeline_np64.process_frame64(frames[0], np.zeros((B, 17, p.num_compressed_bins)), dc.model64(), w, dc.fbank(p), inits[0], n_fft, p.hop,
                                       n_iter=N_ITER)
    r1 = pipeline_np64.process_frame64(frames[1], r0["hx"], dc.model64(), w, dc.fbank(p), inits[1], n_fft, p.hop, n_iter=N_ITER)
    out, hx, resid = dn.process_frame(torch.from_numpy(frames[0]).to(dev), None, init_angles=torch.from_numpy(inits[0]).to(dev), return_residual=True)
    where = dict(n_fft=n_fft, window=name, B=B)
    check("hop_residual", float(np.abs(resid.cpu().numpy() - r0["predicted_diff"]).max()), TOL_RESIDUAL, **where)
    check("hop_hx", float(np.abs(hx.cpu().numpy() - r0["hx"]).max()), TOL_RESIDUAL, **where)
    check_wave("hop", out.cpu().numpy(), r0["out"], n_fft, **where)
    st = DenoiserStream(dn, B)
    d_inits = [torch.from_numpy(a).to(dev) for a in inits]
    outs = []
    for a, b in ((0, 100), (100, n_fft + 5), (n_fft + 5, sig.shape[1])):
        outs.append(st.push(torch.from_numpy(sig[:, a:b].copy()).to(dev), init_angles_per_hop=d_inits[st.hops:]))
    y = torch.cat(outs, 1).cpu().numpy()
    assert y.shape == (B, 2 * p.hop) and not y[:, :p.hop].any() and np.abs(r0["out"][:, :p.hop]).max() > 0.1
    check_wave("stream", y[:, p.hop:], r0["out"][:, :p.hop], n_fft, **where)
    check("hop_hx", float(np.abs(st.hx.cpu().numpy() - r1["hx"]).max()), TOL_RESIDUAL, **where)
    line = np.concatenate([r0["out"][:, p.hop:] + r1["out"][:, :p.hop], r1["out"][:, p.hop:]], axis=1)
    check_wave("stream", st.ola.cpu().numpy(), line, n_fft, what="overlap-add line", **where)


# ------------------------------------------------------------------ n_fft 1024: the schedules that read the host-built tables
N_HOPS = 4


@pytest.fixture(scope="module")
def chains():
    """window name -> (frames (N_HOPS, 7, 1024), phases (N_HOPS, 7, 513, 3), float64 frames, float64 hx, signal (7, 1024 + 3 * 512)): four chained
    hops of seven streams through process_frame64, computed once per window (streams are independent: a test at batch 5 takes the first five)"""
    made = {}

    def get(name):
        if name not in made:
            p, B = geometry(1024), 7
            sig = dc.noise((B, 1024 + (N_HOPS - 1) * 512), 738, dc.HOP_LEVEL)          # (the seed: see profiles/window_parity_margins.txt)
            inits = _inits(np.random.default_rng(739), N_HOPS, B, 513)
            frames = [np.ascontiguousarray(sig[:, h * 512:h * 512 + 1024]) for h in range(N_HOPS)]
            outs64, hx64 = dc.frames64(frames, inits, p, dc.window(name, 1024), N_ITER)
            made[name] = (np.stack(frames), np.stack(inits), np.stack(outs64), hx64, sig)
        return made[name]
    return get


def _run(dev, dn, chain, B, schedule=None, depth=1, group=0):
    """N_HOPS hops of the first B streams through a HopPipeline -> (frames (N_HOPS, B, 1024), hx) as numpy"""
    from audio_denoising_amd.pipeline import HopPipeline
    frames, inits = chain[0][:, :B], chain[1][:, :B]
    fd, ia = torch.from_numpy(frames.copy()).to(dev), torch.from_numpy(inits.copy()).to(dev)
    out, hx = torch.empty(N_HOPS, B, 1024, device=dev), dn.init_hx(B)
    pipe = HopPipeline(dn, B)
    if schedule is not None:
        pipe.set_gl_schedule(schedule)
    if depth != 1:
        pipe.set_depth(depth)
    if group:
        pipe.set_group(group)
        for h in range(0, N_HOPS, group):
            pipe.submit_group(fd[h:h + group], hx, out[h:h + group], seed=0, init_angles=ia[h:h + group])
    else:
        for h in range(N_HOPS):
            pipe.submit(fd[h], hx, out[h], seed=0, init_angles=ia[h])
    pipe.flush()
    torch.cuda.synchronize()
    return out.cpu().numpy(), hx.cpu().numpy()


def _against_float64(stage, got, chain, B, **where):
    out, hx = got
    for h in range(N_HOPS):
        check_wave(stage, out[h], chain[2][h, :B], 1024, hop=h, B=B, **where)
    check("hop_hx", float(np.abs(hx - chain[3][:B]).max()), TOL_RESIDUAL, B=B, **where)


@pytest.mark.parametrize("name", dc.WINDOWS)
def test_pipe_schedules_with_the_window(dev, chains, name):
    """The one-hop pipe at batch 7 (wave per column); DN_GL_WAVE_PER_STREAM forced and depth 2 at batch 5: the wave-per-column pipe's frames
    and hx bit for bit, as under Hann -- and, which the schedules' identity alone cannot show, float64's."""
    from audio_denoising_amd import _lib
    chain, dn = chains(name), denoiser(dev, 1024, name, N_ITER)
    _against_float64("pipe", _run(dev, dn, chain, 7, _lib.DN_GL_WAVE_PER_COLUMN), chain, 7, window=name, schedule="per-column")
    a = _run(dev, dn, chain, 5, _lib.DN_GL_WAVE_PER_COLUMN)
    b = _run(dev, dn, chain, 5, _lib.DN_GL_WAVE_PER_STREAM)
    c = _run(dev, dn, chain, 5, depth=2)
    _against_float64("pipe", b, chain, 5, window=name, schedule="per-stream")
    _against_float64("pipe", c, chain, 5, window=name, schedule="depth 2")
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])


@pytest.mark.parametrize("H", [2, 4])
@pytest.mark.parametrize("name", dc.WINDOWS)
def test_hop_groups_with_the_window(dev, chains, name, H):
    from audio_denoising_amd import _lib
    chain, dn = chains(name), denoiser(dev, 1024, name, N_ITER)
    a = _run(dev, dn, chain, 5, _lib.DN_GL_WAVE_PER_COLUMN)
    b = _run(dev, dn, chain, 5, group=H)
    _against_float64("groups", b, chain, 5, window=name, H=H)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name", dc.WINDOWS)
def test_session_pool_in_both_schedules_with_the_window(dev, chains, name):
    """A pool of 8 with three sessions on scattered slots whose first pushes are one tick apart, pushed in a new order every tick, injected
    phases: the one-launch and the two-launch schedule bit for bit, as under Hann, and each session against the float64 stream."""
    from audio_denoising_amd import SessionPool, _lib
    frames, inits, outs64, _, sig = chains(name)
    dn = denoiser(dev, 1024, name, N_ITER)
    n_sess, slots_wanted = 3, [6, 1, 4]
    # float64: session k emits, with its push j >= 1, the overlap-add line before frame j - 1 is added
    ola = np.zeros((n_sess, 1024))
    want = []
    for f in range(N_HOPS):
        want.append(ola[:, :512].copy())
        ola = np.concatenate([ola[:, 512:], np.zeros((n_sess, 512))], axis=1) + outs64[f, :n_sess]
    want = np.stack(want)                                  # (frame, session, hop)
    got = {}
    for schedule in (_lib.DN_SESS_ONE_LAUNCH, _lib.DN_SESS_TWO_LAUNCHES):
        pool = SessionPool(dn, 8)
        pool.set_schedule(schedule)
        taken = [pool.open(100 + s) for s in range(8)]
        for s in taken:
            if s not in slots_wanted:
                pool.close(s)
        rows = np.zeros((N_HOPS, n_sess, 512), np.float32)
        rg = np.random.default_rng(5)
        for t in range(N_HOPS + n_sess):
            live = [k for k in range(n_sess) if 0 <= t - k <= N_HOPS]
            live = [live[i] for i in rg.permutation(len(live))]
            hops = np.stack([sig[k, (t - k) * 512:(t - k + 1) * 512] for k in live])
            ia = np.stack([inits[max(t - k - 1, 0), k] for k in live])              # (a priming push draws nothing: any row)
            out = pool.push([slots_wanted[k] for k in live], torch.from_numpy(hops).to(dev), init_angles=torch.from_numpy(ia).to(dev)).cpu().numpy()
            for r, k in enumerate(live):
                if t - k == 0:
                    assert not out[r].any()
                else:
                    rows[t - k - 1, k] = out[r]
        got[schedule] = rows
        assert np.abs(want[1:]).max() > 0.1 and not rows[0].any()
        for k in range(n_sess):
            y, ref = rows[1:, k].reshape(1, -1), want[1:, k].reshape(1, -1)
            check_wave("sessions", y, ref, 1024, window=name, schedule=schedule, session=k)
    assert np.array_equal(got[_lib.DN_SESS_ONE_LAUNCH], got[_lib.DN_SESS_TWO_LAUNCHES])


# ------------------------------------------------------------------ the mel stages
def test_mel_scale_and_inverse_with_f_min_and_f_max(dev):
    """MelScale / InverseMelScale(f_min=300, f_max=3400) at 16 kHz, n_fft 1024: the filters start above bin 0 and end below Nyquist; bins
    outside every filter come back exactly 0 from the inverse."""
    from audio_denoising_amd import transforms as T
    from oracle import dsp_np64, dsp_ref
    n_stft, sr, f_min, f_max = 513, 16000, 300.0, 3400.0
    n_mels = 48
    while n_mels > 1:            # CPU check first: no all-zero filter and full rank at this filter count, or the plan cannot build
        fb = dsp_ref.melscale_fbanks(n_stft, n_mels, sr, f_min, f_max)
        if (fb.sum(0) > 0).all() and np.linalg.matrix_rank(fb.numpy().astype(np.float64)) == n_mels:
            break
        n_mels -= 8
    assert n_mels >= 16
    M = T.MelScale(n_mels=n_mels, sample_rate=sr, f_min=f_min, f_max=f_max, n_stft=n_stft).to(dev)
    Mi = T.InverseMelScale(n_stft=n_stft, n_mels=n_mels, sample_rate=sr, f_min=f_min, f_max=f_max).to(dev)
    assert torch.equal(M.fb.cpu(), fb) and torch.equal(Mi.fb.cpu(), fb)
    outside = (fb == 0).all(1).numpy()
    assert outside[:15].all() and outside[230:].all() and not outside[40:200].any()          # 300 Hz = bin 19.2, 3400 Hz = bin 217.6
    g = torch.Generator().manual_seed(41)
    for B in BATCHES:
        mag = torch.rand(B, n_stft, 3, generator=g) * 3.0
        mel = M(mag.to(dev)).cpu().numpy()
        ref = dsp_np64.mel_scale(mag.numpy(), fb.numpy())
        check("mel_scale", float(np.abs(np.log1p(mel) - np.log1p(ref)).max()), TOL_LOGMEL, case="f_min/f_max", B=B)
        mm = torch.rand(B, n_mels, 3, generator=g) * 20.0
        lin = Mi(mm.to(dev)).cpu().numpy()
        ref = dsp_np64.inverse_mel_scale(mm.numpy(), fb.numpy())
        check("inverse_mel", float(np.abs(lin - ref).max()) / max(1.0, float(np.abs(ref).max())), TOL_INVMEL, case="f_min/f_max", B=B)
        assert not lin[:, outside, :].any() and np.abs(lin[:, ~outside, :]).max() > 1.0


def test_rank_deficient_filterbank_is_refused(dev):
    """80 HTK filters over 257 bins at 16 kHz leave filters without a bin of their own: the library's error, not a run."""
    from audio_denoising_amd import transforms as T
    from audio_denoising_amd._lib import DnError
    Mi = T.InverseMelScale(n_stft=257, n_mels=80, sample_rate=16000).to(dev)
    with pytest.raises(DnError, match="rank deficient"):
        Mi(torch.rand(1, 80, 3).to(dev))


def _wide_fbank(n_stft, n_mels, sample_rate):
    """HTK-spaced triangles widened to span two neighbours: filter m runs from point m to point m + 3, so every bin lies in three filters"""
    f_max = sample_rate // 2
    freqs = np.linspace(0.0, f_max, n_stft)
    pts = 700.0 * (10.0 ** (np.linspace(0.0, 2595.0 * np.log10(1.0 + f_max / 700.0), n_mels + 3) / 2595.0) - 1.0)
    fb = np.zeros((n_stft, n_mels))
    for m in range(n_mels):
        lo, hi, ce = pts[m], pts[m + 3], 0.5 * (pts[m + 1] + pts[m + 2])
        fb[:, m] = np.maximum(0.0, np.minimum((freqs - lo) / (ce - lo), (hi - freqs) / (hi - ce)))
    return fb.astype(np.float32)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_mel_stages_at_other_column_counts_and_a_three_filter_bank(dev, n_fft):
    """dn_mel_scale and dn_invmel at T = 1, 2, 5 with B * T = 1, 7 (ragged), 335 rows, on the hop geometry's filterbank (inverse in factors)
    and on a filterbank with three filters a bin and no explicit pseudo-inverse (the plan has to take the dense contraction with the
    pseudo-inverse it computes itself; which path ran is not visible from here: only the result is held to float64 pinv)."""
    from audio_denoising_amd.transforms import DspPlan
    from oracle import dsp_np64
    p = geometry(n_fft)
    wide = _wide_fbank(p.n_stft, 40, p.sample_rate)
    assert ((wide != 0).sum(1) == 3).any() and ((wide != 0).sum(1) <= 3).all() and np.linalg.matrix_rank(wide.astype(np.float64)) == 40
    g = torch.Generator().manual_seed(43 + n_fft)
    for tag, fb in (("htk", dc.fbank(p)), ("three-filter", wide)):
        M = fb.shape[1]
        plan = DspPlan(dev, p.sample_rate, n_fft, p.hop, M, fb=torch.from_numpy(fb))
        for B, T in ((1, 1), (7, 1), (67, 5), (1, 2), (2, 2)):
            mag = torch.rand(B, T, p.n_stft, generator=g) * 3.0
            mel = torch.full((B, T, M), float("nan"), device=dev)
            md = mag.to(dev)
            plan.lib.check(plan.lib.dn_mel_scale(plan.handle, md.data_ptr(), mel.data_ptr(), B, T, None))
            torch.cuda.synchronize()
            ref = np.einsum("btk,km->btm", mag.numpy().astype(np.float64), fb.astype(np.float64))
            check("mel_scale", float(np.abs(np.log1p(mel.cpu().numpy()) - np.log1p(ref)).max()), TOL_LOGMEL, n_fft=n_fft, fb=tag, B=B, T=T)
            mm = torch.rand(B, T, M, generator=g) * 20.0
            lin = torch.full((B, T, p.n_stft), float("nan"), device=dev)
            mmd = mm.to(dev)
            plan.lib.check(plan.lib.dn_invmel(plan.handle, mmd.data_ptr(), lin.data_ptr(), B, T, None))
            torch.cuda.synchronize()
            ref = dsp_np64.inverse_mel_scale(mm.numpy().transpose(0, 2, 1), fb).transpose(0, 2, 1)
            check("inverse_mel", float(np.abs(lin.cpu().numpy() - ref).max()) / max(1.0, float(np.abs(ref).max())), TOL_INVMEL, n_fft=n_fft,
                  fb=tag, B=B, T=T)
