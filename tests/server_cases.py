"""Shared cases of the server-variant tests (tests/test_emu_server.py, tests/test_gpu_server.py, tools/server_margins.py): the geometries,
lengths and inputs, the float64 references (oracle/server_np64.py) and the checks both tiers run.  TEST INFRASTRUCTURE; the kernels are run
by the backend a test hands in (tests/model_abi.Abi: the C ABI on host buffers for the emulated library, on GPU buffers for the product).

Why these kernels need cases of their own: dn_general.hip shares the one-wave FFT with the hop path and nothing else.  Its reflect padding
takes both branches inside one column when L is short; its mel loop walks mel_start / mel_len / mel_w in rounds of 64 lanes, not the hop
kernels' packed schedule; server_rows_kernel has its own exp(logmel - 3 relu(out)) - 1, its own dense contraction with the pseudo-inverse in
rounds of 192 threads with a k < bins tail (2 rounds at 257 bins, 3 at 513, 5 at 769) and its own phasor (hypot and two divisions);
istft_general_kernel has its own two-wave overlap.  Before these cases the suite held them end to end only, against the fp32 restatement,
with the trained checkpoint at 64 mels, and held the two transforms to float64 with logmel = NULL.

Geometries (n_fft, sample rate, n_mels): three the chain runs at (64 / 80 mels = 4 / 5 compressed bins) and two for the mel loop alone -- 40
mels (a lane tail in the first round) and 128 (two full rounds).  Lengths: the minimum hop + 1 (T = 2; column 1 reflects on the right from
its middle on), n_fft - 1 (T = 2), n_fft (T = 3) and a ragged 2 n_fft + hop / 2 + 3 (T = 5).  Windows: periodic Hann and the asymmetric,
nowhere-zero window of tests/dsp_cases.py.

The stage references take the plan's own fp32 tables (dn_dsp_get_tables) in float64; the chain's reference solves the inverse mel scale
itself.  Every liveness condition below is asserted on the float64 reference alone, never on a kernel's output.

Bars are the project's for the same stage: spectrum 2e-6 max|ref| + 1e-6, log-mel 2e-5, rows 2e-5 max(1, max|ref|) (the inverse-mel bar),
dn_istft_general 2e-5 max|ref|, chain waveform TOL_WAVE_RMS / TOL_WAVE_MAX at scale max(1, RMS of the float64 waveform), chain hx
TOL_HX_STREAM.  A tier's guard bands (10 x the worst measured there, profiles/server_parity_margins.txt) sit beside them, never above.
"""
import ctypes as C

import numpy as np

import dsp_cases as dc
import model_cases as mc
from oracle import server_np64
from test_gpu_parity import TOL_HX_STREAM, TOL_WAVE_MAX, TOL_WAVE_RMS

DN_OK, DN_ERR_INVALID = 0, -1

GEOMETRIES = [(512, 16000, 64), (1024, 16000, 80), (1536, 48000, 64), (1536, 48000, 40), (1024, 16000, 128)]
CHAIN_GEOMETRIES = GEOMETRIES[:3]
WINDOWS = ("hann", "asym")
STAGE_CASES = [(g, w) for g in GEOMETRIES for w in WINDOWS]
STAGE_IDS = [f"{g[0]}-{g[2]}mels-{w}" for g, w in STAGE_CASES]
ISTFT_CASES = [(n, w) for n in dc.N_FFTS for w in WINDOWS]
ISTFT_IDS = [f"{n}-{w}" for n, w in ISTFT_CASES]
ISTFT_T = (2, 3, 9)
# (geometry, window, hx_decay): the asymmetric window at the server's own 0.9, and one other decay
CHAIN_CASES = [(g, "asym", 0.9) for g in CHAIN_GEOMETRIES] + [(CHAIN_GEOMETRIES[1], "hann", 0.5)]
CHAIN_IDS = [f"{g[0]}-{g[2]}mels-{w}-decay{d}" for g, w, d in CHAIN_CASES]
CHAIN_B, CHAIN_CHUNKS, CHAIN_SEED = 2, 3, 5

TOL_STFT_REL, TOL_STFT_ABS = 2e-6, 1e-6
TOL_LOGMEL = 2e-5
TOL_ROWS = 2e-5
TOL_ISTFT = 2e-5
# The direction of a planted bin's output, got / |got| against z / |z|: the kernel rounds hypotf (within 1 ulp), one division per component
# (half an ulp correctly rounded, 2.5 ulp at most otherwise) and the product with the magnitude (half an ulp); 1 + 2.5 + 0.5 = 4 ulp of
# 2^-23 is 4.8e-7 relative, and the bar is twice that.  It does not depend on the magnitude, which the rows bar alone would let hide a
# direction error of 2e-5 / mag.
TOL_DIRECTION = 8 * 2.0 ** -23


def lengths(n_fft):
    hop = n_fft // 2
    return (hop + 1, n_fft - 1, n_fft, 2 * n_fft + hop // 2 + 3)


def chain_length(n_fft):
    """9 hops + 192 samples: T = 10, four chunks of the cell's three-column loop, the last one short"""
    return 9 * (n_fft // 2) + 192


class Checker:
    """One tier's figures: prints every figure (`server-margin ...`, visible with -s; tools/server_margins.py reduces the lines), then holds
    it to min(guard band, bar)"""

    def __init__(self, tier, guard):
        self.tier, self.guard = tier, guard

    def __call__(self, stage, value, bar, detail="", **where):
        print(f"server-margin {stage:<14} tier={self.tier} " + " ".join(f"{k}={v}" for k, v in where.items()) + f" value={value:.2e} bar={bar:.2e}")
        limit = min(self.guard.get(stage, bar), bar)
        assert value <= limit, (stage, where, value, limit, detail() if callable(detail) else detail)


# ------------------------------------------------------------------ plans
class Plan:
    def __init__(self, handle, n_fft, sample_rate, n_mels, fb, pinv, window):
        self.handle, self.n_fft, self.hop, self.K = handle, n_fft, n_fft // 2, n_fft // 2 + 1
        self.sample_rate, self.n_mels, self.fb, self.pinv, self.window = sample_rate, n_mels, fb, pinv, window


def read_tables(lib, handle, n_fft, n_mels):
    """-> (fb (K, M), pinv (K, M), window) as the plan holds them (fp32)"""
    K = n_fft // 2 + 1
    fb, pinv, win = np.zeros((K, max(n_mels, 1)), np.float32), np.zeros((K, max(n_mels, 1)), np.float32), np.zeros(n_fft, np.float32)
    lib.check(lib.dn_dsp_get_tables(handle, fb.ctypes.data_as(C.c_void_p), pinv.ctypes.data_as(C.c_void_p), win.ctypes.data_as(C.c_void_p)))
    return fb[:, :n_mels], pinv[:, :n_mels], win


class Plans:
    """(n_fft, sample rate, n_mels, window name) -> Plan with the HTK filterbank, the pseudo-inverse the library computes itself and the
    named window, built on first use; n_mels = 0 is a plan without mel stages"""

    def __init__(self, abi):
        self.abi, self.made = abi, {}

    def get(self, n_fft, sample_rate, n_mels, name):
        key = (n_fft, sample_rate, n_mels, name)
        if key not in self.made:
            from audio_denoising_amd._lib import DspCfg
            from oracle import dsp_ref
            lib = self.abi.lib
            fb = None if n_mels == 0 else np.ascontiguousarray(dsp_ref.melscale_fbanks(n_fft // 2 + 1, n_mels, sample_rate).numpy(), np.float32)
            w = np.ascontiguousarray(dc.window(name, n_fft), np.float32)
            h = C.c_void_p()
            lib.check(lib.dn_dsp_create(C.byref(DspCfg(sample_rate, n_fft, n_fft // 2, n_mels)), None if fb is None else fb.ctypes.data_as(C.c_void_p),
                                        None, w.ctypes.data_as(C.c_void_p), C.byref(h)))
            tfb, pinv, win = read_tables(lib, h, n_fft, n_mels)
            assert np.array_equal(win, w) and (fb is None or np.array_equal(tfb, fb))
            self.made[key] = Plan(h, n_fft, sample_rate, n_mels, tfb, pinv, win)
        return self.made[key]

    def close(self):
        for p in self.made.values():
            self.abi.lib.dn_dsp_destroy(p.handle)
        self.made = {}


def cplx(a):
    """[...][K][2] float32 -> (..., K) complex128"""
    a = np.asarray(a, np.float64)
    return a[..., 0] + 1j * a[..., 1]


def ri(z):
    """(..., K) complex -> [...][K][2] float32"""
    z = np.asarray(z)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1), dtype=np.float32)


# ------------------------------------------------------------------ the three entry points on a backend
def stft_general(abi, plan, x, want_spec=True, want_logmel=True):
    """one dn_stft_general call -> (spec [B][T][K][2] or None, logmel [B][T][M] or None) as numpy"""
    B, L = x.shape
    T = 1 + L // plan.hop
    xd = abi.up(x)
    spec = abi.nan(B, T, plan.K, 2) if want_spec else None
    logmel = abi.nan(B, T, plan.n_mels) if want_logmel else None
    abi.lib.check(abi.lib.dn_stft_general(plan.handle, abi.ptr(xd), abi.ptr(spec), abi.ptr(logmel), B, L, None))
    return None if spec is None else abi.down(spec), None if logmel is None else abi.down(logmel)


def server_rows(abi, plan, logmel, model_out, spec_in, rows, in_place):
    """one dn_server_rows call on the first `rows` rows -> spec_out [R][K][2] (rows past `rows`: NaN out of place, spec_in in place)"""
    lm, mo, si = abi.up(logmel), abi.up(model_out), abi.up(spec_in)
    so = si if in_place else abi.nan(*spec_in.shape)
    abi.lib.check(abi.lib.dn_server_rows(plan.handle, abi.ptr(lm), abi.ptr(mo), abi.ptr(si), abi.ptr(so), rows, None))
    return abi.down(so)


def istft_general(abi, plan, spec):
    B, T = spec.shape[:2]
    sd, wave = abi.up(spec), abi.nan(B, plan.hop * (T - 1))
    abi.lib.check(abi.lib.dn_istft_general(plan.handle, abi.ptr(sd), abi.ptr(wave), B, T, None))
    return abi.down(wave)


# ------------------------------------------------------------------ analysis
def check_analysis(abi, plans, check, geometry, name, batches):
    """spec and logmel of one dn_stft_general call against server_np64.analysis at every length; the spec-only and the logmel-only call give
    the same bits (it is one kernel)"""
    n_fft, sr, n_mels = geometry
    plan = plans.get(n_fft, sr, n_mels, name)
    where = dict(n_fft=n_fft, n_mels=n_mels, window=name)
    for L in lengths(n_fft):
        T = 1 + L // plan.hop
        for B in batches:
            x = dc.noise((B, L), 1000 + L + B)
            spec, logmel = stft_general(abi, plan, x)
            ref_spec, ref_logmel = server_np64.analysis(x, n_fft, plan.hop, plan.window, plan.fb)
            assert ref_spec.shape == (B, T, plan.K) and ref_logmel.shape == (B, T, n_mels)
            m = float(np.abs(ref_spec).max())
            err = np.abs(cplx(spec) - ref_spec)
            check("spec", float(err.max()) / m, TOL_STFT_REL + TOL_STFT_ABS / m,
                  "max-abs error per column " + ", ".join(f"{err[:, t].max():.2e}" for t in range(T)), L=L, B=B, **where)
            err = np.abs(logmel - ref_logmel)
            check("logmel", float(err.max()), TOL_LOGMEL,
                  "max-abs error per column " + ", ".join(f"{err[:, t].max():.2e}" for t in range(T)), L=L, B=B, **where)
            only_spec, none = stft_general(abi, plan, x, want_logmel=False)
            assert none is None and np.array_equal(only_spec, spec), (L, B, "the spec-only call gives other bits")
            none, only_logmel = stft_general(abi, plan, x, want_spec=False)
            assert none is None and np.array_equal(only_logmel, logmel), (L, B, "the logmel-only call gives other bits")


# ------------------------------------------------------------------ rows
ROWS_B = 2
ROW_FIFTY, ROW_NEGATIVE, ROW_PLANTED = 1, 2, 0
PLANTED = (("zero", 0.0 + 0.0j), ("imaginary", 0.0 - 2.0j), ("tiny", 1e-30 - 1e-30j), ("large", 3e3 + 4e3j))
_ROWS = {}


def rows_case(plan):
    """-> dict(logmel (R, M), model_out (R, M), spec_in [R][K][2] fp32 inputs; ref (R, K) complex128; bins: the four planted bins of row 0;
    mag (R, K) the float64 magnitudes).  logmel and the spectrum are the float64 analysis of noise at the ragged length (R = 2 x 5 rows),
    rounded to fp32; model_out is N(0, 1) with a run of 50s in row 1 (exp(logmel - 150) - 1 = -1) and row 2 all negative (the relu zeroes
    it).  The planted bins are the four of row 0 where the float64 magnitude is largest, so that the phasor's direction shows in the output."""
    key = (plan.n_fft, plan.n_mels)
    if key not in _ROWS:
        L = lengths(plan.n_fft)[-1]
        spec, logmel = server_np64.analysis(dc.noise((ROWS_B, L), 2000 + plan.n_fft + plan.n_mels), plan.n_fft, plan.hop, None, plan.fb)
        R, M = ROWS_B * spec.shape[1], plan.n_mels
        logmel = logmel.reshape(R, M).astype(np.float32)
        spec = spec.reshape(R, plan.K).astype(np.complex64)
        rng = np.random.default_rng(2100 + plan.n_fft + plan.n_mels)
        model_out = rng.standard_normal((R, M)).astype(np.float32)
        model_out[ROW_FIFTY, 3:11] = 50.0
        model_out[ROW_NEGATIVE] = -np.abs(model_out[ROW_NEGATIVE]) - 0.01
        mm = server_np64.mel_magnitude(logmel, model_out)
        pre = mm @ plan.pinv.astype(np.float64).T
        mag = np.maximum(pre, 0.0)
        bins = np.sort(np.argsort(mag[ROW_PLANTED])[-len(PLANTED):])
        for k, (_, z) in zip(bins, PLANTED):
            spec[ROW_PLANTED, k] = z
        spec_in = ri(spec)
        tiny = np.abs(spec_in[spec_in != 0]).min()
        assert tiny >= 1e-30 > np.finfo(np.float32).tiny and np.abs(spec_in).max() < 1e5 and np.isfinite(logmel).all()       # no denormals
        # the branches are live, on the reference alone: exp(.) - 1 < 0 somewhere, the inverse mel's relu clamps some bins and not others,
        # the model's relu clamps some entries, row 2 keeps its log-mel magnitudes (relu(out) = 0 all along)
        assert (mm < 0).any() and (mm[ROW_FIFTY, 3:11] == -1.0).all()
        assert (pre < 0).any() and (pre > 0).any() and (model_out < 0).any() and (model_out > 0).any()
        assert np.allclose(mm[ROW_NEGATIVE], np.expm1(logmel[ROW_NEGATIVE].astype(np.float64)), rtol=1e-12, atol=0)
        assert mag[ROW_PLANTED, bins].min() > 1.0, mag[ROW_PLANTED, bins]
        ref = server_np64.rows(logmel, model_out, cplx(spec_in), plan.pinv)
        assert np.abs(ref[ROW_NEGATIVE]).max() > 1.0
        _ROWS[key] = dict(logmel=logmel, model_out=model_out, spec_in=spec_in, ref=ref, bins=bins, mag=mag)
        for a in _ROWS[key].values():
            a.setflags(write=False)
    return _ROWS[key]


def check_rows(abi, plans, check, geometry):
    """dn_server_rows on the rows case against server_np64.rows at rows = B T and rows = 1, in place and out of place; the planted bins"""
    n_fft, sr, n_mels = geometry
    plan = plans.get(n_fft, sr, n_mels, "hann")
    c = rows_case(plan)
    R = c["ref"].shape[0]
    scale = max(1.0, float(np.abs(c["ref"]).max()))
    where = dict(n_fft=n_fft, n_mels=n_mels)
    out = server_rows(abi, plan, c["logmel"], c["model_out"], c["spec_in"], R, in_place=False)
    err = np.abs(cplx(out) - c["ref"])
    check("rows", float(err.max()) / scale, TOL_ROWS, "max-abs error per row " + ", ".join(f"{e:.2e}" for e in err.max(axis=1)), rows=R, **where)
    same = server_rows(abi, plan, c["logmel"], c["model_out"], c["spec_in"], R, in_place=True)
    assert np.array_equal(same, out), "in place and out of place give other bits"
    # rows = 1: the first row alone, nothing written behind it
    one = server_rows(abi, plan, c["logmel"], c["model_out"], c["spec_in"], 1, in_place=False)
    assert np.isnan(one[1:]).all() and np.array_equal(one[0], out[0]), "rows = 1 writes other bits, or past its row"
    one = server_rows(abi, plan, c["logmel"], c["model_out"], c["spec_in"], 1, in_place=True)
    assert np.array_equal(one[1:], c["spec_in"][1:]) and np.array_equal(one[0], out[0])
    # the planted bins, one by one
    got = cplx(out[ROW_PLANTED])
    for k, (what, z) in zip(c["bins"], PLANTED):
        mag, g = float(c["mag"][ROW_PLANTED, k]), got[k]
        check("rows", abs(abs(g) - mag) / scale, TOL_ROWS, rows=R, bin=what, **where)
        if what == "zero":
            assert g.imag == 0.0 and g.real > 0.0, (what, g)                     # angle(0) = 0: (mag, 0)
        elif what == "imaginary":
            assert g.real == 0.0 and g.imag < 0.0, (what, g)                     # (0, -mag); the sign of the zero is not compared
        else:
            check("direction", abs(g / abs(g) - z / abs(z)), TOL_DIRECTION, rows=R, bin=what, **where)


# ------------------------------------------------------------------ synthesis
def istft_spectrum(B, T, n_fft, seed):
    """(B, T, K) complex64 random spectrum, NOT consistent, with real DC and Nyquist bins (numpy's irfft ignores their imaginary part and the
    kernel is not specified there), scaled so that the waveform has RMS ~ 1"""
    rng = np.random.default_rng(seed)
    K = n_fft // 2 + 1
    z = (rng.standard_normal((B, T, K)) + 1j * rng.standard_normal((B, T, K))) * (16.0 * np.sqrt(n_fft / 1024.0))
    z[:, :, 0] = z[:, :, 0].real
    z[:, :, -1] = z[:, :, -1].real
    return z.astype(np.complex64)


def check_istft(abi, plans, check, n_fft, name, batches):
    plan = plans.get(n_fft, dc.HOP_GEOMETRY[n_fft][0], 0, name)
    for T in ISTFT_T:
        for B in batches:
            z = istft_spectrum(B, T, n_fft, 3000 + n_fft + 10 * T + B)
            wave = istft_general(abi, plan, ri(z))
            ref = server_np64.synthesis(z, n_fft, plan.hop, plan.window)
            assert ref.shape == wave.shape == (B, plan.hop * (T - 1))
            err = np.abs(wave - ref)
            check("istft", float(err.max()) / float(np.abs(ref).max()), TOL_ISTFT,
                  "max-abs error per output hop " + ", ".join(f"{err[:, k * plan.hop:(k + 1) * plan.hop].max():.2e}" for k in range(T - 1))
                  + f"; sample 0 {err[:, 0].max():.2e}", n_fft=n_fft, window=name, T=T, B=B)


# ------------------------------------------------------------------ the chain
_CHAINS = {}


def chain_chunks(n_fft):
    """(3, B, L) fp32 white noise of amplitude 1.0.  (At 0.1 the synthetic model's output is positive in 76 .. 98 % of the entries: its relu
    would hardly clamp.)"""
    return dc.noise((CHAIN_CHUNKS, CHAIN_B, chain_length(n_fft)), CHAIN_SEED)


def chain_reference(geometry, name, hx_decay, fb):
    """Three consecutive requests through server_np64.process_chunk64 with the synthetic hop blob, hx carried -> list of dict(out, hx).
    fb: the plan's fp32 filterbank.  Asserts, on float64 alone, that the model stage is live: 25 .. 90 % of model_out positive, the waveform
    at least 10 % RMS away from the one with model_out = 0, the output RMS at least 10 % of the input's."""
    key = (geometry, name, hx_decay)
    if key not in _CHAINS:
        n_fft, _, n_mels = geometry
        hop, w, m64 = n_fft // 2, dc.window(name, n_fft), mc.hop_model64()
        hx = np.zeros((CHAIN_B, 17, n_mels // 16))
        res = []
        for x in chain_chunks(n_fft):
            r = server_np64.process_chunk64(x, hx, m64, n_fft, hop, w, fb, hx_decay)
            off = server_np64.process_chunk64(x, hx, m64, n_fft, hop, w, fb, hx_decay, zero_model_out=True)["out"]
            assert r["model_out"].shape == (CHAIN_B, 10, n_mels) and r["out"].shape == (CHAIN_B, 9 * hop)
            positive = float((r["model_out"] > 0).mean())
            rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))          # noqa: E731
            moved, level = rms(r["out"] - off) / rms(off), rms(r["out"]) / rms(x)
            print(f"server-chain reference n_fft={n_fft} n_mels={n_mels} window={name} decay={hx_decay}: model_out positive {positive:.2f}, "
                  f"waveform moved by the model {moved:.2f}, output RMS / input RMS {level:.2f}")
            assert 0.25 <= positive <= 0.90 and moved >= 0.10 and level >= 0.10, (positive, moved, level)
            hx = r["hx"]
            res.append(dict(out=r["out"], hx=r["hx"]))
        _CHAINS[key] = res
    return _CHAINS[key]


def check_chain(check, geometry, name, hx_decay, fb, run):
    """run(chunk index, x (B, L) fp32, hx or None) -> (wave, hx) as numpy, hx handed on by the caller as the tier carries it"""
    n_fft, _, n_mels = geometry
    refs = chain_reference(geometry, name, hx_decay, fb)
    hx = None
    for c, (x, ref) in enumerate(zip(chain_chunks(n_fft), refs)):
        wave, hx_np, hx = run(c, x, hx)
        assert wave.shape == ref["out"].shape and hx_np.shape == ref["hx"].shape
        rms, mx, scale = dc.wave_errors(wave, ref["out"])
        err = np.abs(wave - ref["out"])
        hop = n_fft // 2
        per_hop = lambda: "max-abs error per output hop " + ", ".join(f"{err[:, k * hop:(k + 1) * hop].max():.2e}" for k in range(9))      # noqa: E731
        where = dict(n_fft=n_fft, n_mels=n_mels, window=name, decay=hx_decay, chunk=c)
        check("chain_rms", rms / scale, TOL_WAVE_RMS, per_hop, **where)
        check("chain_max", mx / scale, TOL_WAVE_MAX, per_hop, **where)
        check("chain_hx", float(np.abs(hx_np - ref["hx"]).max()), TOL_HX_STREAM, **where)


def abi_chain_runner(abi, plan, hx_decay):
    """the four ABI calls of one request (as ServerDenoiser.process makes them: dn_server_rows in place) on a backend"""
    lib, Cb = abi.lib, plan.n_mels // 16
    model = abi.model(mc.hop_blob(), Cb)

    def run(c, x, hx):
        B, L = x.shape
        T = 1 + L // plan.hop
        xd, hx0 = abi.up(x), abi.up(np.zeros((B, 17, Cb), np.float32)) if hx is None else hx
        spec, logmel, out, hx1, wave = abi.nan(B, T, plan.K, 2), abi.nan(B, T, plan.n_mels), abi.nan(B, T, plan.n_mels), abi.nan(B, 17, Cb), abi.nan(B, plan.hop * (T - 1))
        lib.check(lib.dn_stft_general(plan.handle, abi.ptr(xd), abi.ptr(spec), abi.ptr(logmel), B, L, None))
        lib.check(lib.dn_cell_forward_ex(model, abi.ptr(logmel), abi.ptr(hx0), abi.ptr(out), abi.ptr(hx1), B, T, plan.n_mels, Cb, C.c_float(hx_decay), None))
        lib.check(lib.dn_server_rows(plan.handle, abi.ptr(logmel), abi.ptr(out), abi.ptr(spec), abi.ptr(spec), B * T, None))
        lib.check(lib.dn_istft_general(plan.handle, abi.ptr(spec), abi.ptr(wave), B, T, None))
        return abi.down(wave), abi.down(hx1), hx1

    return run, lambda: lib.dn_model_destroy(model)


# ------------------------------------------------------------------ refusals
def check_refusals(abi, plans):
    """Every refusal returns DN_ERR_INVALID with a message before anything is launched: the NaN-filled outputs stay NaN.  B = 0 and rows = 0
    return DN_OK and touch nothing."""
    lib = abi.lib
    mel, bare = plans.get(512, 16000, 64, "hann"), plans.get(512, 16000, 0, "hann")
    hop, K, M, B, T = mel.hop, mel.K, mel.n_mels, 2, 3
    x = abi.up(dc.noise((B, 2 * hop), 4000))
    spec, logmel, wave, rows_out = abi.nan(B, T, K, 2), abi.nan(B, T, M), abi.nan(B, hop * (T - 1)), abi.nan(B * T, K, 2)
    lm_in, mo_in, sp_in = abi.up(np.zeros((B * T, M))), abi.up(np.zeros((B * T, M))), abi.up(np.ones((B * T, K, 2)))
    p = abi.ptr

    def untouched():
        return all(np.isnan(abi.down(t)).all() for t in (spec, logmel, wave, rows_out))

    def refused(rc, *words):
        msg = lib.dn_last_error().decode("utf-8", "replace")
        assert rc == DN_ERR_INVALID and msg and all(w in msg for w in words), (rc, msg, words)
        assert untouched(), msg

    refused(lib.dn_stft_general(mel.handle, p(x), p(spec), p(logmel), B, hop, None), "dn_stft_general", "n_fft/2")          # L = hop
    refused(lib.dn_stft_general(mel.handle, p(x), None, None, B, 2 * hop, None), "dn_stft_general", "null")
    refused(lib.dn_stft_general(bare.handle, p(x), p(spec), p(logmel), B, 2 * hop, None), "without mel stages")
    refused(lib.dn_stft_general(mel.handle, p(x), p(spec), p(logmel), -1, 2 * hop, None), "dn_stft_general", "negative")
    refused(lib.dn_server_rows(bare.handle, p(lm_in), p(mo_in), p(sp_in), p(rows_out), B * T, None), "without mel stages")
    refused(lib.dn_server_rows(mel.handle, p(lm_in), p(mo_in), p(sp_in), p(rows_out), -1, None), "dn_server_rows", "negative")
    refused(lib.dn_istft_general(mel.handle, p(sp_in), p(wave), B, 1, None), "dn_istft_general", "2 columns")             # T = 1
    refused(lib.dn_istft_general(mel.handle, p(sp_in), p(wave), -1, T, None), "dn_istft_general")
    # nothing to do
    assert lib.dn_stft_general(mel.handle, p(x), p(spec), p(logmel), 0, 2 * hop, None) == DN_OK
    assert lib.dn_server_rows(mel.handle, p(lm_in), p(mo_in), p(sp_in), p(rows_out), 0, None) == DN_OK
    assert lib.dn_istft_general(mel.handle, p(sp_in), p(wave), 0, T, None) == DN_OK
    assert untouched()
    # (the bare plan does run the spectrum alone)
    lib.check(lib.dn_stft_general(bare.handle, p(x), p(spec), None, B, 2 * hop, None))
    assert np.isfinite(abi.down(spec)).all() and np.isnan(abi.down(logmel)).all()
