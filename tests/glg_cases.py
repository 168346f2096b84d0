"""Shared cases of the any-length Griffin-Lim tests (tests/test_oracle_glg.py, tests/test_emu_glg.py, tests/test_gpu_glg.py,
tools/glg_margins.py): inputs, float64 references (oracle/dsp_np64.griffinlim, oracle/server_np64.py), the conditioning table and the checks
both tiers run.  TEST INFRASTRUCTURE; the kernels are run by the backend a test hands in (tests/model_abi.Abi).

dn_griffinlim_general has two forms that must give the same bits: WHOLE (one launch, T <= WHOLE_MAX columns on chip) and STEPS (two launches
an iteration, any T).  Shapes are the smallest that reach each branch: T = 3 (both reflections land in blocks 0 and 1), T = 4 (one middle
column), T = WHOLE_MAX (the last on-chip size), WHOLE_MAX + 1 (the first STEPS-only size), 19 (several workgroups of middle columns).

Conditioning.  Griffin-Lim amplifies rounding with a heavy tail (tests/dsp_cases.py, GL32_SEED_K).  A batch is used only if the float64
reference alone moves no stream by more than 1e-4 RMS (at scale max(1, RMS)) under two 1e-7 relative perturbations of the magnitudes;
SEED_K holds the first such candidate k per case, computed from the reference alone; tests/test_oracle_glg.py derives it again on the CPU.

Bars are the project's waveform bars (TOL_WAVE_RMS 1e-3, TOL_WAVE_MAX 2e-2 at scale max(1, RMS of the float64 waveform)); a tier's guard
bands (10 x the worst measured there, profiles/glg_parity_margins.txt) sit beside them, never above.
"""
import ctypes as C

import numpy as np
import torch

import dsp_cases as dc
import model_cases as mc
import server_cases as sc
from oracle import dsp_np64, philox_ref, server_np64
from test_gpu_parity import TOL_WAVE_MAX, TOL_WAVE_RMS

DN_OK, DN_ERR_INVALID, DN_ERR_UNSUPPORTED = 0, -1, -2
WHOLE, STEPS, NORMALIZE = 2, 4, 16           # DN_GLG_WHOLE, DN_GLG_STEPS, DN_GL_INIT_NORMALIZE
WHOLE_MAX = 8                                # dn_griffinlim_general_whole_max (asserted by both tiers)
BATCH = 3                                    # the conditioning rule's batch; the emulator runs the first two streams of it
N_ITER, MOMENTUM = 8, 0.99


def magnitudes(B, n_fft, T, seed):
    """dsp_cases.magnitudes generalised to T columns: (B, K, T) fp32 magnitudes scaled for a waveform RMS ~ 1 and (B, K, T) complex64 phases
    with real and imaginary parts ~ U[0, 1)"""
    g = torch.Generator().manual_seed(seed)
    K = n_fft // 2 + 1
    mag = torch.rand(B, K, T, generator=g) * (46.0 * np.sqrt(n_fft / 1024.0))
    init = torch.rand(B, K, T, dtype=torch.complex64, generator=g)
    return mag.numpy(), init.numpy()


def seed_of(n_fft, T, n_iter, k):
    return 7000 + n_fft + 10 * T + n_iter + 1000 * k


def reference(mag, init, n_fft, name, n_iter, momentum):
    return dsp_np64.griffinlim(np.asarray(mag, np.float64), n_fft, n_fft // 2, init, n_iter=n_iter, momentum=momentum, window=dc.window(name, n_fft))


def is_well_conditioned(mag, init, n_fft, name, n_iter, momentum, trials=2, relative=1e-7, limit=1e-4):
    """the rule of dsp_cases.gl32_batch_is_well_conditioned on any (B, K, T) batch"""
    mag = np.asarray(mag, np.float64)
    ref = reference(mag, init, n_fft, name, n_iter, momentum)
    scale = np.maximum(1.0, np.sqrt(np.mean(ref ** 2, axis=1)))
    rg = np.random.default_rng(1)
    for _ in range(trials):
        y = reference(mag * (1.0 + relative * rg.standard_normal(mag.shape)), init, n_fft, name, n_iter, momentum)
        if (np.sqrt(np.mean((y - ref) ** 2, axis=1)) / scale).max() > limit:
            return False
    return True


def first_well_conditioned_k(n_fft, name, T, n_iter, momentum, k_max=8):
    for k in range(k_max):
        mag, init = magnitudes(BATCH, n_fft, T, seed_of(n_fft, T, n_iter, k))
        if is_well_conditioned(mag, init, n_fft, name, n_iter, momentum):
            return k
    raise AssertionError((n_fft, name, T, n_iter, momentum, "no well-conditioned candidate"))


# (n_fft, window, T, n_iter, momentum) -> first well-conditioned candidate k: 0 unless listed.  Computed from the reference alone
# (first_well_conditioned_k); tests/test_oracle_glg.py derives every entry again on the CPU, so the table cannot go stale.
_SEED_K_NOT_0 = {(512, "asym", 3, 8, 0.99): 1, (512, "asym", 5, 8, 0.99): 1, (1024, "asym", 4, 4, 0.99): 1, (1024, "asym", 5, 8, 0.99): 1,
                 (1024, "hamming", 9, 8, 0.99): 1}


class _SeedK(dict):
    def __missing__(self, key):
        return 0


SEED_K = _SeedK(_SEED_K_NOT_0)

# ------------------------------------------------------------------ the parity cases of a tier: (n_fft, window, T, n_iter, momentum, form)
EMU_WHOLE_T, EMU_STEPS_T = (3, 4, 5), (3, 9)
GPU_WHOLE_T, GPU_STEPS_T = (3, 4, WHOLE_MAX), (3, WHOLE_MAX + 1, 19)


def parity_cases(tier):
    whole_t, steps_t = (EMU_WHOLE_T, EMU_STEPS_T) if tier == "emu" else (GPU_WHOLE_T, GPU_STEPS_T)
    cases = [(n, w, T, N_ITER, MOMENTUM, form) for n in dc.N_FFTS for w in dc.WINDOWS
             for form, ts in ((WHOLE, whole_t), (STEPS, steps_t)) for T in ts]
    cases += [(n, "hann", whole_t[-1], 32, MOMENTUM, WHOLE) for n in dc.N_FFTS]
    cases += [(1024, "asym", 4, N_ITER, 0.0, WHOLE), (512, "hamming", 9, N_ITER, 0.5, STEPS)]
    return cases


def case_id(c):
    return f"{c[0]}-{c[1]}-T{c[2]}-it{c[3]}-m{c[4]}-{'whole' if c[5] == WHOLE else 'steps'}"


def all_keys():
    keys = {c[:5] for tier in ("emu", "gpu") for c in parity_cases(tier)}
    keys |= {(n, "asym", 4, 4, MOMENTUM) for n in dc.N_FFTS}                 # the DN_GL_INIT_NORMALIZE cases
    return sorted(keys)


_INPUTS, _REFS = {}, {}


def inputs(key):
    """key = (n_fft, window, T, n_iter, momentum) -> (mag (B, K, T) fp32, init (B, K, T) complex64) of the table's candidate"""
    if key not in _INPUTS:
        n_fft, _, T, n_iter, _ = key
        mag, init = magnitudes(BATCH, n_fft, T, seed_of(n_fft, T, n_iter, SEED_K[key]))
        mag.setflags(write=False)
        init.setflags(write=False)
        _INPUTS[key] = (mag, init)
    return _INPUTS[key]


def case_reference(key):
    if key not in _REFS:
        mag, init = inputs(key)
        _REFS[key] = reference(mag, init, key[0], key[1], key[3], key[4])
        _REFS[key].setflags(write=False)
    return _REFS[key]


class Checker:
    """One tier's figures: prints every figure (`glg-margin ...`, visible with -s; tools/glg_margins.py reduces the lines), then holds it to
    min(guard band, bar)"""

    def __init__(self, tier, guard):
        self.tier, self.guard = tier, guard

    def __call__(self, stage, value, bar, detail="", **where):
        print(f"glg-margin {stage:<14} tier={self.tier} " + " ".join(f"{k}={v}" for k, v in where.items()) + f" value={value:.2e} bar={bar:.2e}")
        limit = min(self.guard.get(stage, bar), bar)
        assert value <= limit, (stage, where, value, limit, detail() if callable(detail) else detail)

    def band(self, stage, bar):
        return min(self.guard.get(stage, bar), bar)


# ------------------------------------------------------------------ the entry points on a backend
def rows_of(a):
    """(B, K, T) real -> [B][T][K] fp32"""
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 1), np.float32)


def plan_of(plans, n_fft, name):
    return plans.get(n_fft, dc.HOP_GEOMETRY[n_fft][0], 0, name)


def workspace(abi, plan, B, T):
    n = int(abi.lib.dn_griffinlim_general_workspace_bytes(plan.handle, B, T))
    assert n > 0
    return abi.up(np.zeros(n // 4, np.float32))


def run_general(abi, plan, mag, init, n_iter, momentum, flags, seed=0, sid0=0):
    """mag (B, K, T), init (B, K, T) complex or None -> wave (B, hop (T - 1)) through one dn_griffinlim_general call"""
    B, _, T = mag.shape
    md, idv = abi.up(rows_of(mag)), None if init is None else abi.up(dc.ri(init))
    wave, ws = abi.nan(B, plan.hop * (T - 1)), workspace(abi, plan, B, T)
    abi.lib.check(abi.lib.dn_griffinlim_general(plan.handle, abi.ptr(md), abi.ptr(idv), seed, sid0, abi.ptr(wave), abi.ptr(ws), B, T, n_iter,
                                                C.c_float(momentum), flags, None))
    return abi.down(wave)


def run_hop_chain(abi, plan, mag, init, n_iter, momentum, seed=0, sid0=0):
    """the 3-column dn_griffinlim on the same layout"""
    B = mag.shape[0]
    md, idv = abi.up(rows_of(mag)), None if init is None else abi.up(dc.ri(init))
    wave = abi.nan(B, plan.n_fft)
    abi.lib.check(abi.lib.dn_griffinlim(plan.handle, abi.ptr(md), abi.ptr(idv), seed, sid0, None, abi.ptr(wave), B, n_iter, C.c_float(momentum), None))
    return abi.down(wave)


def draw_general(abi, plan, seed, sid0, B, T):
    out = abi.nan(B, T, plan.K, 2)
    abi.lib.check(abi.lib.dn_griffinlim_draw_phases_general(plan.handle, seed, sid0, abi.ptr(out), B, T, None))
    return abi.down(out)


def hop_error_pattern(err, hop):
    return "max-abs error per output hop " + ", ".join(f"{err[:, k * hop:(k + 1) * hop].max():.2e}" for k in range(err.shape[1] // hop)) \
        + f"; sample 0 {err[:, 0].max():.2e}, last {err[:, -1].max():.2e}"


# ------------------------------------------------------------------ 1. parity with float64
def check_parity(abi, plans, check, case, batch):
    n_fft, name, T, n_iter, momentum, form = case
    key = case[:5]
    plan = plan_of(plans, n_fft, name)
    mag, init = inputs(key)
    ref = case_reference(key)[:batch]
    got = run_general(abi, plan, mag[:batch], init[:batch], n_iter, momentum, form)
    assert got.shape == ref.shape == (batch, plan.hop * (T - 1))
    rms, mx, scale = dc.wave_errors(got, ref)
    err = np.abs(got - ref)
    stage = "whole" if form == WHOLE else "steps"
    where = dict(n_fft=n_fft, window=name, T=T, n_iter=n_iter, momentum=momentum)
    check(stage + "_rms", rms / scale, TOL_WAVE_RMS, lambda: hop_error_pattern(err, plan.hop), **where)
    check(stage + "_max", mx / scale, TOL_WAVE_MAX, lambda: hop_error_pattern(err, plan.hop), **where)


# ------------------------------------------------------------------ 2. WHOLE and STEPS, bit for bit; 3. n_iter = 0
BITS_N_ITER = (0, 1, 7, 8)


def check_forms_agree(abi, plans, n_fft, Ts, batch):
    """injected phases and the device draw, every n_iter of BITS_N_ITER, under the asymmetric window"""
    plan = plan_of(plans, n_fft, "asym")
    for T in Ts:
        mag, init = magnitudes(batch, n_fft, T, 8100 + n_fft + T)
        for n_iter in BITS_N_ITER:
            for ia in (init, None):
                a = run_general(abi, plan, mag, ia, n_iter, MOMENTUM, WHOLE, seed=5, sid0=9)
                b = run_general(abi, plan, mag, ia, n_iter, MOMENTUM, STEPS, seed=5, sid0=9)
                assert np.isfinite(a).all() and float(np.sqrt(np.mean(a.astype(np.float64) ** 2))) > 0.1
                assert np.array_equal(a, b), (n_fft, T, n_iter, "injected" if ia is not None else "drawn", float(np.abs(a - b).max()),
                                              hop_error_pattern(np.abs(a - b), plan.hop))
                if ia is not None:               # with neither flag WHOLE runs where it fits: the same bits either way
                    assert np.array_equal(run_general(abi, plan, mag, ia, n_iter, MOMENTUM, 0), a)


def check_zero_iterations(abi, plans, n_fft, Ts, batch):
    """n_iter = 0 is dn_istft_general of init * mag (multiplied in fp32 on the host), bit for bit, in both forms"""
    plan = plan_of(plans, n_fft, "asym")
    for T in Ts:
        mag, init = magnitudes(batch, n_fft, T, 8200 + n_fft + T)
        z = dc.ri(init) * rows_of(mag)[..., None]                       # fp32 products
        want = sc.istft_general(abi, plan, z)
        for form in (WHOLE, STEPS) if T <= WHOLE_MAX else (STEPS,):
            got = run_general(abi, plan, mag, init, 0, MOMENTUM, form)
            assert np.array_equal(got, want), (n_fft, T, form, float(np.abs(got - want).max()))


# ------------------------------------------------------------------ 4. T = 3 against the hop chain
def check_against_hop_chain(abi, plans, check, n_fft, name, batch):
    """dn_griffinlim_general(T = 3) and dn_griffinlim on the same inputs: apart by no more than the sum of their two guard bands (other
    rounding is allowed, another algorithm is not).  The hop chain's Griffin-Lim stages have no guard band below their bars on either tier
    (tests/test_gpu_windows.py: ten times the worst measured is above the bar), so its band is the bar itself."""
    key = (n_fft, name, 3, N_ITER, MOMENTUM)
    plan = plan_of(plans, n_fft, name)
    mag, init = inputs(key)
    ref = case_reference(key)[:batch]
    a = run_general(abi, plan, mag[:batch], init[:batch], N_ITER, MOMENTUM, WHOLE)
    b = run_hop_chain(abi, plan, mag[:batch], init[:batch], N_ITER, MOMENTUM)
    rms, mx, scale = dc.wave_errors(a, b.astype(np.float64))
    scale = max(1.0, float(np.sqrt(np.mean(ref ** 2))))
    where = dict(n_fft=n_fft, window=name)
    check("hop_pair_rms", rms / scale, check.band("whole_rms", TOL_WAVE_RMS) + TOL_WAVE_RMS, **where)
    check("hop_pair_max", mx / scale, check.band("whole_max", TOL_WAVE_MAX) + TOL_WAVE_MAX, **where)


# ------------------------------------------------------------------ 5. device phases
def philox_column(seed, sid, col, n_stft):
    """(n_stft,) complex64: column `col` of stream `sid`, restated from oracle/philox_ref.py's block numbering"""
    nc = n_stft - 1
    m = np.arange(nc // 2 + 1, dtype=np.uint64)
    n = len(m)
    unit = lambda w: (w >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)      # noqa: E731
    w = philox_ref.philox4x32_10(m, np.full(n, col, np.uint64), np.full(n, sid & 0xFFFFFFFF, np.uint64), np.full(n, (sid >> 32) & 0xFFFFFFFF, np.uint64),
                                 seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty(n_stft, np.complex64)
    out[nc - m.astype(np.int64)] = unit(w[2]) + 1j * unit(w[3])
    out[m.astype(np.int64)] = unit(w[0]) + 1j * unit(w[1])
    return out


def check_device_phases(abi, plans, n_fft, T_null):
    plan = plan_of(plans, n_fft, "hamming")
    seed, sid0, B = (1 << 40) + 77, (1 << 33) + 5, 5
    d3, d9 = draw_general(abi, plan, seed, sid0, 2, 3), draw_general(abi, plan, seed, sid0, 2, 9)
    old = abi.nan(2, 3, plan.K, 2)
    abi.lib.check(abi.lib.dn_griffinlim_draw_phases(plan.handle, seed, sid0, abi.ptr(old), 2, None))
    assert np.array_equal(d3, abi.down(old)), "draw_phases_general(T = 3) is not dn_griffinlim_draw_phases"
    assert np.array_equal(d9[:, :3], d3), "the first 3 columns of a T = 9 draw are not the T = 3 draw"
    want = philox_column(seed, sid0 + 1, 7, plan.K)
    got = d9[1, 7, :, 0] + 1j * d9[1, 7, :, 1]
    assert np.array_equal(got.astype(np.complex64), want), "column 7 of stream 1 is not oracle/philox_ref's"
    # a NULL-phase run is the run fed the drawn phases; stream b of a batch is the stream alone with stream_id0 + b
    mag, _ = magnitudes(B, n_fft, T_null, 8300 + n_fft)
    drawn = draw_general(abi, plan, seed, sid0, B, T_null)
    zi = (drawn[..., 0] + 1j * drawn[..., 1]).transpose(0, 2, 1).astype(np.complex64)
    for form in (WHOLE, STEPS) if T_null <= WHOLE_MAX else (STEPS,):
        null = run_general(abi, plan, mag, None, 3, MOMENTUM, form, seed, sid0)
        fed = run_general(abi, plan, mag, zi, 3, MOMENTUM, form, seed, sid0)
        assert np.isfinite(null).all() and np.array_equal(null, fed), (form, "the NULL-phase run is not the run fed the drawn phases")
        for b in (0, 3, 4):
            alone = run_general(abi, plan, mag[b:b + 1], None, 3, MOMENTUM, form, seed, sid0 + b)
            assert np.array_equal(alone[0], null[b]), (form, b, "a stream alone draws other phases")


# ------------------------------------------------------------------ 6. DN_GL_INIT_NORMALIZE
PLANTED = ((0.0 + 0.0j), (1e-30 - 1e-30j), (3e3 + 4e3j))


def normalize_case(n_fft):
    """-> (mag (B, K, T) fp32, spectrum (B, K, T) complex64 with planted bins in stream 0 / column 1, float64-normalised phasors rounded to
    fp32, the planted bins).  The spectrum is the case's phases times a positive random level, so its phasors are the phases' directions."""
    key = (n_fft, "asym", 4, 4, MOMENTUM)
    mag, init = inputs(key)
    rng = np.random.default_rng(8400 + n_fft)
    spec = (init.astype(np.complex128) * rng.uniform(0.5, 20.0, init.shape)).astype(np.complex64)
    bins = np.sort(np.argsort(mag[0, :, 1])[-len(PLANTED):])
    for k, z in zip(bins, PLANTED):
        spec[0, k, 1] = z
    re, im = spec.real.astype(np.float64), spec.imag.astype(np.float64)
    p = re * re + im * im
    tiny = p < float(np.finfo(np.float32).tiny)             # the kernel's rule: |X|^2 below the smallest normal float counts as zero
    unit = np.where(tiny, 1.0 + 0.0j, (re + 1j * im) / np.sqrt(np.where(tiny, 1.0, p))).astype(np.complex64)
    assert tiny.sum() == 2 and unit[0, bins[0], 1] == 1.0 and unit[0, bins[1], 1] == 1.0 and abs(unit[0, bins[2], 1] - (0.6 + 0.8j)) < 1e-7
    return mag, spec, unit, bins


def check_init_normalize(abi, plans, check, n_fft, batch):
    plan = plan_of(plans, n_fft, "asym")
    mag, spec, unit, bins = normalize_case(n_fft)
    mag, spec, unit = mag[:batch], spec[:batch], unit[:batch]
    T = mag.shape[2]
    # n_iter = 0 in the spectral domain: the run's samples are istft(u * mag); feed one bin at a time?  No: compare the waveforms of the
    # normalised run and the run fed the float64 phasors -- both go through the same istft, so 8 ulp per phasor component bounds the
    # waveform difference by 8 ulp of sum_k mag / NC x window peak, which the direction bar states relative to the waveform's peak.
    for form in (WHOLE, STEPS):
        a = run_general(abi, plan, mag, spec, 0, MOMENTUM, form | NORMALIZE)
        b = run_general(abi, plan, mag, unit, 0, MOMENTUM, form)
        amp = float(np.abs(b).max())
        # every bin's phasor is off by at most TOL_DIRECTION; a sample sums K bins of magnitude mag / (NC envelope): bound by the l1 norm
        bound = sc.TOL_DIRECTION * float(np.abs(rows_of(mag)).sum(axis=2).max()) / (n_fft // 2) * 2.0 * float(np.abs(plan.window).max()) / float(dc.envelope(plan.window).min())
        check("normalize0", float(np.abs(a - b).max()) / amp, bound / amp, n_fft=n_fft, form=form)
        ref = reference(mag, unit, n_fft, "asym", 4, MOMENTUM)
        got = run_general(abi, plan, mag, spec, 4, MOMENTUM, form | NORMALIZE)
        rms, mx, scale = dc.wave_errors(got, ref)
        check("normalize4_rms", rms / scale, TOL_WAVE_RMS, n_fft=n_fft, form=form)
        check("normalize4_max", mx / scale, TOL_WAVE_MAX, n_fft=n_fft, form=form)
    # the planted bins themselves, through a one-hot magnitude: the waveform of a single bin IS its phasor's direction
    for k, z in zip(bins, PLANTED):
        hot = np.zeros_like(mag[:1])
        hot[0, k, 1] = 1000.0
        a = run_general(abi, plan, hot, spec[:1], 0, MOMENTUM, WHOLE | NORMALIZE)
        b = run_general(abi, plan, hot, unit[:1], 0, MOMENTUM, WHOLE)
        check("direction", float(np.abs(a - b).max()) / float(np.abs(b).max()), sc.TOL_DIRECTION, n_fft=n_fft, bin=str(z))


# ------------------------------------------------------------------ 7. dn_server_mag
MAG_GEOMETRIES = [(512, 16000, 64), (1024, 16000, 80), (1536, 48000, 40)]


def check_server_mag(abi, plans, check, geometry):
    n_fft, sr, n_mels = geometry
    plan = plans.get(n_fft, sr, n_mels, "hann")
    c = sc.rows_case(plan)
    R = c["ref"].shape[0]
    lm, mo, out = abi.up(c["logmel"]), abi.up(c["model_out"]), abi.nan(R, plan.K)
    abi.lib.check(abi.lib.dn_server_mag(plan.handle, abi.ptr(lm), abi.ptr(mo), abi.ptr(out), R, None))
    got = abi.down(out)
    ref = np.maximum(server_np64.mel_magnitude(c["logmel"], c["model_out"]) @ plan.pinv.astype(np.float64).T, 0.0)
    scale = max(1.0, float(np.abs(ref).max()))
    check("mag_rows", float(np.abs(got - ref).max()) / scale, sc.TOL_ROWS, n_fft=n_fft, n_mels=n_mels)
    polar = sc.server_rows(abi, plan, c["logmel"], c["model_out"], np.zeros_like(c["spec_in"]), R, in_place=False)
    assert np.array_equal(polar[..., 0], got) and (polar[..., 1] == 0).all(), "dn_server_mag is not the real part of dn_server_rows on a zero spectrum"
    one = abi.nan(R, plan.K)
    abi.lib.check(abi.lib.dn_server_mag(plan.handle, abi.ptr(lm), abi.ptr(mo), abi.ptr(one), 1, None))
    one = abi.down(one)
    assert np.isnan(one[1:]).all() and np.array_equal(one[0], got[0])


# ------------------------------------------------------------------ 8. the server chain with Griffin-Lim behind the model
CHAIN_N_ITER = 4
_GL_CHAINS = {}


def gl_chain_reference(geometry, name, hx_decay, fb):
    """Three requests: server_np64.process_chunk64's stages, then dsp_np64.griffinlim(lin, init = unit_phasor(spec)) in place of the istft.
    Asserts the conditioning rule on every request's Griffin-Lim."""
    key = (geometry, name, hx_decay)
    if key not in _GL_CHAINS:
        n_fft, _, n_mels = geometry
        hop, w, m64 = n_fft // 2, dc.window(name, n_fft), mc.hop_model64()
        hx = np.zeros((sc.CHAIN_B, 17, n_mels // 16))
        res = []
        for x in sc.chain_chunks(n_fft):
            r = server_np64.process_chunk64(x, hx, m64, n_fft, hop, w, fb, hx_decay)
            lin, u = r["lin"].transpose(0, 2, 1), server_np64.unit_phasor(r["spec"]).transpose(0, 2, 1)
            assert is_well_conditioned(lin, u, n_fft, name, CHAIN_N_ITER, MOMENTUM), (geometry, "the chain's Griffin-Lim is ill conditioned")
            out = dsp_np64.griffinlim(lin, n_fft, hop, u, n_iter=CHAIN_N_ITER, momentum=MOMENTUM, window=w)
            hx = r["hx"]
            res.append(dict(out=out, hx=r["hx"], out0=r["out"]))
        _GL_CHAINS[key] = res
    return _GL_CHAINS[key]


def check_gl_chain(check, geometry, name, hx_decay, fb, run):
    """run(chunk index, x, hx) -> (wave, hx as numpy, hx as the tier carries it)"""
    n_fft = geometry[0]
    hx = None
    for c, (x, ref) in enumerate(zip(sc.chain_chunks(n_fft), gl_chain_reference(geometry, name, hx_decay, fb))):
        wave, hx_np, hx = run(c, x, hx)
        rms, mx, scale = dc.wave_errors(wave, ref["out"])
        err = np.abs(wave - ref["out"])
        where = dict(n_fft=n_fft, window=name, chunk=c)
        check("glchain_rms", rms / scale, TOL_WAVE_RMS, lambda: hop_error_pattern(err, n_fft // 2), **where)
        check("glchain_max", mx / scale, TOL_WAVE_MAX, lambda: hop_error_pattern(err, n_fft // 2), **where)
        check("glchain_hx", float(np.abs(hx_np - ref["hx"]).max()), sc.TOL_HX_STREAM, **where)


def abi_gl_chain_runner(abi, plan, hx_decay, n_iter):
    """the ABI calls of one request as ServerDenoiser(n_iter=, phase="input") makes them"""
    lib, Cb = abi.lib, plan.n_mels // 16
    model = abi.model(mc.hop_blob(), Cb)

    def run(c, x, hx):
        B, L = x.shape
        T = 1 + L // plan.hop
        xd, hx0 = abi.up(x), abi.up(np.zeros((B, 17, Cb), np.float32)) if hx is None else hx
        spec, logmel, out, hx1 = abi.nan(B, T, plan.K, 2), abi.nan(B, T, plan.n_mels), abi.nan(B, T, plan.n_mels), abi.nan(B, 17, Cb)
        mag, wave, ws = abi.nan(B, T, plan.K), abi.nan(B, plan.hop * (T - 1)), workspace(abi, plan, B, T)
        lib.check(lib.dn_stft_general(plan.handle, abi.ptr(xd), abi.ptr(spec), abi.ptr(logmel), B, L, None))
        lib.check(lib.dn_cell_forward_ex(model, abi.ptr(logmel), abi.ptr(hx0), abi.ptr(out), abi.ptr(hx1), B, T, plan.n_mels, Cb, C.c_float(hx_decay), None))
        lib.check(lib.dn_server_mag(plan.handle, abi.ptr(logmel), abi.ptr(out), abi.ptr(mag), B * T, None))
        lib.check(lib.dn_griffinlim_general(plan.handle, abi.ptr(mag), abi.ptr(spec), 0, 0, abi.ptr(wave), abi.ptr(ws), B, T, n_iter, C.c_float(MOMENTUM),
                                            NORMALIZE, None))
        return abi.down(wave), abi.down(hx1), hx1

    return run, lambda: lib.dn_model_destroy(model)


# ------------------------------------------------------------------ 10. refusals
def check_refusals(abi, plans):
    """Every refusal returns its code with a message before anything is launched: the NaN-filled outputs stay NaN.  B = 0 returns DN_OK."""
    lib = abi.lib
    plan = plan_of(plans, 512, "hann")
    mel = plans.get(512, 16000, 64, "hann")
    B, T, K, hop = 2, 4, plan.K, plan.hop
    assert lib.dn_griffinlim_general_whole_max(plan.handle) == WHOLE_MAX and lib.dn_griffinlim_general_whole_max(None) == 0
    assert lib.dn_griffinlim_general_workspace_bytes(None, B, T) == 0 and lib.dn_griffinlim_general_workspace_bytes(plan.handle, B, 2) == 0
    assert lib.dn_griffinlim_general_workspace_bytes(plan.handle, B, 3) > 0 and lib.dn_griffinlim_general_workspace_bytes(plan.handle, 1, 1000) > 0
    mag, init = abi.up(np.ones((B, WHOLE_MAX + 1, K))), abi.up(np.ones((B, WHOLE_MAX + 1, K, 2)))
    wave, ws = abi.nan(B, hop * WHOLE_MAX), workspace(abi, plan, B, WHOLE_MAX + 1)
    ws_nan = abi.nan(*ws.shape)
    mag_out = abi.nan(B * T, K)
    lm = abi.up(np.zeros((B * T, 64)))
    p = abi.ptr

    def untouched():
        return all(np.isnan(abi.down(t)).all() for t in (wave, ws_nan, mag_out))

    def refused(rc, code, *words):
        msg = lib.dn_last_error().decode("utf-8", "replace")
        assert rc == code and msg and all(w in msg for w in words), (rc, msg, words)
        assert untouched(), msg

    def call(d=plan.handle, m=mag, ia=init, w=wave, s=ws_nan, b=B, t=T, n=2, mom=0.99, flags=0):
        return lib.dn_griffinlim_general(d, p(m), p(ia), 0, 0, p(w), p(s), b, t, n, C.c_float(mom), flags, None)

    refused(call(d=None), DN_ERR_INVALID, "dn_griffinlim_general", "null")
    refused(call(m=None), DN_ERR_INVALID, "dn_griffinlim_general", "null")
    refused(call(w=None), DN_ERR_INVALID, "dn_griffinlim_general", "null")
    refused(call(s=None), DN_ERR_INVALID, "dn_griffinlim_general", "null")
    refused(call(b=-1), DN_ERR_INVALID, "dn_griffinlim_general", "negative")
    refused(call(n=-1), DN_ERR_INVALID, "dn_griffinlim_general", "negative")
    refused(call(t=2), DN_ERR_INVALID, "dn_griffinlim_general", "3 columns")
    refused(call(mom=1.0), DN_ERR_INVALID, "momentum")
    refused(call(mom=-0.1), DN_ERR_INVALID, "momentum")
    refused(call(flags=1), DN_ERR_INVALID, "dn_griffinlim_general", "flag")
    refused(call(flags=8), DN_ERR_INVALID, "dn_griffinlim_general", "flag")
    refused(call(flags=WHOLE | STEPS), DN_ERR_INVALID, "DN_GLG_WHOLE", "DN_GLG_STEPS")
    refused(call(ia=None, flags=NORMALIZE), DN_ERR_INVALID, "DN_GL_INIT_NORMALIZE")
    refused(call(t=WHOLE_MAX + 1, flags=WHOLE), DN_ERR_UNSUPPORTED, "DN_GLG_WHOLE", str(WHOLE_MAX))
    refused(lib.dn_server_mag(plan.handle, p(lm), p(lm), p(mag_out), B * T, None), DN_ERR_INVALID, "without mel stages")
    refused(lib.dn_server_mag(mel.handle, p(lm), p(lm), None, B * T, None), DN_ERR_INVALID, "dn_server_mag", "null")
    refused(lib.dn_server_mag(mel.handle, p(lm), p(lm), p(mag_out), -1, None), DN_ERR_INVALID, "dn_server_mag", "negative")
    refused(lib.dn_griffinlim_draw_phases_general(plan.handle, 0, 0, None, B, T, None), DN_ERR_INVALID, "dn_griffinlim_draw_phases_general", "null")
    assert call(b=0) == DN_OK and lib.dn_server_mag(mel.handle, p(lm), p(lm), p(mag_out), 0, None) == DN_OK
    assert lib.dn_griffinlim_draw_phases_general(plan.handle, 0, 0, None, 0, T, None) == DN_OK
    assert untouched()
    # (and the same arguments do run: T = WHOLE_MAX + 1 without a force flag takes STEPS)
    lib.check(call(t=WHOLE_MAX + 1, s=ws))
    assert np.isfinite(abi.down(wave)).all()
