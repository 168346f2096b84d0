"""Shared cases of the synthetic-weight model tests (tests/test_oracle_model.py, tests/test_emu_model_synth.py,
tests/test_gpu_model_synth.py, tools/model_synth_margins.py): the weight blobs, the inputs, the float64 and fp32 CPU references and the
bf16 yardstick.  TEST INFRASTRUCTURE; nothing here touches a kernel.

Why other weights than the three trained checkpoints (every model test before these ran with them, against the reference's fp32 goldens
at 1e-4): oracle/synth_weights.py says what they cannot see -- dead channels, identical offset buffers in the three gates -- and the
shapes below are the ones no test launched: C = 1, 2, 3 (the stand-alone cell_kernel<0,0>), T = 2 and 4 (kCellChunk = 3: a short
chunk, a full chunk, chunk + 1, two chunks + 1), every MOMO3 padding triple, both values of every decoder level's output_padding.

Inputs: B = 6 streams, x signed and scaled to +-6 (the goldens' x is a log1p, always positive), hx0 random except for one case.

Live-channel condition (on the INPUT, not on any kernel; tests/test_oracle_model.py asserts it for every case): in the float64 oracle
run every channel of d0..d3 (d0..d2 for MOMO3) and gate_h is nonzero at some stream, position or step, so that every weight row,
every tap and every tile row reaches the compared outputs.

The reference is always float64 (oracle/model_ref.forward, oracle/momo_ref.forward on float64 tensors of the fp32 weight values); the
tolerance of a case is R x e_ref, e_ref = max-abs error of the same oracle run in fp32 on the CPU (reference_error).
"""
import itertools

import numpy as np
import torch

from oracle import model_ref, momo_ref, synth_weights

B = 6
X_SCALE = 6.0
CAP = 1e-5          # R x e_ref of the fp32 families must stay under this on every case: ten times under the project's 1e-4 bar


# ------------------------------------------------------------------ GRUUNet2
class GruCase:
    def __init__(self, C, T, seed, hx_zero=False):
        self.C, self.T, self.F, self.seed, self.hx_zero = C, T, 16 * C, seed, hx_zero
        self.id = f"C{C}-T{T}-{synth_weights.offset_kind(seed)}" + ("-hx0" if hx_zero else "")

    def blob(self):
        return synth_weights.gruunet2_blob(self.seed)

    def inputs(self):
        """x (B, T, F), hx0 (B, 17, C) fp32"""
        rng = np.random.default_rng(1000 + self.seed)
        x = rng.uniform(-X_SCALE, X_SCALE, (B, self.T, self.F)).astype(np.float32)
        hx = (0.5 * rng.standard_normal((B, 17, self.C))).astype(np.float32)
        return x, np.zeros_like(hx) if self.hx_zero else hx


# C in 1..5 x T in {1, 2, 3, 4, 7}: cell_kernel<0,0> (C <= 3), <4,0> / <4,3>, <5,0> / <5,3> (the T = 3 instantiations).  The seed decides
# the offset kind (seed % 3: shifted, uneven, spacing != 0.2), so every C and every T meets all three.  hx0 = 0 once, at T = 4.
# GRU_SEED_K / MOMO_SEED_K: per case, the first k = 0, 1, 2 ... for which seed + 3 k (the same offset kind) leaves no channel dead in the
# float64 oracle run -- computed from the reference alone, not from any kernel's output; test_oracle_model.py asserts the condition.
GRU_SEED_K = [6, 2, 6, 2, 1, 3, 1, 0, 2, 0, 2, 1, 0, 1, 0, 0, 0, 1, 0, 1, 0, 3, 0, 0, 2]
MOMO_SEED_K = [7, 1, 9, 2, 4, 0, 1, 0, 27, 0, 0, 0, 4, 0, 2, 9, 4, 0, 0, 0, 23, 0, 0, 3, 0]
GRU_CASES = [GruCase(C, T, 100 + 5 * C + i + 3 * GRU_SEED_K[5 * (C - 1) + i], hx_zero=(C, T) == (3, 4))
             for C in (1, 2, 3, 4, 5) for i, T in enumerate((1, 2, 3, 4, 7))]
GRU_IDS = [c.id for c in GRU_CASES]
# The bf16 cases (C = 4, 5 x T = 3, 7) have seeds of their own: besides the live-channel condition, the fp32 and the float64 run of the bf16
# yardstick must agree to BF16_NO_FLIP.  Rounding to bf16 is discontinuous: where an operand sits on a rounding boundary the two runs round it
# to different neighbours and end 3e-5 .. 4e-4 apart, and e_ref would measure that flip instead of the arithmetic (it did at the fp32 cases'
# own seeds of C4-T3 and C5-T7: 4.5e-4 and 9.1e-5 against 5e-7 .. 8e-7 elsewhere, a bound of 0.05 .. 0.2 after R).  BF16_SEED_K: the first k whose
# seed + 3 k meets both conditions, from the reference alone (first_seed_k; test_oracle_model.py derives all three lists again).
BF16_NO_FLIP = 2e-6
BF16_SEED_K = [2, 1, 0, 4]
GRU_BF16_CASES = [GruCase(C, T, 100 + 5 * C + i + 3 * BF16_SEED_K[2 * (C - 4) + j]) for C in (4, 5) for j, (i, T) in enumerate(((2, 3), (4, 7)))]
for _c in GRU_BF16_CASES:
    _c.id += "-bf16"
GRU_EX_CASE = next(c for c in GRU_CASES if (c.C, c.T) == (4, 3))       # dn_cell_forward_ex, hx_scale 0.9
HX_SCALE = 0.9


def bf16_round(t):
    """round to nearest even to bf16, as dn_model_create packs the bf16 fragments and the kernel rounds the activations"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


_CACHE = {}


def _sd(blob, dtype):
    return {k: v.to(dtype) for k, v in model_ref.unflatten_weights(blob).items()}


def gru_reference(case, dtype=torch.float64, bf16=False, hx_scale=1.0):
    """-> dict(out, hx, steps): oracle/model_ref.forward in `dtype` on the case (cached, read-only).  bf16: the yardstick of
    dn_cell_forward_bf16 (model_ref.cell_step's mfma_round).  hx_scale: dn_cell_forward_ex multiplies the hx it
    returns by it (server.py:214; once per call, the steps inside hand on the unscaled state)."""
    key = ("gru", case.id, dtype, bf16, hx_scale)
    if key not in _CACHE:
        sd = _sd(case.blob(), dtype)
        x, hx = (torch.from_numpy(a).to(dtype) for a in case.inputs())
        steps, outs = [], []
        with torch.no_grad():
            for t in range(case.T):
                inter = {}
                o, hx = model_ref.cell_step(sd, x[:, t], hx, inter, mfma_round=bf16_round if bf16 else None)
                steps.append({k: v.numpy() for k, v in inter.items()})
                outs.append(o)
        r = dict(out=torch.stack(outs, 1).numpy(), hx=(hx * hx_scale).numpy(), steps=steps)
        for a in (r["out"], r["hx"]):
            a.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def bf16_yardstick_gap(case):
    """max-abs distance between the bf16 yardstick and the unrounded forward, both float64: what the bf16 tiles cost, 5e-3 .. 1e-2 here"""
    y = gru_reference(case, bf16=True)
    return errors(y["out"], y["hx"], gru_reference(case))


def gru_case_is_usable(case, bf16=False):
    """the conditions on a case's seed, from the float64 / fp32 oracle runs alone: every channel live; for a bf16 case also no rounding flip
    between the fp32 and the float64 run of the yardstick"""
    if dead_channels(gru_reference(case)["steps"], ("d0", "d1", "d2", "d3", "gate_h")):
        return False
    return not bf16 or reference_error(gru_reference(case, torch.float32, bf16=True), gru_reference(case, bf16=True)) <= BF16_NO_FLIP


def first_seed_k(make_case, usable, k_max=64):
    """the first k = 0, 1, 2 ... whose case make_case(k) is usable (candidate cases get ids of their own, so that the cache keeps them apart)"""
    for k in range(k_max):
        c = make_case(k)
        c.id += f"-candidate{k}"
        if usable(c):
            return k
    raise AssertionError("no usable seed")


def derive_seed_tables():
    """-> (GRU_SEED_K, BF16_SEED_K, MOMO_SEED_K) computed again from the oracles (tools/model_synth_margins.py --seeds prints them)"""
    gru = [first_seed_k(lambda k: GruCase(C, T, 100 + 5 * C + i + 3 * k, hx_zero=(C, T) == (3, 4)), gru_case_is_usable)
           for C in (1, 2, 3, 4, 5) for i, T in enumerate((1, 2, 3, 4, 7))]
    bf16 = [first_seed_k(lambda k: GruCase(C, T, 100 + 5 * C + i + 3 * k), lambda c: gru_case_is_usable(c, bf16=True))
            for C in (4, 5) for i, T in ((2, 3), (4, 7))]
    momo = [first_seed_k(lambda k: MomoCase(c.pads, c.F, c.T, c.with_prev, 300 + n + 3 * k),
                         lambda m: not dead_channels(momo_reference(m)["steps"], ("d0", "d1", "d2", "gate_h"))) for n, c in enumerate(MOMO_CASES)]
    return gru, bf16, momo


def reference_error(ref32, ref64):
    """e_ref: max-abs error of the fp32 CPU oracle against float64 over out and hx"""
    return max(float(np.abs(ref32["out"].astype(np.float64) - ref64["out"]).max()), float(np.abs(ref32["hx"].astype(np.float64) - ref64["hx"]).max()))


def errors(out, hx, ref64):
    return max(float(np.abs(np.asarray(out, np.float64) - ref64["out"]).max()), float(np.abs(np.asarray(hx, np.float64) - ref64["hx"]).max()))


def dead_channels(steps, names):
    """{name: indices of the channels that are zero at every stream, position and step}"""
    dead = {}
    for n in names:
        alive = np.zeros(steps[0][n].shape[1], bool)
        for s in steps:
            alive |= (s[n] != 0).any(axis=(0, 2))
        if not alive.all():
            dead[n] = np.flatnonzero(~alive).tolist()
    return dead


# ------------------------------------------------------------------ MOMO3
MOMO_MIN_F, MOMO_MAX_F = 3, 64                       # what dn_momo_forward accepts (kMomoMaxF)
PADDING_TRIPLES = list(itertools.product((0, 1), repeat=3))


def momo_lengths(F, pads):
    """(L1, L2, C) or None when a level runs out of samples"""
    Ls, L = [], F
    for p in pads:
        if L + 2 * p < 3:
            return None
        L = (L + 2 * p - 3) // 2 + 1
        Ls.append(L)
    return tuple(Ls)


def momo_output_paddings(F, pads):
    """output_padding of the three decoder levels in execution order (momo3.py:185-187: output_size = length of the skip)"""
    L1, L2, C = momo_lengths(F, pads)
    return (L2 - ((C - 1) * 2 - 2 * pads[2] + 3), L1 - ((L2 - 1) * 2 - 2 * pads[1] + 3), F - ((L1 - 1) * 2 - 2 * pads[0] + 3))


def momo_bins(pads):
    """The F values of one padding triple: the smallest accepted, 64, and the fewest further ones (smallest first) after which every
    decoder level has run with output_padding 0 and with 1."""
    ok = [F for F in range(MOMO_MIN_F, MOMO_MAX_F + 1) if momo_lengths(F, pads) is not None]
    chosen = [ok[0], MOMO_MAX_F]
    seen = {(l, op) for F in chosen for l, op in enumerate(momo_output_paddings(F, pads))}
    for F in ok:
        new = {(l, op) for l, op in enumerate(momo_output_paddings(F, pads))} - seen
        if new:
            chosen.append(F)
            seen |= new
    assert seen == {(l, op) for l in range(3) for op in (0, 1)}, (pads, seen)
    return sorted(set(chosen))


class MomoCase:
    def __init__(self, pads, F, T, with_prev, seed):
        self.pads, self.F, self.T, self.with_prev, self.seed = pads, F, T, with_prev, seed
        self.C = momo_lengths(F, pads)[2]
        self.id = f"p{''.join(map(str, pads))}-F{F}-T{T}-{'prev' if with_prev else 'noprev'}"

    def blob(self):
        return synth_weights.momo3_blob(self.seed)

    def inputs(self):
        """x (B, T, F), hx0 (B, 16, C), prev (B, 1, F) or None"""
        rng = np.random.default_rng(2000 + self.seed)
        x = rng.uniform(-X_SCALE, X_SCALE, (B, self.T, self.F)).astype(np.float32)
        hx = (0.5 * rng.standard_normal((B, 16, self.C))).astype(np.float32)
        prev = rng.uniform(-X_SCALE, X_SCALE, (B, 1, self.F)).astype(np.float32)
        return x, hx, prev if self.with_prev else None


def _momo_cases():
    """every padding triple x its F values; (T, prev) walks through (1, given), (4, None), (4, given), (1, None) so that every triple meets
    both T and both conventions"""
    combos = [(1, True), (4, False), (4, True), (1, False)]
    cases, n = [], 0
    for pads in PADDING_TRIPLES:
        for F in momo_bins(pads):
            T, with_prev = combos[n % 4]
            cases.append(MomoCase(pads, F, T, with_prev, 300 + n + 3 * MOMO_SEED_K[n]))
            n += 1
    return cases


MOMO_CASES = _momo_cases()
MOMO_IDS = [c.id for c in MOMO_CASES]


def momo_reference(case, dtype=torch.float64):
    key = ("momo", case.id, dtype)
    if key not in _CACHE:
        sd = {k: v.to(dtype) for k, v in momo_ref.unflatten_weights(case.blob()).items()}
        x, hx, prev = case.inputs()
        steps = []
        with torch.no_grad():
            out, h = momo_ref.forward(sd, torch.from_numpy(x).to(dtype), torch.from_numpy(hx).to(dtype),
                                      None if prev is None else torch.from_numpy(prev).to(dtype), paddings=case.pads, intermediates=steps)
        r = dict(out=out.numpy(), hx=h.numpy(), steps=[{k: v.numpy() for k, v in s.items()} for s in steps])
        for a in (r["out"], r["hx"]):
            a.setflags(write=False)
        _CACHE[key] = r
    return _CACHE[key]


def momo_refusals():
    """(pads, F) that dn_momo_forward's shape rules accept (3 <= F <= 64, every level keeps a sample) but whose transposed convs cannot
    reach the skip lengths with an output_padding of 0 or 1, which the reference refuses: none.  A stride-2, kernel-3 level maps L to
    Lo = (L + 2 p - 3) // 2 + 1 and its transpose maps Lo back to 2 Lo + 1 - 2 p, which is L or L - 1.  This restates the rules in Python;
    tests/test_emu_model_synth.py pins the library's own answer one bin under the smallest accepted F."""
    bad = []
    for pads in PADDING_TRIPLES:
        for F in range(MOMO_MIN_F, MOMO_MAX_F + 1):
            if momo_lengths(F, pads) is not None and any(op not in (0, 1) for op in momo_output_paddings(F, pads)):
                bad.append((pads, F))
    return bad


# ------------------------------------------------------------------ cell_body inside the hop kernels: synthetic weights, offsets of spacing 0.2
# with a different shift per gate (hop_blob)
HOP_SEED = 401
HOP_B = 3


def hop_blob():
    return synth_weights.gruunet2_blob(HOP_SEED, offsets="shifted")


def hop_model64():
    """GRUUNet2 forward in float64 on the hop blob, as pipeline_np64.process_frame64 wants it"""
    sd = _sd(hop_blob(), torch.float64)

    def run(x, hx):
        with torch.no_grad():
            o, h = model_ref.forward(sd, torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(hx, np.float64)))
        return o.numpy(), h.numpy()
    return run


# ------------------------------------------------------------------ the checks, shared by the emulation and the gpu tier
# The backends that run the kernels are in tests/model_abi.py.
#
# Tolerance: R x e_ref per family and tier.  The rule (guard_factor): 10 x the worst ratio error / e_ref measured over the family's cases in
# one run of tools/model_synth_margins.py on that tier, rounded up to a power of two.  For the fp32 families R x e_ref must also stay <= CAP
# on every case.  Where the two collide the CAP wins and R is the largest power of two that keeps it (capped_factor): the fp32 oracle's own
# error reaches 0.9e-6 (GRUUNet2) and 1.0e-6 (MOMO3) on these cases, so ten times a ratio of 1.3 .. 2 no longer fits under 1e-5 although
# the kernels are as close to float64 as the oracle is; the bound is then TIGHTER than the rule's, with 4 .. 6 x left over the measured
# worst (the kernels are deterministic).  profiles/model_synth_margins.txt holds every ratio and absolute error behind the constants.
# The bf16 family is not held to the cap: the kernel can sit one bf16 rounding flip away from its yardstick (3e-5 on one of the four cases,
# the other three are within e_ref).  Its cases are chosen so that e_ref itself holds no flip (BF16_NO_FLIP), which keeps R x e_ref at a few
# 1e-4, and check_gru_bf16 asserts that the bound stays under a quarter of what the bf16 tiles cost (bf16_yardstick_gap, 5e-3 .. 1e-2): a
# forward that ran fp32 tiles, truncated instead of rounding, or left an operand unrounded is outside it.
def guard_factor(worst_ratio):
    return 2 ** int(np.ceil(np.log2(10.0 * worst_ratio)))


def capped_factor(worst_ratio, worst_e_ref):
    return min(guard_factor(worst_ratio), 2 ** int(np.floor(np.log2(CAP / worst_e_ref))))


R = {
    # worst measured ratio -> rule -> cap:  gru 1.34 -> 16 -> 8;  gru_ex 0.41 -> 8;  bf16 39.1 -> 512 (bounds 2.8e-4 .. 7.7e-4);  hop 1.39 -> 16;  momo 1.97 -> 32 -> 8
    "emu": dict(gru=8, gru_ex=8, bf16=512, hop=16, momo=8),
    # (one MI355X run)                      gru 1.27 -> 16 -> 8;  gru_ex 0.40 -> 4;  bf16 39.1 -> 512;  hop 1.79 -> 32 -> 16;  momo 1.97 -> 32 -> 8
    "gpu": dict(gru=8, gru_ex=4, bf16=512, hop=16, momo=8),
}


def check(err, e_ref, family, tier, what, capped=True, report=None):
    """assert err <= R x e_ref (and R x e_ref <= CAP); `report` (a list) collects (what, err, e_ref) instead of asserting"""
    if report is not None:
        report.append((family, what, err, e_ref))
        return
    bound = R[tier][family] * e_ref
    print(f"{family} {what}: error {err:.3e}, e_ref {e_ref:.3e}, ratio {err / e_ref:.2f}, bound {bound:.3e}")
    if capped:
        assert bound <= CAP, (f"{what}: R x e_ref = {bound:.2e} exceeds the cap {CAP:.0e}.  e_ref is the fp32 CPU oracle's own error on THIS host "
                              f"({e_ref:.3e}; 1.03e-6 at most on the hosts of profiles/model_synth_margins.txt): another torch build or thread "
                              f"count moves it, so look at e_ref first; the kernel's error is {err:.3e}")
    assert err <= bound, f"{what}: error {err:.3e} > {R[tier][family]} x e_ref {e_ref:.3e}"


def check_gru(backend, case, tier, modes=("fp32",), report=None):
    """(a): dn_cell_forward (and GRUUNet2.forward) against float64 on out and hx"""
    ref64 = gru_reference(case)
    e_ref = reference_error(gru_reference(case, torch.float32), ref64)
    x, hx0 = case.inputs()
    for mode in modes:
        out, hx = backend.cell(case.blob(), case.C, x, hx0, mode)
        assert out.shape == ref64["out"].shape and hx.shape == ref64["hx"].shape
        check(errors(out, hx, ref64), e_ref, "gru", tier, f"{case.id} {mode}", report=report)


def check_gru_ex(backend, tier, report=None):
    """(b): dn_cell_forward_ex with hx_scale 0.9 against float64 times 0.9"""
    case = GRU_EX_CASE
    ref64 = gru_reference(case, hx_scale=HX_SCALE)
    assert np.array_equal(ref64["out"], gru_reference(case)["out"]) and np.allclose(ref64["hx"], HX_SCALE * gru_reference(case)["hx"], rtol=0, atol=1e-15)
    e_ref = reference_error(gru_reference(case, torch.float32, hx_scale=HX_SCALE), ref64)
    x, hx0 = case.inputs()
    out, hx = backend.cell(case.blob(), case.C, x, hx0, ("ex", HX_SCALE))
    check(errors(out, hx, ref64), e_ref, "gru_ex", tier, f"{case.id} hx_scale {HX_SCALE}", report=report)


def check_gru_bf16(backend, case, tier, modes=("bf16",), report=None):
    """(c): dn_cell_forward_bf16 against the float64 forward whose MFMA convs see bf16-rounded inputs and weights"""
    ref64 = gru_reference(case, bf16=True)
    e_ref = reference_error(gru_reference(case, torch.float32, bf16=True), ref64)
    gap = bf16_yardstick_gap(case)
    assert e_ref <= BF16_NO_FLIP, f"{case.id}: the fp32 and float64 runs of the yardstick are {e_ref:.2e} apart (a rounding flip): pick another seed"
    if report is None:
        # the bound tells the bf16 forward from the unrounded one with room to spare
        assert R[tier]["bf16"] * e_ref <= 0.25 * gap, f"{case.id}: bound {R[tier]['bf16'] * e_ref:.2e} against a bf16-to-fp32 gap of {gap:.2e}"
    x, hx0 = case.inputs()
    for mode in modes:
        out, hx = backend.cell(case.blob(), case.C, x, hx0, mode)
        check(errors(out, hx, ref64), e_ref, "bf16", tier, f"{case.id} {mode} (bf16-to-fp32 gap {gap:.2e})", capped=False, report=report)


def check_momo(backend, case, tier, vias=("abi",), report=None):
    """(e): dn_momo_forward (and MOMO3.forward) against float64 momo_ref.forward(paddings=...); prev_out is the last frame, bit for bit"""
    ref64 = momo_reference(case)
    e_ref = reference_error(momo_reference(case, torch.float32), ref64)
    x, hx0, prev = case.inputs()
    for via in vias:
        out, hx, last = backend.momo(case.blob(), case.pads, x, hx0, prev, via)
        assert out.shape == ref64["out"].shape and hx.shape == ref64["hx"].shape
        if last is not None:
            assert np.array_equal(last, x[:, -1, :]), f"{case.id}: prev_out is not the last frame"
        check(errors(out, hx, ref64), e_ref, "momo", tier, f"{case.id} {via}", report=report)


# (d) cell_body inside the other kernels.  Only the mel residual and hx are compared, never the waveform, so the Griffin-Lim chains run one
# iteration.  Frames are white noise (the hop normalises by the frame's peak), hx0 random for the single hops.
HOP_N_ITER = 1
HOP_GEOMETRIES = [(n_fft, n_mels) for n_fft in (512, 1024, 1536) for n_mels in (80, 32)]
HOP_SAMPLE_RATE = {512: 16000, 1024: 16000, 1536: 48000}
CHAIN_HOPS, CHAIN_GROUP = 4, 3
CHAIN_PATHS = ("group", "split", "sessions", "clip",
               "sessions_two_launches")          # (the pool's other schedule: its front kernel picks its own (bf16, C) instantiation)


def hop_params(n_fft, n_mels):
    from oracle import pipeline_ref
    return pipeline_ref.Params(HOP_SAMPLE_RATE[n_fft], n_fft, n_fft // 2, n_mels)


CHAIN_P = hop_params(1024, 80)          # the geometry the group pipe, the split hop, the session schedules and clip mode share


def hop_fbank(p):
    from oracle import dsp_ref
    return dsp_ref.melscale_fbanks(p.n_stft, p.n_mels, p.sample_rate).numpy()


def hop_window(n_fft):
    return torch.hann_window(n_fft).numpy()


def hop_inputs(p, n_samples, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((HOP_B, n_samples)).astype(np.float32), (0.5 * rng.standard_normal((HOP_B, 17, p.num_compressed_bins))).astype(np.float32)


def _hop_model_stage(p, frames, hx, dtype):
    """analysis (P1-P6) + model (P7) of one hop in `dtype` -> (mel residual, hx)"""
    from oracle import pipeline_np64, pipeline_ref
    if dtype == torch.float64:
        r = pipeline_np64.process_frame64(frames, np.asarray(hx, np.float64), hop_model64(), hop_window(p.n_fft), hop_fbank(p),
                                          np.ones((frames.shape[0], p.n_stft, 3), np.complex64), p.n_fft, p.hop, n_iter=0)
        return r["predicted_diff"], r["hx"]
    with torch.no_grad():
        mel, _ = pipeline_ref.analysis(torch.from_numpy(frames), p, torch.from_numpy(hop_fbank(p)))
        diff, h = model_ref.forward(_sd(hop_blob(), torch.float32), mel, torch.from_numpy(np.asarray(hx, np.float32)))
    return diff.numpy(), h.numpy()


def hop_reference(n_fft, n_mels, dtype=torch.float64):
    """-> dict(out = mel residual, hx) of one dn_process_frame hop (cached)"""
    key = ("hop", n_fft, n_mels, dtype)
    if key not in _CACHE:
        p = hop_params(n_fft, n_mels)
        frames, hx0 = hop_inputs(p, n_fft, 500 + n_fft + n_mels)
        out, hx = _hop_model_stage(p, frames, hx0, dtype)
        _CACHE[key] = dict(out=out, hx=hx)
    return _CACHE[key]


def chain_signal():
    return hop_inputs(CHAIN_P, CHAIN_P.n_fft + (CHAIN_HOPS - 1) * CHAIN_P.hop, 700)[0]


def chain_reference(dtype=torch.float64):
    """-> dict(out, hx): hx after CHAIN_HOPS chained hops from zero (out = the last hop's mel residual, which no chained path returns)"""
    key = ("chain", dtype)
    if key not in _CACHE:
        p, sig = CHAIN_P, chain_signal()
        hx = np.zeros((HOP_B, 17, p.num_compressed_bins), np.float64 if dtype == torch.float64 else np.float32)
        for h in range(CHAIN_HOPS):
            out, hx = _hop_model_stage(p, np.ascontiguousarray(sig[:, h * p.hop:h * p.hop + p.n_fft]), hx, dtype)
        _CACHE[key] = dict(out=out, hx=hx)
    return _CACHE[key]


def check_hop(backend, n_fft, n_mels, tier, report=None):
    """(d): dn_process_frame's mel residual and hx against pipeline_np64.process_frame64 with the synthetic blob"""
    p = hop_params(n_fft, n_mels)
    ref64 = hop_reference(n_fft, n_mels)
    e_ref = reference_error(hop_reference(n_fft, n_mels, torch.float32), ref64)
    frames, hx0 = hop_inputs(p, n_fft, 500 + n_fft + n_mels)
    resid, hx = backend.process_frame(p, frames, hx0)
    check(errors(resid, hx, ref64), e_ref, "hop", tier, f"process_frame n_fft {n_fft} n_mels {n_mels}", report=report)


def check_chain(backend, path, tier, report=None):
    """(d): hx after four chained hops through a group pipe, the split hop, a session pool or clip mode against the float64 chain"""
    ref64, ref32 = chain_reference(), chain_reference(torch.float32)
    e_ref = float(np.abs(ref32["hx"].astype(np.float64) - ref64["hx"]).max())
    hx = backend.chain(path, chain_signal())
    assert hx.shape == ref64["hx"].shape
    check(float(np.abs(hx.astype(np.float64) - ref64["hx"]).max()), e_ref, "hop", tier, f"chain of {CHAIN_HOPS} hops, {path}", report=report)
