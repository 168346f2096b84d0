"""Shared by the resampler tests: a float64 restatement of torchaudio.transforms.Resample (2.6.0: _get_sinc_resample_kernel /
_apply_sinc_resample_kernel, restated from the published source; parity with torchaudio itself is unpinned), the streaming model
of dn_resample_push, and the case table.

    g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base), KW = 2 width + o
    k[p][j] = sinc(pi t) window(t) base / o,  t = (-p / n + (j - width) / o) base clamped to +-lpw
    y[q n + p] = sum_j k[p][j] xz[q o + j - width],  ceil(n L / o) samples

Everything here is numpy on the CPU; nothing is taken from the code under test."""
import math

import numpy as np

# the first six pairs of the issue's table: the case table of the parity tests
PAIRS = ((48000, 16000), (16000, 48000), (8000, 16000), (44100, 48000), (48000, 44100), (44100, 16000))
SMALL_PAIRS = PAIRS[:3]
# pairs that run the kernel variants PAIRS does not: even o (the skewed LDS tile: o = 2, 4, 8), four accumulators a lane (3 : 4), and a general
# ratio with more than one phase tile a block (n = 640 > 256).  Their table rows stay within ROW_L1_MAX too (test_oracle_resample.py).
VARIANT_PAIRS = ((16000, 8000), (48000, 12000), (32000, 4000), (12000, 16000), (11025, 16000))
B = 3
KAISER_BETA = 14.769656459379492
ROW_L1_MAX = 1.87          # the largest L1 norm of a table row over PAIRS (checked in test_oracle_resample.py)


class Geometry:
    def __init__(self, orig, new, lpw=6, rolloff=0.99):
        g = math.gcd(orig, new)
        self.orig, self.new, self.lpw, self.rolloff = orig, new, lpw, rolloff
        self.o, self.n = orig // g, new // g
        self.base = min(self.o, self.n) * rolloff
        self.width = math.ceil(lpw * self.o / self.base)
        self.KW = 2 * self.width + self.o
        self.D = -(-self.width // self.o)
        self.H = self.D * self.o + self.width

    def out_len(self, L):
        return -(-self.n * L // self.o)


def table64(geo, method="sinc_interp_hann", beta=None):
    """k[p][j] in float64"""
    p = np.arange(geo.n, dtype=np.float64)[:, None]
    j = np.arange(geo.KW, dtype=np.float64)[None, :]
    t = (-p / geo.n + (j - geo.width) / geo.o) * geo.base
    t = np.clip(t, -float(geo.lpw), float(geo.lpw))
    if method == "sinc_interp_hann":
        c = np.cos(t * math.pi / geo.lpw / 2)
        window = c * c
    else:
        beta = KAISER_BETA if beta is None else beta
        window = np.i0(beta * np.sqrt(1.0 - (t / geo.lpw) ** 2)) / np.i0(beta)
    t = t * math.pi
    scale = geo.base / geo.o
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(t) / t)
    return sinc * (window * scale)


def table32(geo, method="sinc_interp_hann", beta=None):
    """the table as the library holds it: rounded once to float32"""
    return table64(geo, method, beta).astype(np.float32)


def _windows(geo, x, lead):
    """rows [.., blocks, KW] of the virtual input: `lead` zeros, x, zeros"""
    L = x.shape[-1]
    blocks = -(-geo.out_len(L) // geo.n)
    xz = np.zeros(x.shape[:-1] + (lead + max(L, (blocks - 1) * geo.o + geo.KW),), dtype=x.dtype)
    xz[..., lead:lead + L] = x
    idx = np.arange(blocks)[:, None] * geo.o + np.arange(geo.KW)[None, :]
    return xz[..., idx], blocks


def resample64(geo, x, table):
    """(.., L) -> (.., ceil(n L / o)) in float64 with the float32-rounded `table` [n][KW] (so what differs from the kernels is the fp32 chain alone)"""
    x = np.asarray(x, dtype=np.float64)
    w, blocks = _windows(geo, x, geo.width)
    y = np.einsum("...bj,pj->...bp", w, np.asarray(table, dtype=np.float64))
    return y.reshape(x.shape[:-1] + (blocks * geo.n,))[..., :geo.out_len(x.shape[-1])]


def resample32(geo, x, table):
    """the same ascending sum evaluated in float32 on the CPU: acc = fl(acc + fl(k x)) over j ascending (an fp32 chain of KW terms, without the
    fused multiply-add the device has) -- the reference error e_ref of the tolerance"""
    x = np.asarray(x, dtype=np.float32)
    w, blocks = _windows(geo, x, geo.width)
    k = np.asarray(table, dtype=np.float32)
    acc = np.zeros(x.shape[:-1] + (blocks, geo.n), dtype=np.float32)
    for j in range(geo.KW):
        acc = acc + w[..., :, j, None] * k[None, :, j]
    return acc.reshape(x.shape[:-1] + (blocks * geo.n,))[..., :geo.out_len(x.shape[-1])]


def stream_model(geo, x, table, pushes):
    """dn_resample_push restated: the state is the last H samples, block b of a push reads [history | chunk][b o : b o + KW).  `pushes`: blocks per
    push; x (.., sum(pushes) o).  Returns the concatenated outputs (.., sum(pushes) n), float64."""
    x = np.asarray(x, dtype=np.float64)
    k = np.asarray(table, dtype=np.float64)
    hist = np.zeros(x.shape[:-1] + (geo.H,))
    out, at = [], 0
    for blocks in pushes:
        chunk = x[..., at:at + blocks * geo.o]
        at += blocks * geo.o
        c = np.concatenate([hist, chunk], axis=-1)
        idx = np.arange(blocks)[:, None] * geo.o + np.arange(geo.KW)[None, :]
        out.append(np.einsum("...bj,pj->...bp", c[..., idx], k).reshape(x.shape[:-1] + (blocks * geo.n,)))
        hist = c[..., c.shape[-1] - geo.H:]
    return np.concatenate(out, axis=-1)


def lengths(geo):
    """the L of the case table: {1, o - 1 when >= 1, o, width, KW - 1, KW, 2 KW + o + 1, 1009}"""
    ls = [1, geo.o - 1, geo.o, geo.width, geo.KW - 1, geo.KW, 2 * geo.KW + geo.o + 1, 1009]
    return sorted({v for v in ls if v >= 1})


def inputs(geo, L, seed):
    """name -> (B, L) float64: uniform +-1 noise (wideband: every tap matters), a unit impulse at sample 0, one at sample L - 1"""
    rng = np.random.default_rng(seed)
    first, last = np.zeros((B, L)), np.zeros((B, L))
    first[:, 0] = 1.0
    last[:, L - 1] = 1.0
    return {"noise": rng.uniform(-1.0, 1.0, (B, L)), "impulse_first": first, "impulse_last": last}


def seed_of(orig, new, L):
    return (orig * 31 + new * 17 + L) % (2 ** 31)


def to_s16(x):
    """float64 in [-1, 1] -> int16 the way the kernels write it: clip, * 32767, truncate"""
    return np.trunc(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)


def to_s16_f32(x32):
    """float32 values -> int16 with the store's own arithmetic: the clip and the product in float32, then the truncation"""
    x32 = np.asarray(x32, dtype=np.float32)
    return np.trunc(np.clip(x32, np.float32(-1.0), np.float32(1.0)) * np.float32(32767.0)).astype(np.int16)


# ---- tolerance against float64.  The bound of a case is R x e_ref, e_ref the error of resample32 (an fp32 CPU evaluation of the same ascending sum,
# never the code under test) on that case; R from the ratios measured on the MI355X with ten times the measured margin
# (profiles/resample_parity_margins.txt).  Independently no case may exceed the worst case of an fp32 chain of KW terms on rows of L1 norm <= 1.87.
R = 26.0          # measured: the largest err / e_ref over the case table is 2.55 (8000 -> 16000, L = 7), 1.35 from L = 41 on


def hard_bound(geo):
    return geo.KW * 2.0 ** -24 * ROW_L1_MAX


def bound(geo, e_ref):
    return min(R * e_ref, hard_bound(geo))


def s16_input(x16):
    """int16 samples -> (the float64 values they stand for, the float32 values the kernels form at the load: a true division in float32)"""
    return x16.astype(np.float64) / 32767.0, x16.astype(np.float32) / np.float32(32767.0)


def s16_differences(got16, want64, fbound):
    """How many int16 outputs differ from the float64 path's truncation.  A difference must be one count, at a sample whose float64 value times
    32767 lies within the float bound (plus the rounding of that product in float32) of an integer; anything else raises."""
    scaled = np.clip(want64, -1.0, 1.0) * 32767.0
    diff = got16.astype(np.int64) - np.trunc(scaled).astype(np.int64)
    bad = diff != 0
    near = np.abs(scaled - np.round(scaled)) <= fbound * 32767.0 + 32767.0 * 2.0 ** -24
    assert (np.abs(diff[bad]) == 1).all() and near[bad].all(), (diff[bad], scaled[bad])
    return int(bad.sum())


_S16_SEEDS = {}


def s16_case(orig, new, L, rows=B):
    """(x int16 (rows, L), the seed): half-scale noise from the first seed from seed_of on for which the fp32 CPU evaluation alone differs from the
    float64 truncation in under 1 % of the samples (test_oracle_resample.py checks exactly that)"""
    key = (orig, new, L, rows)
    if key not in _S16_SEEDS:
        geo = Geometry(orig, new)
        k = table32(geo)
        seed = seed_of(orig, new, L)
        while True:
            x16 = to_s16(0.5 * np.random.default_rng(seed).uniform(-1.0, 1.0, (rows, L)))
            x64, x32 = s16_input(x16)
            want = resample64(geo, x64, k)
            cpu = resample32(geo, x32, k)
            if (to_s16_f32(cpu) != to_s16(want)).sum() < 0.01 * want.size:
                break
            seed += 1
        _S16_SEEDS[key] = (x16, seed)
    return _S16_SEEDS[key]
