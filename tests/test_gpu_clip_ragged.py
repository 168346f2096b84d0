"""The ragged clip call on the MI355X (``pytest -m gpu``): ``dn_clip_process_ragged`` behind ``Denoiser.clip_ragged`` and
``Denoiser.denoise_clips``.  For every stream with hops the call is "n_hops[b] calls of ``dn_stream_step`` with B = 1, bit for bit": the yardstick
is ``DenoiserStream.push`` (the unchanged ``dn_stream_step``) on a stream of its own with ``stream_id0 + b``, run once per stream and variant, and
every comparison is ``torch.equal`` / ``np.array_equal`` on the hops out, ``ring``, ``ola`` and ``hx``.  Cases: tests/clip_ragged_cases.py.

32 Griffin-Lim iterations.  B = 5, n_hops = (1, 0, 2, 9, 3): 15 frames, four chain workgroups of the wavefront-per-frame form with the last partly
filled, N = 1, 2, 3 and 9 in the fold, a zero-length stream between live ones.  Stream b has run WARM[b] hops before, so the streams' frame0 differ.
The calls through the C interface get a workspace full of NaNs, exactly as long as the library asks, with a canary behind it and behind hops_out."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: F401
import clip_ragged_cases as cases
from clip_ragged_cases import DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM, GPU_CASES, GPU_N_HOPS, SEED, SID0, WARM
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu

B5 = len(GPU_N_HOPS)
HOPS = max(GPU_N_HOPS)
CANARY = 0x5A


def _geo(tag):
    from oracle import pipeline_ref
    return {"S": pipeline_ref.PARAMS_S, "R1": pipeline_ref.PARAMS_R1, "L16": pipeline_ref.Params(16000, 512, 256, 64)}[tag]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def denoisers(dev):
    from audio_denoising_amd.pipeline import Denoiser
    cache = {}

    def get(tag, variant="plain"):
        key = (tag, variant if variant in ("bf16", "phin") else "plain")
        if key not in cache:
            p = _geo(tag)
            m = _model(dev, p.num_compressed_bins)
            m.conv_precision = "bf16" if variant == "bf16" else "fp32"
            cache[key] = Denoiser(m, p.sample_rate, p.n_fft, p.hop, p.n_mels, phase="input" if variant == "phin" else "random")
        return cache[key]
    return get


@pytest.fixture(scope="module")
def yard(dev, denoisers):
    """(tag, variant) -> per stream b: (its hops in (HOPS hop,) float32 or int16, its state (ring, ola, hx) after WARM[b] hops, [(state, hops out so
    far) after 1 .. GPU_N_HOPS[b] pushes]): the hop-by-hop streams, run once and only read by the tests"""
    from audio_denoising_amd.pipeline import DenoiserStream
    cache = {}

    def get(tag, variant="plain"):
        if (tag, variant) not in cache:
            dn = denoisers(tag, variant)
            sig = cases.signal(B5, (1 + max(WARM) + HOPS) * dn.hop, 300 + dn.n_fft)
            per = []
            for b in range(B5):
                s = DenoiserStream(dn, 1, stream_id0=SID0 + b, seed=SEED)
                head = (1 + WARM[b]) * dn.hop
                s.push(sig[b:b + 1, :head].to(dev))
                assert s.hops == WARM[b]
                start = (s.ring.clone(), s.ola.clone(), s.hx.clone())
                hops = sig[b, head:head + HOPS * dn.hop]
                fed = hops
                if variant == "s16":
                    hops = torch.from_numpy(cases.to_pcm(hops.numpy()))
                    fed = torch.from_numpy(hops.numpy().astype(np.float32) / np.float32(32767.0))          # app3.py:172, a true division
                after, outs = [], []
                for i in range(GPU_N_HOPS[b]):
                    outs.append(s.push(fed[None, i * dn.hop:(i + 1) * dn.hop].to(dev)))
                    ref = torch.cat(outs, dim=1)[0]
                    if variant == "s16":
                        ref = torch.from_numpy(cases.pcm_out(ref.cpu().numpy())).to(dev)
                    after.append(((s.ring.clone(), s.ola.clone(), s.hx.clone()), ref))
                assert start[1].abs().max() > 1e-3 and start[2].abs().max() > 1e-3
                per.append((hops.to(dev), start, after))
            cache[tag, variant] = per
        return cache[tag, variant]
    return get


def _start(per):
    return [torch.cat([per[b][1][k] for b in range(len(per))]).contiguous() for k in range(3)]


def _packed(per, n_hops, hop, first=None):
    first = first or [0] * len(n_hops)
    return torch.cat([per[b][0][first[b] * hop:(first[b] + n_hops[b]) * hop] for b in range(len(n_hops))]).contiguous()


def _check(per, n_hops, hop, out, state, start, done=None):
    """the packed hops `out` and `state` against the yardsticks: stream b has run done[b] + n_hops[b] hops, the last n_hops[b] of them in this call"""
    off = cases.offsets(n_hops)
    done = done or [0] * len(n_hops)
    for b in range(len(n_hops)):
        total = done[b] + n_hops[b]
        want = start if total == 0 else per[b][2][total - 1][0]
        rows = slice(b, b + 1)
        for k in range(3):
            assert torch.equal(state[k][rows], want[k][rows] if total == 0 else want[k]), (b, k)
        if n_hops[b]:
            assert torch.equal(out[off[b] * hop:off[b + 1] * hop], per[b][2][total - 1][1][done[b] * hop:]), b


def _raw(dn, dev, packed, n_hops, frame0, state, flags, want_rc=0):
    """dn_clip_process_ragged through the C interface: NaN-filled workspace of exactly the size asked for, canaries behind it and behind hops_out"""
    lib = dn.lib
    B, F = len(n_hops), sum(n_hops)
    need = lib.dn_clip_ragged_workspace_bytes(dn.plan.handle, B, F, dn._flags())
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 1024,), CANARY, dtype=torch.uint8, device=dev)
    ws[:need].view(torch.float32).fill_(float("nan"))
    out = torch.full(((F + 1) * dn.hop,), 7, dtype=packed.dtype, device=dev)
    s16 = packed.dtype == torch.int16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dn_clip_process_ragged(dn.model._native(dev), dn.plan.handle, packed.data_ptr(), int(s16), state[0].data_ptr(), state[1].data_ptr(),
                                    state[2].data_ptr(), out.data_ptr(), int(s16), None, SEED, SID0, (C.c_int32 * B)(*n_hops),
                                    (C.c_uint64 * B)(*frame0), dn.n_iter, dn.momentum, ws.data_ptr(), B, dn._flags() | flags, st)
    torch.cuda.synchronize()
    assert rc == want_rc, lib.dn_last_error()
    assert (ws[need:] == CANARY).all(), "the call wrote behind its workspace"
    assert (out[F * dn.hop:] == 7).all(), "the call wrote behind hops_out"
    return out[:F * dn.hop], ws[:need]


@pytest.mark.parametrize("case", sorted(GPU_CASES))
def test_ragged_call_equals_push_per_stream(dev, denoisers, yard, case):
    tag, gl, variant = GPU_CASES[case]
    dn = denoisers(tag, variant)
    per = yard(tag, variant)
    start = _start(per)
    state = [t.clone() for t in start]
    out, _ = _raw(dn, dev, _packed(per, GPU_N_HOPS, dn.hop), GPU_N_HOPS, WARM, state, gl)
    assert out.dtype == (torch.int16 if variant == "s16" else torch.float32)
    _check(per, GPU_N_HOPS, dn.hop, out, state, start)
    assert out.float().abs().max() > (30 if variant == "s16" else 1e-3)
    if variant == "bf16":          # the flag reaches the model stage
        assert not torch.equal(out, torch.cat([yard(tag)[b][2][-1][1] for b in range(B5) if GPU_N_HOPS[b]]))


def test_clip_ragged_and_a_second_call_that_continues_it(dev, denoisers, yard):
    dn = denoisers("S")
    per = yard("S")
    start = _start(per)
    state = [t.clone() for t in start]
    n1 = (1, 0, 1, 4, 2)
    n2 = tuple(a - b for a, b in zip(GPU_N_HOPS, n1))          # (0, 0, 1, 5, 1)
    out = dn.clip_ragged(_packed(per, n1, dn.hop), n1, *state, frame0=WARM, seed=SEED, stream_id0=SID0)
    _check(per, n1, dn.hop, out, state, start)
    out = dn.clip_ragged(_packed(per, n2, dn.hop, n1), n2, *state, frame0=[w + n for w, n in zip(WARM, n1)], seed=SEED, stream_id0=SID0)
    _check(per, n2, dn.hop, out, state, start, n1)


def test_clip_ragged_tiles_under_a_frame_cap_and_takes_injected_phases(dev, denoisers, yard):
    """drawn phases fed back reproduce the seeded call (whatever seed and stream id the call carries); a cap of 4 frames: rounds of (1, 0, 1, 1, 1),
    (0, 0, 1, 1, 1), (0, 0, 0, 2, 1), (0, 0, 0, 4, 0), (0, 0, 0, 1, 0) hops, finished streams held at 0, each round with its own hops' phases"""
    dn = denoisers("S")
    per = yard("S")
    start = _start(per)
    inits = torch.cat([dn.draw_phases(1, SEED + WARM[b] + i, SID0 + b) for b in range(B5) for i in range(GPU_N_HOPS[b])])
    for cap in (None, 4):
        state = [t.clone() for t in start]
        out = dn.clip_ragged(_packed(per, GPU_N_HOPS, dn.hop), GPU_N_HOPS, *state, seed=SEED + 1000, stream_id0=SID0 + 50, init_angles=inits, frame_cap=cap)
        _check(per, GPU_N_HOPS, dn.hop, out, state, start)
    state = [t.clone() for t in start]
    out = dn.clip_ragged(_packed(per, GPU_N_HOPS, dn.hop), GPU_N_HOPS, *state, frame0=WARM, seed=SEED, stream_id0=SID0, frame_cap=4)
    _check(per, GPU_N_HOPS, dn.hop, out, state, start)


# ------------------------------------------------------------------ whole clips
def _waves(dn, dev, dtypes):
    lengths = (dn.hop - 1, 2 * dn.hop, 3 * dn.hop + 17, 0)
    sig = cases.signal(len(lengths), max(lengths), 91)
    waves = []
    for b, (L, dt) in enumerate(zip(lengths, dtypes)):
        w = sig[b, :L]
        waves.append((torch.from_numpy(cases.to_pcm(4 * w.numpy())) if dt == torch.int16 else w).to(dev))
    return waves


@pytest.mark.parametrize("dtypes", ["float32", "int16", "mixed"])
def test_denoise_clips_equals_denoise_clip_per_clip(dev, denoisers, dtypes):
    dn = denoisers("S")
    f, s = torch.float32, torch.int16
    waves = _waves(dn, dev, {"float32": (f, f, f, f), "int16": (s, s, s, s), "mixed": (s, f, f, s)}[dtypes])
    outs = dn.denoise_clips(waves, seed=SEED, stream_id0=SID0)
    capped = dn.denoise_clips(waves, seed=SEED, stream_id0=SID0, frame_cap=7)          # several rounds, some with streams held at 0
    assert len(outs) == len(waves)
    for b, w in enumerate(waves):
        assert outs[b].shape == w.shape and outs[b].dtype == w.dtype, b
        if w.numel():
            want = dn.denoise_clip(w[None], seed=SEED, stream_id0=SID0 + b)[0]
            assert torch.equal(outs[b], want) and want.float().abs().max() > (30 if w.dtype == s else 1e-3), b
        assert torch.equal(capped[b], outs[b]), b


def test_denoise_clips_with_injected_phases(dev, denoisers):
    dn = denoisers("S")
    waves = _waves(dn, dev, (torch.float32,) * 4)
    g = torch.Generator().manual_seed(92)
    inits = [[torch.rand(dn.n_stft, 3, dtype=torch.complex64, generator=g).to(dev) for _ in range(dn.clip_hops(w.numel()) if w.numel() else 0)] for w in waves]
    outs = dn.denoise_clips(waves, init_angles=inits)
    for b, w in enumerate(waves):
        if w.numel():
            assert torch.equal(outs[b], dn.denoise_clip(w[None], init_angles=[z[None] for z in inits[b]])[0]), b
    assert not torch.equal(outs[2], dn.denoise_clips(waves)[2])
    with pytest.raises(ValueError):
        denoisers("S", "phin").denoise_clips(waves, init_angles=inits)


# ------------------------------------------------------------------ errors
def test_refusals_change_nothing(dev, denoisers, yard):
    from audio_denoising_amd._lib import DnError
    dn = denoisers("S")
    per = yard("S")
    start = _start(per)
    state = [t.clone() for t in start]
    packed = _packed(per, GPU_N_HOPS, dn.hop)
    bad = (
        (ValueError, dict(n_hops=(1, 0, 2, -9, 3))),
        (ValueError, dict(n_hops=(1, 0, 2, 9, 4))),                                        # hops_in does not hold sum(n_hops) hops
        (ValueError, dict(n_hops=GPU_N_HOPS[:4])),                                          # ring has another number of rows
        (ValueError, dict(frame_cap=0)),
        (DnError, dict(gl=DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM)),
        (DnError, dict(gl=64)),
    )
    for exc, kw in bad:
        a = dict(n_hops=GPU_N_HOPS, frame0=WARM, seed=SEED, stream_id0=SID0)
        a.update(kw)
        n = a.pop("n_hops")
        with pytest.raises(exc):
            dn.clip_ragged(packed, n, *state, **a)
        torch.cuda.synchronize()
        assert all(torch.equal(state[k], start[k]) for k in range(3)), kw
    with pytest.raises(ValueError):
        denoisers("S", "phin").clip_ragged(packed, GPU_N_HOPS, *state, init_angles=torch.zeros(sum(GPU_N_HOPS), dn.n_stft, 3, dtype=torch.complex64, device=dev))
    # the C interface: a negative entry, too many frames, a null workspace; state, hops out and workspace stay as they were
    for n_hops, code in (((1, 0, 2, -1, 3), -1), ((cases.MAX_FRAMES, 1, 0, 0, 0), -1)):
        lib = dn.lib
        ws = torch.full((4096,), CANARY, dtype=torch.uint8, device=dev)
        out = torch.full((16 * dn.hop,), 7.0, device=dev)
        rc = lib.dn_clip_process_ragged(dn.model._native(dev), dn.plan.handle, packed.data_ptr(), 0, state[0].data_ptr(), state[1].data_ptr(),
                                        state[2].data_ptr(), out.data_ptr(), 0, None, SEED, SID0, (C.c_int32 * B5)(*n_hops), None, dn.n_iter, dn.momentum,
                                        ws.data_ptr(), B5, 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == code and lib.dn_last_error(), n_hops
        assert (ws == CANARY).all() and (out == 7.0).all() and all(torch.equal(state[k], start[k]) for k in range(3)), n_hops
    # the wavefront-per-stream chains are built for n_fft 1024
    q = denoisers("L16")
    per_q = yard("L16")
    start_q = _start(per_q)
    state_q = [t.clone() for t in start_q]
    with pytest.raises(DnError) as e:
        q.clip_ragged(_packed(per_q, GPU_N_HOPS, q.hop), GPU_N_HOPS, *state_q, gl=DN_CLIP_GL_PER_STREAM)
    torch.cuda.synchronize()
    assert e.value.code == -2 and "1024" in str(e.value)
    assert all(torch.equal(state_q[k], start_q[k]) for k in range(3))
