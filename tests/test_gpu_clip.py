"""Clip mode on the MI355X (``pytest -m gpu``): ``dn_clip_process`` -- N hops of B streams per call -- behind ``DenoiserStream.push_many`` and
``Denoiser.denoise_clip``.  The call is defined as "exactly N calls of ``dn_stream_step``, bit for bit": the yardstick is ``DenoiserStream.push``
(the unchanged ``dn_stream_step``) fed the same samples, seed and stream ids, and every comparison is ``torch.equal`` / ``np.array_equal`` on the
hops out, ``ring``, ``ola`` and ``hx``.  Only ``denoise_clip`` against the oracle carries a tolerance: ``_wave_close`` of tests/test_gpu_parity.py.

  S   = 16 kHz, n_fft 1024, hop 512, 80 mels      R1 = 48 kHz, n_fft 1536, hop 768, 64 mels      L16 = 16 kHz, n_fft 512, hop 256, 64 mels

32 Griffin-Lim iterations.  Shapes are the smallest at which the code takes another path: N = 1 (only the old overlap-add line feeds the output),
N = 2 (the old line's second half under hop 0's frame), N >= 3 (the general term); B x N = 1, 5, 9, 12 frames for the wavefront-per-frame chains
(a partly filled workgroup, a full and a partly filled one, several).  Every stream has run two hops before the clip call."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN  # noqa: F401
from test_gpu_parity import _model, _state_dict, _wave_close

pytestmark = pytest.mark.gpu

SEED, SID0, B3 = 17, 2 ** 33 + 5, 3
WARM, HOPS = 2, 9


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

    def get(tag, precision="fp32"):
        if (tag, precision) not in cache:
            p = _geo(tag)
            m = _model(dev, p.num_compressed_bins)
            m.conv_precision = precision
            cache[tag, precision] = Denoiser(m, p.sample_rate, p.n_fft, p.hop, p.n_mels)
        return cache[tag, precision]
    return get


def _signal(n, length, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(length) / 16000.0
    tones = torch.stack([(0.05 + 0.2 * k) * torch.sin(2 * np.pi * (180.0 + 95.0 * k) * t) for k in range(n)])
    return (tones + 0.03 * torch.randn(n, length, generator=g)).float()


def _snap(s):
    return s.ring.clone(), s.ola.clone(), s.hx.clone(), s.hops


def _fork(dn, snap, rows=slice(None), sid0=SID0, **kw):
    """a DenoiserStream that carries the state `snap` of the streams `rows`"""
    from audio_denoising_amd.pipeline import DenoiserStream
    ring, ola, hx, hops = snap
    s = DenoiserStream(dn, ring[rows].shape[0], stream_id0=sid0, seed=SEED, **kw)
    s.ring, s.ola, s.hx, s.hops = ring[rows].clone(), ola[rows].clone(), hx[rows].clone(), hops
    s.filled = dn.n_fft - dn.hop
    return s


def _same(s, snap, rows=slice(None)):
    ring, ola, hx, hops = snap
    return torch.equal(s.ring, ring[rows]) and torch.equal(s.ola, ola[rows]) and torch.equal(s.hx, hx[rows]) and s.hops == hops


@pytest.fixture(scope="module")
def yard(dev, denoisers):
    """tag -> (the hops (3, HOPS hop) behind the warm-up, the state after WARM hops, [(state, hops out so far) after 1 .. HOPS pushes]): the
    hop-by-hop stream, run once per geometry and only read by the tests"""
    from audio_denoising_amd.pipeline import DenoiserStream
    cache = {}

    def get(tag):
        if tag not in cache:
            dn = denoisers(tag)
            sig = _signal(B3, (1 + WARM + HOPS) * dn.hop, 100 + dn.n_fft).to(dev)
            s = DenoiserStream(dn, B3, stream_id0=SID0, seed=SEED)
            assert s.push(sig[:, :(1 + WARM) * dn.hop]).shape == (B3, WARM * dn.hop)
            start, after, outs = _snap(s), [], []
            rest = sig[:, (1 + WARM) * dn.hop:]
            for k in range(HOPS):
                outs.append(s.push(rest[:, k * dn.hop:(k + 1) * dn.hop]))
                after.append((_snap(s), torch.cat(outs, dim=1)))
            assert start[1].abs().max() > 1e-3 and start[2].abs().max() > 1e-3 and after[-1][1].abs().max() > 1e-3
            cache[tag] = (rest, start, after)
        return cache[tag]
    return get


# ------------------------------------------------------------------ N hops per call
@pytest.mark.parametrize("N", [1, 2, 3, 9])
@pytest.mark.parametrize("tag", ["S", "R1", "L16"])
def test_push_many_equals_push_hop_by_hop(denoisers, yard, tag, N):
    dn = denoisers(tag)
    rest, start, after = yard(tag)
    s = _fork(dn, start)
    out = s.push_many(rest[:, :N * dn.hop])
    assert torch.equal(out, after[N - 1][1])
    assert _same(s, after[N - 1][0])


def test_cutting_the_clip_and_handing_over_to_push_and_back(denoisers, yard):
    dn = denoisers("S")
    rest, start, after = yard("S")
    s = _fork(dn, start)
    a = s.push_many(rest[:, :5 * dn.hop])
    assert _same(s, after[4][0])
    b = s.push_many(rest[:, 5 * dn.hop:])
    assert torch.equal(torch.cat([a, b], dim=1), after[8][1]) and _same(s, after[8][0])
    # a stream that carries the state a clip call returned goes on with push, bit for bit ...
    s = _fork(dn, start)
    a = s.push_many(rest[:, :5 * dn.hop])
    b = _fork(dn, _snap(s)).push(rest[:, 5 * dn.hop:])
    assert torch.equal(torch.cat([a, b], dim=1), after[8][1])
    # ... and the other way round (samples that do not fill a hop wait in either)
    s = _fork(dn, start)
    a = s.push(rest[:, :3 * dn.hop + 100])
    b = s.push_many(rest[:, 3 * dn.hop + 100:])
    assert a.shape[1] == 3 * dn.hop and torch.equal(torch.cat([a, b], dim=1), after[8][1]) and _same(s, after[8][0])


def test_push_many_tiles_under_a_frame_cap(denoisers, yard):
    """a cap of 4 frames on 3 streams x 5 hops: five calls of one hop each"""
    dn = denoisers("S")
    rest, start, after = yard("S")
    s = _fork(dn, start, clip_frame_cap=4)
    assert torch.equal(s.push_many(rest[:, :5 * dn.hop]), after[4][1]) and _same(s, after[4][0])
    s = _fork(dn, start)
    assert torch.equal(s.push_many(rest[:, :5 * dn.hop], frame_cap=7), after[4][1]) and _same(s, after[4][0])          # 2 + 2 + 1 hops


# ------------------------------------------------------------------ the chain schedules at n_fft 1024
@pytest.mark.parametrize("B,N", [(1, 1), (1, 5), (3, 3), (3, 4)])
def test_chain_schedules_give_equal_bits(denoisers, yard, B, N):
    from audio_denoising_amd._lib import DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM
    dn = denoisers("S")
    rest, start, after = yard("S")
    rows = slice(0, B)
    want_state, want_out = after[N - 1]
    for gl in (DN_CLIP_GL_PER_STREAM, DN_CLIP_GL_PER_COLUMN, 0):
        ring, ola, hx = start[0][rows].clone(), start[1][rows].clone(), start[2][rows].clone()
        out = dn._clip(rest[rows, :N * dn.hop].contiguous(), ring, ola, hx, None, SEED + start[3], SID0, gl=gl)
        assert torch.equal(out, want_out[rows]), gl
        assert torch.equal(ring, want_state[0][rows]) and torch.equal(ola, want_state[1][rows]) and torch.equal(hx, want_state[2][rows]), gl


@pytest.mark.parametrize("tag", ["L16", "R1"])
def test_the_per_stream_flag_is_refused_off_1024(denoisers, yard, tag):
    from audio_denoising_amd._lib import DN_CLIP_GL_PER_STREAM, DnError
    dn = denoisers(tag)
    rest, start, _ = yard(tag)
    ring, ola, hx = start[0].clone(), start[1].clone(), start[2].clone()
    with pytest.raises(DnError) as e:
        dn._clip(rest[:, :dn.hop].contiguous(), ring, ola, hx, None, SEED, SID0, gl=DN_CLIP_GL_PER_STREAM)
    torch.cuda.synchronize()
    assert e.value.code == -2 and "1024" in str(e.value)
    assert torch.equal(ring, start[0]) and torch.equal(ola, start[1]) and torch.equal(hx, start[2])


# ------------------------------------------------------------------ transport and phases
def test_int16_in_and_out(dev, denoisers):
    from audio_denoising_amd.pipeline import DenoiserStream
    dn = denoisers("S")
    N = 3
    pcm = (_signal(B3, (N + 1) * dn.hop, 51).numpy() * 32767.0).astype(np.int16)
    as_float = torch.from_numpy(pcm.astype(np.float32) / np.float32(32767.0)).to(dev)          # app3.py:172, a true division
    ref = DenoiserStream(dn, B3, stream_id0=SID0, seed=SEED)
    ref.push(as_float[:, :dn.hop])
    # an overlap-add line with samples past full scale, so that the first two hops out clip at +-32767
    ref.ola = (0.8 * torch.randn(B3, dn.n_fft, generator=torch.Generator().manual_seed(52))).to(dev)
    start = _snap(ref)
    ref_out = ref.push(as_float[:, dn.hop:]).cpu().numpy()
    want = (np.clip(ref_out, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)              # app3.py:244-245: clip, scale, truncate
    assert (want == 32767).any() and (want == -32767).any() and np.abs(want[:, 2 * dn.hop:]).max() > 30
    ring, ola, hx = start[0].clone(), start[1].clone(), start[2].clone()
    out = dn._clip(torch.from_numpy(pcm[:, dn.hop:]).to(dev).contiguous(), ring, ola, hx, None, SEED, SID0)
    assert out.dtype == torch.int16 and np.array_equal(out.cpu().numpy(), want)
    assert _same(ref, (ring, ola, hx, N))


def test_injected_phases_equal_the_same_phases_handed_to_push(dev, denoisers, yard):
    dn = denoisers("S")
    rest, start, _ = yard("S")
    N = 3
    g = torch.Generator().manual_seed(61)
    inits = [torch.rand(B3, dn.n_stft, 3, dtype=torch.complex64, generator=g).to(dev) for _ in range(N)]
    ref = _fork(dn, start)
    want = ref.push(rest[:, :N * dn.hop], inits)
    s = _fork(dn, start)
    assert torch.equal(s.push_many(rest[:, :N * dn.hop], inits), want) and _same(s, _snap(ref))
    s = _fork(dn, start)
    assert torch.equal(s.push_many(rest[:, :N * dn.hop], inits, frame_cap=2 * B3), want) and _same(s, _snap(ref))      # tiles take their own hops' phases


def test_drawn_phases_fed_back_reproduce_the_seeded_call(denoisers, yard):
    dn = denoisers("S")
    rest, start, after = yard("S")
    N = 3
    inits = [dn.draw_phases(B3, SEED + start[3] + i, SID0) for i in range(N)]
    s = _fork(dn, start)
    assert torch.equal(s.push_many(rest[:, :N * dn.hop], inits), after[N - 1][1]) and _same(s, after[N - 1][0])


def test_streams_are_independent(denoisers, yard):
    """three streams in one call equal three calls of one stream with stream_id0 + b"""
    dn = denoisers("L16")
    rest, start, after = yard("L16")
    N = 3
    for b in range(B3):
        rows = slice(b, b + 1)
        s = _fork(dn, start, rows=rows, sid0=SID0 + b)
        assert torch.equal(s.push_many(rest[rows, :N * dn.hop]), after[N - 1][1][rows]), b
        assert _same(s, after[N - 1][0], rows), b


def test_bf16_conv_tiles(dev, denoisers):
    from audio_denoising_amd.pipeline import DenoiserStream
    dn = denoisers("S", "bf16")
    fp32 = denoisers("S")
    N = 3
    sig = _signal(B3, (N + 1) * dn.hop, 71).to(dev)
    ref = DenoiserStream(dn, B3, stream_id0=SID0, seed=SEED)
    want = ref.push(sig)
    s = DenoiserStream(dn, B3, stream_id0=SID0, seed=SEED)
    assert torch.equal(s.push_many(sig), want) and _same(s, _snap(ref))
    other = DenoiserStream(fp32, B3, stream_id0=SID0, seed=SEED).push(sig)
    assert not torch.equal(other, want)                   # the flag reaches the model stage


# ------------------------------------------------------------------ a whole clip
def _clip_by_push(dn, wave, seed, sid0, inits=None):
    """denoise_clip restated on DenoiserStream.push: prime, pad to whole hops plus the two that drain the line, drop the first hop out, trim"""
    from audio_denoising_amd.pipeline import DenoiserStream
    B, L = wave.shape
    n_hops = -(-L // dn.hop) + 1
    padded = torch.zeros(B, (n_hops + 1) * dn.hop, dtype=torch.float32, device=wave.device)
    padded[:, :L] = wave
    out = DenoiserStream(dn, B, stream_id0=sid0, seed=seed).push(padded, inits)
    assert out.shape == (B, n_hops * dn.hop)
    return out[:, dn.hop:dn.hop + L]


@pytest.mark.parametrize("tag", ["S", "L16"])
def test_denoise_clip_equals_its_restatement_on_push(dev, denoisers, tag):
    dn = denoisers(tag)
    L = 5 * dn.hop + 37
    wave = _signal(2, L, 81).to(dev)
    out = dn.denoise_clip(wave, seed=SEED, stream_id0=SID0)
    assert out.shape == wave.shape and out.dtype == wave.dtype
    assert torch.equal(out, _clip_by_push(dn, wave, SEED, SID0)) and out.abs().max() > 1e-3
    assert dn.clip_hops(L) == 7


def test_denoise_clip_int16(dev, denoisers):
    dn = denoisers("L16")
    L = 5 * dn.hop + 37
    pcm = np.clip(_signal(2, L, 82).numpy() * 4 * 32767.0, -32768, 32767).astype(np.int16)
    out = dn.denoise_clip(torch.from_numpy(pcm).to(dev), seed=SEED, stream_id0=SID0)
    assert out.shape == pcm.shape and out.dtype == torch.int16
    as_float = torch.from_numpy(pcm.astype(np.float32) / np.float32(32767.0)).to(dev)
    ref = _clip_by_push(dn, as_float, SEED, SID0).cpu().numpy()
    want = (np.clip(ref, -1.0, 1.0) * np.float32(32767.0)).astype(np.int16)
    assert np.array_equal(out.cpu().numpy(), want) and np.abs(want).max() > 30


def test_denoise_clip_matches_the_oracle_stream(dev, denoisers):
    from oracle import pipeline_ref
    dn = denoisers("S")
    p = _geo("S")
    B, L = 2, 5 * dn.hop + 37
    wave = _signal(B, L, 83)
    n_hops = dn.clip_hops(L)
    g = torch.Generator().manual_seed(84)
    inits = [torch.rand(B, p.n_stft, 3, dtype=torch.complex64, generator=g) for _ in range(n_hops)]
    padded = torch.zeros(B, (n_hops + 1) * p.hop)
    padded[:, :L] = wave
    with torch.no_grad():
        ref = pipeline_ref.StreamRef(_state_dict("dari_tult"), p, B).push(padded, inits)
    assert ref.shape == (B, n_hops * p.hop)
    out = dn.denoise_clip(wave.to(dev), init_angles=[ia.to(dev) for ia in inits])
    _wave_close(out.cpu().numpy(), ref[:, p.hop:p.hop + L].numpy())
    assert ref[:, p.hop:p.hop + L].abs().max() > 1e-3


# ------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_any_launch(dev, denoisers, yard):
    from audio_denoising_amd._lib import DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM
    dn = denoisers("S")
    rest, start, _ = yard("S")
    lib = dn.lib
    ring, ola, hx = start[0].clone(), start[1].clone(), start[2].clone()
    hops_in = rest[:, :2 * dn.hop].contiguous()
    out = torch.zeros_like(hops_in)
    ws = torch.empty(lib.dn_clip_workspace_bytes(dn.plan.handle, B3, 2), dtype=torch.uint8, device=dev)
    model_h = dn.model._native(dev)

    def call(B=B3, N=2, flags=0, ws_ptr=ws.data_ptr(), ring_ptr=ring.data_ptr()):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        return lib.dn_clip_process(model_h, dn.plan.handle, hops_in.data_ptr(), 0, ring_ptr, ola.data_ptr(), hx.data_ptr(), out.data_ptr(), 0, None,
                                   SEED, SID0, dn.n_iter, dn.momentum, ws_ptr, B, N, flags, st)
    for kw in (dict(N=0), dict(B=0), dict(flags=DN_CLIP_GL_PER_COLUMN | DN_CLIP_GL_PER_STREAM), dict(ws_ptr=None), dict(ring_ptr=None)):
        assert call(**kw) < 0, kw
        assert lib.dn_last_error(), kw
        torch.cuda.synchronize()
        assert torch.equal(ring, start[0]) and torch.equal(ola, start[1]) and torch.equal(hx, start[2]) and not out.any(), kw
    assert call() == 0          # the same arguments, valid: the call goes through
    torch.cuda.synchronize()
    assert out.abs().max() > 1e-3
