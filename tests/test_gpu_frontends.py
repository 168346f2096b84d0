"""The glue of the Python front ends on the MI355X (``pytest -m gpu``): what every front end does with ``init_angles``.

  1. A ``Denoiser(phase="input")`` refuses ``init_angles`` at EVERY front end that takes them, with ValueError, before it launches anything: the
     counters of the pipe or pool and the ``hops`` of the stream are what they were.  B = 2, one hop each, n_iter 1; n_fft 512, and 1024 for the
     group calls (groups are built there).
  2. The two group calls, whose (H, B, K, 3) phases are packed in one piece: the phases ``draw_phases`` returns for (seed + f, stream_id0), passed
     back as ``init_angles``, reproduce the seeded calls bit for bit.  B = 2, groups of 2, three launches, n_fft 1024.
tests/test_frontend_glue.py holds the packer, the tensor check and the ragged schedule to their definitions on the CPU."""
import numpy as np
import pytest
import torch

import phase_cases as pcs
from test_gpu_parity import _model

pytestmark = pytest.mark.gpu

B = 2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


def _denoiser(dev, n_fft, phase, n_iter=1):
    from audio_denoising_amd.pipeline import Denoiser
    p = pcs.geometry(n_fft)
    return Denoiser(_model(dev, p.num_compressed_bins), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter, phase=phase)


def _refused(call):
    with pytest.raises(ValueError, match="init_angles"):
        call()


def test_input_phase_denoiser_refuses_init_angles_at_every_front_end(dev):
    from audio_denoising_amd.pipeline import DenoiserStream, HopPipeline, PipelinedStream
    from audio_denoising_amd.sessions import SessionPool
    dn, dng = _denoiser(dev, 512, "input"), _denoiser(dev, 1024, "input")

    def ia(d, *lead):
        return torch.zeros(*lead, d.n_stft, 3, dtype=torch.complex64, device=dev)

    def zeros(*shape):
        return torch.zeros(*shape, device=dev)

    # the hop body
    _refused(lambda: dn.process_frame(zeros(B, dn.n_fft), None, init_angles=ia(dn, B)))
    # frame pipes: one hop, a group
    pipe = HopPipeline(dn, B)
    before = pipe.counters()
    _refused(lambda: pipe.submit(zeros(B, dn.n_fft), dn.init_hx(B), zeros(B, dn.n_fft), init_angles=ia(dn, B)))
    assert pipe.counters() == before
    pipe = HopPipeline(dng, B)
    pipe.set_group(2)
    before = pipe.counters()
    _refused(lambda: pipe.submit_group(zeros(2, B, dng.n_fft), dng.init_hx(B), zeros(2, B, dng.n_fft), init_angles=ia(dng, 2, B)))
    assert pipe.counters() == before
    # stream pipes: one hop, a group
    st = PipelinedStream(dn, B)
    before = st.counters()
    _refused(lambda: st.push_(zeros(B, dn.hop), zeros(B, dn.hop), init_angles=ia(dn, B)))
    assert st.counters() == before
    st = PipelinedStream(dng, B)
    st.set_group(2)
    before = st.counters()
    _refused(lambda: st.push_group_(zeros(2, B, dng.hop), zeros(2, B, dng.hop), init_angles=ia(dng, 2, B)))
    assert st.counters() == before
    # the unpipelined stream, hop by hop and through clip mode: primed, so that the push below would run its first hop
    for name in ("push", "push_many"):
        ds = DenoiserStream(dn, B)
        assert ds.push(zeros(B, dn.hop)).shape == (B, 0) and ds.hops == 0
        _refused(lambda: getattr(ds, name)(zeros(B, dn.hop), init_angles_per_hop=[ia(dn, B)]))
        assert ds.hops == 0 and not ds.ola.any() and not ds.hx.any()
    # clips
    L = dn.hop + 3
    n = dn.clip_hops(L)
    _refused(lambda: dn.denoise_clip(zeros(B, L), init_angles=[ia(dn, B)] * n))
    _refused(lambda: dn.denoise_clips([zeros(L), zeros(L)], init_angles=[[ia(dn)] * n] * 2))
    ring, ola, hx = zeros(B, dn.n_fft), zeros(B, dn.n_fft), dn.init_hx(B)
    _refused(lambda: dn.clip_ragged(zeros(B * dn.hop), [1, 1], ring, ola, hx, init_angles=ia(dn, B)))
    assert not ring.any() and not ola.any() and not hx.any()
    # sessions
    pool = SessionPool(dn, 3)
    slots = [pool.open() for _ in range(B)]
    before = [pool.counters(s) for s in slots]
    _refused(lambda: pool.push(slots, zeros(B, dn.hop), init_angles=ia(dn, B)))
    assert [pool.counters(s) for s in slots] == before and not pool._pushes.any()


def test_drawn_phases_reproduce_the_seeded_group_calls(dev):
    from audio_denoising_amd.pipeline import HopPipeline, PipelinedStream
    H, launches, seed, sid0 = 2, 3, 77, 5
    dn = _denoiser(dev, 1024, "random", n_iter=2)
    sig = torch.from_numpy(pcs.stream_signal(B, 1024, H * launches)).to(dev)          # (B, (H * launches + 1) hops)
    drawn = [dn.draw_phases(B, seed + f, sid0) for f in range(H * launches)]          # of frame f
    # frame mode: the f-th frame of the pipe draws from seed + f
    frames = torch.stack([sig[:, f * dn.hop:f * dn.hop + dn.n_fft] for f in range(H * launches)]).contiguous()
    got = []
    for injected in (False, True):
        pipe = HopPipeline(dn, B)
        pipe.set_group(H)
        out, hx = torch.empty_like(frames), dn.init_hx(B)
        for g in range(launches):
            rows = slice(g * H, (g + 1) * H)
            pipe.submit_group(frames[rows], hx, out[rows], seed=seed, stream_id0=sid0, init_angles=torch.stack(drawn[rows]) if injected else None)
        pipe.flush()
        torch.cuda.synchronize()
        got.append((out, hx))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert float(got[0][0].abs().max()) > 1e-3 and torch.isfinite(got[0][0]).all()
    # stream mode: hop j delivers frame j - 1 (hop 0 primes and draws nothing: any phases)
    hops = torch.stack([sig[:, j * dn.hop:(j + 1) * dn.hop] for j in range(H * launches)]).contiguous()
    got = []
    for injected in (False, True):
        st = PipelinedStream(dn, B, stream_id0=sid0, seed=seed)
        st.set_group(H)
        out = torch.empty_like(hops)
        for g in range(launches):
            rows = slice(g * H, (g + 1) * H)
            ia = torch.stack([drawn[max(j - 1, 0)] for j in range(g * H, (g + 1) * H)]) if injected else None
            st.push_group_(hops[rows], out[rows], init_angles=ia)
        tail, valid = st.flush_group()
        state = st.state()
        torch.cuda.synchronize()
        got.append((out, tail, valid) + tuple(state))
    assert got[0][2] == got[1][2] and got[0][6] == got[1][6] == H * launches - 1
    assert all(torch.equal(a, b) for a, b in zip(got[0][:2] + got[0][3:6], got[1][:2] + got[1][3:6]))
    assert float(got[0][0].abs().max()) > 1e-3 and np.isfinite(got[0][0].cpu().numpy()).all()
