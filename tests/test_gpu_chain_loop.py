"""The iteration loop of the wavefront-per-stream Griffin-Lim chain (glw_body) on the GPU: two iterations a trip, two register sets of previous
spectra that swap roles.  Everything that decides how many iterations a wavefront runs in one piece, where it starts and what it does at the end
-- short counts, hop groups of every size, the unequal segments of a deep pipe, the resume from a head start, the streaming fold -- against the
per-column chain (gl_body) of the one-hop pipe: frames, hx, overlap-add lines and emitted hops, torch.equal.  B = 3 and 5: a chain workgroup with
an idle wavefront; a full one and one with a single live wavefront.  The same matrix as tests/test_emu_chain_loop.py, plus 32 iterations."""
import pytest
import torch

from test_gpu_parity import _model, _params

pytestmark = pytest.mark.gpu

BATCHES = [3, 5]
N_FRAMES = 5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ctx(dev):
    """one model, one Denoiser per iteration count, the inputs and the yardstick results, all made once"""
    from audio_denoising_amd.pipeline import Denoiser
    p = _params("S")
    model = _model(dev, 5)
    g = torch.Generator().manual_seed(5150)
    c = {"p": p, "dev": dev, "dn": {}, "ref": {}}
    c["frames"] = {B: (0.1 * torch.randn(N_FRAMES, B, p.n_fft, generator=g)).to(dev) for B in BATCHES}
    c["pcm"] = {B: ((0.3 * torch.randn(B, 6 * p.hop, generator=g)).clamp(-1, 1) * 32767.0).to(torch.int16).to(dev) for B in BATCHES}

    def dn(n_iter):
        if n_iter not in c["dn"]:
            c["dn"][n_iter] = Denoiser(model, p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter)
        return c["dn"][n_iter]
    c["denoiser"] = dn
    return c


def _frames_run(ctx, B, n_iter, n, setup, H=0):
    """n chained hops in frame mode -> (frames out, hx); `setup` configures the pipe; H > 0: submitted as groups of H"""
    from audio_denoising_amd.pipeline import HopPipeline
    dn = ctx["denoiser"](n_iter)
    frames = ctx["frames"][B][:n]
    pipe = HopPipeline(dn, B)
    setup(pipe)
    hx, out = dn.init_hx(B), torch.empty_like(frames)
    if H:
        pipe.set_group(H)
        for i in range(0, n, H):
            pipe.submit_group(frames[i:i + H], hx, out[i:i + H], seed=77, stream_id0=5)
    else:
        for i in range(n):
            pipe.submit(frames[i], hx, out[i], seed=77, stream_id0=5)
    pipe.flush()
    torch.cuda.synchronize()
    assert pipe.counters()[2] is False
    return out, hx


def _per_column(pipe):
    from audio_denoising_amd import _lib
    pipe.set_gl_schedule(_lib.DN_GL_WAVE_PER_COLUMN)
    pipe.set_head_start(0)


def _frames_ref(ctx, B, n_iter, n=N_FRAMES):
    """the yardstick, once per shape: the one-hop pipe, a wavefront per column, no head start (a shorter run is a prefix only of the frames,
    not of hx, so every length is its own entry)"""
    key = ("frames", B, n_iter, n)
    if key not in ctx["ref"]:
        out, hx = _frames_run(ctx, B, n_iter, n, _per_column)
        assert torch.isfinite(out).all() and out.abs().max().item() > 1e-3
        ctx["ref"][key] = (out, hx)
    return ctx["ref"][key]


def _check_frames(ctx, B, n_iter, n, setup, H=0):
    out, hx = _frames_run(ctx, B, n_iter, n, setup, H)
    ref_out, ref_hx = _frames_ref(ctx, B, n_iter, n)
    assert torch.equal(out, ref_out) and torch.equal(hx, ref_hx)


def _stream_run(ctx, B, n_iter, setup, H=0):
    """six int16 pushes and the drain -> (emitted samples, ring, ola, hx)"""
    from audio_denoising_amd.pipeline import PipelinedStream
    dn = ctx["denoiser"](n_iter)
    p, pcm = ctx["p"], ctx["pcm"][B]
    ps = PipelinedStream(dn, B, seed=3, stream_id0=40)
    setup(ps)
    if H:
        ps.set_group(H)
        o = []
        for i in range(0, 6, H):
            o += list(ps.push_group(torch.stack([pcm[:, j * p.hop:(j + 1) * p.hop] for j in range(i, i + H)]).contiguous()))
        tail, valid = ps.flush_group(s16=True)
        assert valid == H
        o += list(tail)
    else:
        o = [ps.push(pcm[:, i * p.hop:(i + 1) * p.hop].contiguous()) for i in range(6)] + [ps.flush(s16=True)]
    ring, ola, hx, frames = ps.state()
    torch.cuda.synchronize()
    assert frames == 5
    return torch.cat(o, 1), ring, ola, hx


def _check_stream(ctx, B, n_iter, setup, lag_hops, H=0):
    key = ("stream", B, n_iter)
    if key not in ctx["ref"]:
        ctx["ref"][key] = _stream_run(ctx, B, n_iter, _per_column)
        assert ctx["ref"][key][0].abs().max().item() > 0
    ea, ring_a, ola_a, hx_a = ctx["ref"][key]
    eb, ring_b, ola_b, hx_b = _stream_run(ctx, B, n_iter, setup, H)
    lag = lag_hops * ctx["p"].hop
    assert torch.equal(eb[:, lag:lag + ea.shape[1]], ea[:, :eb.shape[1] - lag]) and not eb[:, :lag].any()
    assert eb.shape[1] - lag >= 6 * ctx["p"].hop                   # every sample the yardstick emitted for the six pushes was compared
    assert torch.equal(ring_a, ring_b) and torch.equal(ola_a, ola_b) and torch.equal(hx_a, hx_b)


def _per_stream(pipe):
    from audio_denoising_amd import _lib
    pipe.set_gl_schedule(_lib.DN_GL_WAVE_PER_STREAM)
    pipe.set_head_start(0)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_iter", [0, 1, 2, 3, 4, 5])
def test_whole_chain_at_every_short_count(ctx, B, n_iter):
    """zero trips, the odd iteration alone, one trip, one trip and the odd iteration, ...: as one piece under the one-hop pipe (frame mode and
    the streaming emit), and as the chain waves of a hop group"""
    _check_frames(ctx, B, n_iter, 3, _per_stream)
    _check_frames(ctx, B, n_iter, 3, lambda pipe: None, H=2)
    _check_stream(ctx, B, n_iter, _per_stream, 0)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_hop_groups_of_every_size(ctx, B, H):
    """five hops as groups of H (full groups and a short last one; H = 3: an idle chain wavefront), three iterations"""
    _check_frames(ctx, B, 3, N_FRAMES, lambda pipe: None, H=H)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_deep_pipe_segments_on_both_parities(ctx, B, depth):
    """five iterations in `depth` segments of unequal length: segments start on odd and on even iterations and run an odd and an even number
    of them; frame mode, then the streaming emit `depth - 1` pushes later"""
    _check_frames(ctx, B, 5, N_FRAMES, lambda pipe: pipe.set_depth(depth))
    _check_stream(ctx, B, 5, lambda ps: ps.set_depth(depth), depth - 1)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("head_start,depth", [(3, 1), (2, 1), (3, 2)])
def test_resume_from_a_head_start(ctx, B, head_start, depth):
    """the front workgroup's per-column chain parks X and the previous spectra after 3 or 2 iterations; the wavefront-per-stream chain resumes
    there, as one piece or as the first segment of a deep pipe"""
    from audio_denoising_amd import _lib

    def setup(pipe):
        if depth > 1:
            pipe.set_depth(depth)
        else:
            pipe.set_gl_schedule(_lib.DN_GL_WAVE_PER_STREAM)
        pipe.set_head_start(head_start)
    _check_frames(ctx, B, 5, 3, setup)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H", [2, 3])
def test_streaming_groups_with_a_flush(ctx, B, H):
    """the chains of one stream finish in the same launch and fold into its overlap-add line in order: the one-hop pipe's samples H - 1 hops
    later, the same ring, overlap-add line and hx after the flush group"""
    _check_stream(ctx, B, 3, lambda ps: None, H - 1, H=H)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("mode", ["H4", "depth4"])
def test_thirty_two_iterations(ctx, B, mode):
    """the count the product runs: sixteen trips as one piece (groups of four), segments of eight (depth 4)"""
    if mode == "H4":
        _check_frames(ctx, B, 32, N_FRAMES, lambda pipe: None, H=4)
    else:
        _check_frames(ctx, B, 32, N_FRAMES, lambda pipe: pipe.set_depth(4))
