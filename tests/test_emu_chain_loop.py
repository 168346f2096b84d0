"""The iteration loop of the wavefront-per-stream Griffin-Lim chain (glw_body) on the host emulation of the kernel sources.  The loop runs two
iterations a trip with two register sets of previous spectra that swap roles; a count that is odd, zero or one, a segment of a deep pipe that
starts or stops on either parity, a chain resumed from a head start and the chain waves of a hop group (an idle one at H = 3) must all leave
exactly what the per-column chain (gl_body) of the one-hop pipe leaves: frames, hx, overlap-add lines, emitted hops -- np.array_equal, no
tolerance.  B = 3: one chain workgroup with an idle wavefront.  The emulator runs a work-item per OS thread, so hops are few; the gpu tier
(tests/test_gpu_chain_loop.py) runs the same matrix at B = 3 and 5 and adds 32 iterations."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
from audio_denoising_amd._lib import DN_GL_AUTO, DN_GL_WAVE_PER_COLUMN, DN_GL_WAVE_PER_STREAM, DspCfg  # noqa: E402
from oracle import dsp_ref, pipeline_ref  # noqa: E402
from test_emu_kernels import _run_groups, _run_pipe, make_model  # noqa: E402

P = pipeline_ref.PARAMS_S
B = 3


@pytest.fixture(scope="module")
def lib():
    return emu.load()


@pytest.fixture(scope="module")
def dsp(lib):
    fb = dsp_ref.melscale_fbanks(P.n_stft, P.n_mels, P.sample_rate).numpy()
    h = C.c_void_p()
    lib.check(lib.dn_dsp_create(C.byref(DspCfg(P.sample_rate, P.n_fft, P.hop, P.n_mels)), emu.ptr(emu.f32(fb)), None, None, C.byref(h)))
    yield h
    lib.dn_dsp_destroy(h)


@pytest.fixture(scope="module")
def model(lib):
    m = make_model(lib, 5)
    yield m
    lib.dn_model_destroy(m)


G = {"signal": load_golden("stream_S.npz")["signal"]}
_REF = {}


def _ref(lib, dsp, model, n_hops, n_iter, stream=False):
    """the yardstick, computed once per shape: the one-hop pipe with one wavefront per COLUMN and no head start"""
    key = (n_hops, n_iter, stream)
    if key not in _REF:
        outs = _run_pipe(lib, dsp, model, DN_GL_WAVE_PER_COLUMN, B, n_hops, G, n_iter=n_iter, stream=stream)
        assert np.abs(np.concatenate(outs[:-3], axis=1) if stream else outs[0]).max() > 0          # (the comparison is of real output)
        for o in outs:
            o.setflags(write=False)
        _REF[key] = outs
    return _REF[key]


def _same(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), i


@pytest.mark.parametrize("n_iter", [0, 1, 2, 3, 4, 5])
def test_whole_chain_at_every_short_count(lib, dsp, model, n_iter):
    """zero trips, the odd iteration alone, one trip, one trip and the odd iteration, ...: the chain as one piece under the one-hop pipe and as
    the chain waves of a hop group"""
    ref = _ref(lib, dsp, model, 2, n_iter)
    _same(ref, _run_pipe(lib, dsp, model, DN_GL_WAVE_PER_STREAM, B, 2, G, n_iter=n_iter))
    _same(ref, _run_groups(lib, dsp, model, B, 2, G, 2, n_iter=n_iter))


@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_hop_groups_of_every_size(lib, dsp, model, H):
    """four hops as groups of H (H = 3: a full group with an idle chain wavefront, then a short one), three iterations"""
    _same(_ref(lib, dsp, model, 4, 3), _run_groups(lib, dsp, model, B, 4, G, H, n_iter=3))


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_deep_pipe_segments_on_both_parities(lib, dsp, model, depth):
    """five iterations in `depth` segments of unequal length (2/3, 1/2/2, 1/1/1/2): segments start on odd and on even iterations, run an odd
    and an even number of them, and every boundary goes through park_segment and the resume from it"""
    n_hops = depth + 1
    _same(_ref(lib, dsp, model, n_hops, 5), _run_pipe(lib, dsp, model, DN_GL_AUTO, B, n_hops, G, n_iter=5, depth=depth))


@pytest.mark.parametrize("head_start,depth", [(3, 1), (2, 1), (3, 2)])
def test_resume_from_a_head_start(lib, dsp, model, head_start, depth):
    """the front workgroup's per-column chain runs the first iterations and parks X and the previous spectra; the wavefront-per-stream chain
    resumes on an odd (3) or even (2) iteration, as one piece or as the first segment of a deep pipe"""
    n_hops = depth + 1
    got = _run_pipe(lib, dsp, model, DN_GL_WAVE_PER_STREAM if depth == 1 else DN_GL_AUTO, B, n_hops, G, n_iter=5, depth=depth, head_start=head_start)
    _same(_ref(lib, dsp, model, n_hops, 5), got)


@pytest.mark.parametrize("H", [2, 3])
def test_streaming_groups_with_a_flush(lib, dsp, model, H):
    """the streaming group form: the chains of one stream finish in the same launch and fold into its overlap-add line in order; the emitted
    stream is the one-hop pipe's H - 1 hops later, and ring, overlap-add line and hx after the flush are the same"""
    n_hops = 5                                              # six pushes: three groups of two, two of three; then the flush group
    a = _ref(lib, dsp, model, n_hops, 3, stream=True)
    b = _run_groups(lib, dsp, model, B, n_hops, G, H, stream=True, n_iter=3)
    ea, eb = np.concatenate(a[:-3], axis=1), np.concatenate(b[:-4], axis=1)
    lag = (H - 1) * P.hop
    assert np.array_equal(eb[:, lag:lag + ea.shape[1]], ea) and not eb[:, :lag].any() and np.abs(ea).max() > 0
    assert not eb[:, lag + ea.shape[1]:].any()
    _same(a[-3:], b[-3:])
