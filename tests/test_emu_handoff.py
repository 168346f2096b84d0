"""The pair-order hand-off of the real transforms through the wave's LDS tile (rfft_split_pairs / irfft_merge_pairs, dn_wavefft.hpp) on the
host emulation of the kernel sources.

1.  The earlier hand-off (ds_bpermute and per-value selects for lane 0) stays in the sources behind -DDN_HANDOFF_BPERMUTE.  A second emulator
    library is built with it -- the g++ line of tests/emu/emu.py plus the define -- and the same short chain runs through both: B = 3 (a chain
    workgroup with an idle wavefront), three iterations, two hops, as the one-hop pipe with a wavefront per column, with a wavefront per stream,
    and as a hop group of two; frame mode and the streaming emit.  Frames, hx, emitted hops, ring and overlap-add line: np.array_equal.  Only
    who carries a value changed, so not a bit may move.
2.  dn_stft and dn_istft at n_fft 512 / 1024 / 1536 on signals and spectra whose energy sits in one bin, against float64 numpy.fft
    (tests/handoff_cases.py: lane 0's bins, lane 32's, one ordinary pair), at the bars of tests/test_emu_windows.py.
The gpu tier (tests/test_gpu_handoff.py) runs the same single-bin cases and the chain against the per-column pipe on the device."""
import ctypes as C
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import dsp_cases as dc  # noqa: E402
import handoff_cases as hc  # noqa: E402
from audio_denoising_amd._lib import DN_GL_WAVE_PER_COLUMN, DN_GL_WAVE_PER_STREAM, DnLib, DspCfg  # noqa: E402
from oracle import dsp_np64, dsp_ref, pipeline_ref  # noqa: E402
from test_emu_kernels import _run_groups, _run_pipe, make_model  # noqa: E402
from test_emu_windows import geometry, wave_close  # noqa: E402

P = pipeline_ref.PARAMS_S
B, N_ITER = 3, 3


def build_bpermute():
    """the emulator library of tests/emu/emu.py, compiled with -DDN_HANDOFF_BPERMUTE"""
    out = emu.OUT.replace(".so", "_bpermute.so")
    srcs = sorted(glob.glob(os.path.join(emu.CSRC, "*.hip")))
    deps = srcs + glob.glob(os.path.join(emu.CSRC, "*.hpp")) + [os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "dn_cpx.hpp"),
                                                                os.path.join(emu.REPO, "include", "dn_denoise.h")]
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    opt = ["-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer"] if emu.ASAN else ["-O2"]
    cmd = ["g++", "-std=c++17"] + opt + ["-DDN_HANDOFF_BPERMUTE", "-fPIC", "-shared", "-pthread", "-x", "c++", "-I", emu.HERE] + srcs + ["-o", out]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def lib():
    return emu.load()


# ------------------------------------------------------------------ both hand-offs, bit for bit
G = {"signal": load_golden("stream_S.npz")["signal"]}

RUNS = {
    "pipe, wavefront per column": lambda lib, dsp, m, **kw: _run_pipe(lib, dsp, m, DN_GL_WAVE_PER_COLUMN, B, n_iter=N_ITER, g=G, **kw),
    "pipe, wavefront per stream": lambda lib, dsp, m, **kw: _run_pipe(lib, dsp, m, DN_GL_WAVE_PER_STREAM, B, n_iter=N_ITER, g=G, **kw),
    "hop group of two": lambda lib, dsp, m, **kw: _run_groups(lib, dsp, m, B, H=2, n_iter=N_ITER, g=G, **kw),
}


@pytest.fixture(scope="module")
def both(lib):
    """(results of every run through the library under test, through the -DDN_HANDOFF_BPERMUTE library), each computed once"""
    res = []
    for one in (lib, DnLib(build_bpermute())):
        fb = dsp_ref.melscale_fbanks(P.n_stft, P.n_mels, P.sample_rate).numpy()
        dsp = C.c_void_p()
        one.check(one.dn_dsp_create(C.byref(DspCfg(P.sample_rate, P.n_fft, P.hop, P.n_mels)), emu.ptr(emu.f32(fb)), None, None, C.byref(dsp)))
        m = make_model(one, 5)
        r = {}
        for name, run in RUNS.items():
            r[name, "frames"] = run(one, dsp, m, n_hops=2)                     # two frames, then hx
            r[name, "stream"] = run(one, dsp, m, n_hops=1, stream=True)        # two pushes and the drain: emitted hops, .., ring, overlap-add line, hx
        one.dn_model_destroy(m)
        one.dn_dsp_destroy(dsp)
        res.append(r)
    return res


@pytest.mark.parametrize("mode", ["frames", "stream"])
@pytest.mark.parametrize("name", list(RUNS))
def test_tile_hand_off_leaves_what_the_permute_hand_off_leaves(both, name, mode):
    new, old = both[0][name, mode], both[1][name, mode]
    assert len(new) == len(old) >= 3
    for i, (x, y) in enumerate(zip(new, old)):
        assert np.array_equal(x, y), (name, mode, i)
    assert sum(int(np.abs(np.asarray(x, np.float64)).max() > 0) for x in new) >= 2                 # (the comparison is of real output)


@pytest.mark.parametrize("mode", ["frames", "stream"])
def test_schedules_agree_under_the_tile_hand_off(both, mode):
    """the wavefront-per-stream chain (three hand-offs a direction through regions of the two tiles) against the per-column one (the wave's own
    tile): frames and hx bit for bit; the hop group emits the same frames"""
    new = both[0]
    col, stream, group = (new[n, mode] for n in RUNS)
    for i, (x, y) in enumerate(zip(col, stream)):
        assert np.array_equal(x, y), i
    if mode == "frames":
        for i, (x, y) in enumerate(zip(col, group)):
            assert np.array_equal(x, y), i


# ------------------------------------------------------------------ one bin at a time, against float64
@pytest.fixture(scope="module")
def plans(lib):
    made = {}
    for n_fft in hc.N_FFTS:
        p = geometry(n_fft)
        h = C.c_void_p()
        lib.check(lib.dn_dsp_create(C.byref(DspCfg(p.sample_rate, p.n_fft, p.hop, p.n_mels)), emu.ptr(emu.f32(dc.fbank(p))), None, None, C.byref(h)))
        made[n_fft] = h
    yield made
    for h in made.values():
        lib.dn_dsp_destroy(h)


@pytest.mark.parametrize("n_fft", hc.N_FFTS)
def test_stft_of_a_signal_in_one_bin(lib, plans, n_fft):
    hop, bad = n_fft // 2, []
    for k, who in hc.bins(n_fft):
        x = hc.signal(n_fft, k, 1)
        spec = np.zeros((1, 3, hop + 1, 2), np.float32)
        lib.check(lib.dn_stft(plans[n_fft], emu.ptr(x), emu.ptr(spec), 1, 0, None))
        ref = dsp_np64.stft(x, n_fft, hop)
        err = float(np.abs(dc.cplx(spec) - ref).max())
        assert np.abs(ref[:, k, 1]).max() > 0.1 * n_fft                                      # (the energy is where the case says)
        if err > hc.stft_bar(ref):
            bad.append(f"bin {k} ({who}): {err:.2e} > {hc.stft_bar(ref):.2e}; {dc.error_pattern(dc.cplx(spec), ref, n_fft)}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("n_fft", hc.N_FFTS)
def test_istft_of_a_spectrum_in_one_bin(lib, plans, n_fft):
    hop, bad = n_fft // 2, []
    for k, who in hc.bins(n_fft):
        z = hc.spectrum(n_fft, k, 1)
        wave = np.zeros((1, n_fft), np.float32)
        lib.check(lib.dn_istft(plans[n_fft], emu.ptr(dc.ri(z)), emu.ptr(wave), 1, None))
        ref = dsp_np64.istft(z, n_fft, hop)
        assert np.sqrt(np.mean(ref ** 2)) > 0.1                                              # (real output, not a spectrum that cancels)
        try:
            wave_close(wave, ref, n_fft, f"bin {k} ({who})")
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "\n".join(bad)
