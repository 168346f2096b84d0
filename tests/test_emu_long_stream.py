"""The branchy part of the long-stream tests on the host emulation of the kernel sources (tests/test_emu_kernels.py has the tier's how and why):
32 hops of the conversation at n_fft 1024, B = 2 -- the windows cut around a silence's onset, around its end (a clipped burst follows it),
around the trio (consecutive frames that are silent, of peak 1 / 32767, and loud) and around the start of the sub-threshold stretch (frames
of peak 5e-7 and of peak exactly float32(1e-6): neither is normalised) -- through dn_stream_step in input-phase mode, n_iter 0.
Each window starts from the fixture's float64 state in front of it, rounded to fp32 (tests/golden/long_stream_1024.npz); the float64 reference
is recomputed from those same rounded values.  hx after every hop is held to R x E_k, R x E_near and the absolute bar, the emitted hops to
R x e_ref_wave per hop relative to the hop's own peak and absolute (tests/long_cases.py; tests/test_gpu_long_stream.py runs the whole signal).
(No hop of these windows is exactly zero in float64 -- a silent frame still emits what the model makes of hx -- so the exact comparison of zero
hops has nothing to do here; the first hop of a fresh stream is one, and test_a_fresh_stream_emits_an_exactly_zero_first_hop holds it.)
The trio then goes through a depth-4 pipe restored to the same state (dn_pipe_stream_set_state) with the device generator's phases and two
iterations -- parked chains, one slot a frame, the peak in the slot -- and must give the stream step's bits."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import long_cases as lc  # noqa: E402

N_FFT = 1024
WINDOWS = ("voiced->silence(1)", "silence(40)->burst", "silence(2)->onecount(1)->loud", "voiced->sub")


@pytest.fixture(scope="module")
def run():
    r = lc.Runner(emu.load())
    yield r
    r.close()


def excerpt(run, label, report=None):
    d = lc.load(N_FFT)
    i = [str(s) for s in d["win_label"]].index(label)
    f0 = int(d["win_f0"][i])
    ola, hx = d["win_ola64"][i].astype(np.float32), d["win_hx64"][i].astype(np.float32)
    y64, hx64 = lc.window64(N_FFT, f0, hx.astype(np.float64), ola.astype(np.float64))
    frames = range(f0, f0 + lc.WINDOW_HOPS)
    res = run.steps(run.plan(N_FFT), lc.signal32(N_FFT)[:lc.B_REF], f0, lc.WINDOW_HOPS, keep=set(frames), state=(ola, hx))
    fix = dict(cps=np.array(frames), hx64=hx64, e_ref=d["e_ref"])
    lc.check_hx(res, fix, "emu", f"emu {label!r}", report)
    lc.check_window(res["out"], y64, float(d["win_e_rel"][i]), float(d["win_e_abs"][i]), "emu", f"emu {label!r} at frame {f0}", report)
    return res, y64


@pytest.mark.parametrize("label", WINDOWS)
def test_stream_step_across_a_segment_boundary(run, label):
    res, y64 = excerpt(run, label)
    assert np.isfinite(res["out"]).all() and np.abs(y64).max(axis=2).min() > 0


@pytest.mark.parametrize("mode", ["depth4", "head_start"])
def test_pipe_carries_the_trio_through_its_slots(run, mode):
    d = lc.load(N_FFT)
    i = [str(s) for s in d["win_label"]].index(WINDOWS[2])
    f0 = int(d["win_f0"][i])
    state = (d["win_ola64"][i].astype(np.float32), d["win_hx64"][i].astype(np.float32))
    sig, plan = lc.signal32(N_FFT)[:lc.B_REF], run.plan(N_FFT)
    kw = dict(state=state, n_iter=2, flags=0, seed=2 ** 32 - f0 - 4, sid0=3)          # (seed + frame crosses 2**32 inside the window)
    modes = dict(depth4={"depth": 4}, head_start={"head": 2})
    depth = modes[mode].get("depth", 1)
    a = run.steps(plan, sig, f0, lc.WINDOW_HOPS, **kw)
    b = run.pipe_steps(plan, sig, f0, lc.WINDOW_HOPS, modes[mode], **kw)
    assert np.isfinite(a["out"]).all() and not b["out"][:depth].any()
    assert np.array_equal(b["out"][depth:].transpose(1, 0, 2), a["out"]), "the pipe's samples are not the stream step's"
    assert all(np.array_equal(a[k], b[k]) for k in ("ring", "ola", "hx"))


def test_a_fresh_stream_emits_an_exactly_zero_first_hop(run):
    sig = lc.signal32(N_FFT)[:lc.B_REF]
    res = run.steps(run.plan(N_FFT), sig, 0, 2)
    assert lc.check_zero_hops(res["out"][:, :1], np.zeros((lc.B_REF, 1, N_FFT // 2)), "first hop") == lc.B_REF and res["out"][:, 1].any()


def test_the_excerpts_hold_the_frames_they_are_cut_for():
    p = lc.geometry(N_FFT)
    d = lc.load(N_FFT)
    sig = lc.signal32(N_FFT)[:lc.B_REF]
    peaks = {}
    for label in WINDOWS:
        f0 = int(d["win_f0"][[str(s) for s in d["win_label"]].index(label)])
        peaks[label] = np.stack([np.abs(lc.frame_of(sig, p, f)).max(axis=1) for f in range(f0, f0 + lc.WINDOW_HOPS)])
    one = np.float32(1) / np.float32(32767)
    assert (peaks[WINDOWS[1]][:2] == 0).all() and (peaks[WINDOWS[1]][3:] == 1.0).all(), "silent frames (peak stays 1), then the clipped burst"
    trio = peaks[WINDOWS[2]]
    assert any((trio[k] == 0).all() and (trio[k + 1] == one).all() and (trio[k + 2] > 0.5).all() for k in range(lc.WINDOW_HOPS - 2))
    assert (peaks[WINDOWS[0]] > 0).all()            # half a frame of silence: no frame is silent
    sub = peaks[WINDOWS[3]]
    assert (sub[4:6] == np.float32(lc.SUB_LEVEL)).all() and (sub[6:] == lc.SUB_EDGE).all(), "below the threshold, then exactly on it"
