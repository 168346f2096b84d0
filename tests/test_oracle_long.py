"""The long-stream signal and its fixtures, from the references alone (no GPU, no emulator, no built library): tests/long_cases.py builds the
"conversation", oracle/make_long_golden.py wrote tests/golden/long_stream_<n_fft>.npz.

  * the generated int16 signal is the one the fixture was computed on (sha256);
  * regenerating the first 48 hops reproduces the fixture's first checkpoints exactly, and its fp32 yardstick;
  * the conditioning the R x e_ref bounds rest on: the fp32 oracle's hx error does not grow over the run;
  * the segment table is what the signal holds;
  * the windows' float64 waveforms follow from the stored state, and the fp32 oracle's own int16 samples differ from the float64
    truncation in under 1 % of every window (the cap of the GPU tier's int16 comparison is a condition on the input, checked here)."""
import numpy as np
import pytest

import long_cases as lc

PREFIX_HOPS = 48


@pytest.fixture(scope="module")
def prefix():
    cache = {}

    def get(n_fft):
        if n_fft not in cache:
            cache[n_fft] = lc.chains(n_fft, PREFIX_HOPS)
        return cache[n_fft]
    return get


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_signal_is_the_fixtures(n_fft):
    d = lc.load(n_fft)
    assert str(d["sha256"]) == lc.sha256(n_fft), "this numpy draws another signal than the fixture was computed on: regenerate the fixtures"
    assert int(d["hops"]) == lc.HOPS[n_fft] and d["cps"].tolist() == list(lc.checkpoints(n_fft))
    assert d["win_f0"].tolist() == [f0 for _, f0 in lc.windows(n_fft)] and 6 <= d["win_f0"].size <= 9
    assert lc.signal16(n_fft).shape == (lc.B_GPU, (lc.HOPS[n_fft] + 1) * (n_fft // 2))


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_prefix_reproduces_the_first_checkpoints(n_fft, prefix):
    d = lc.load(n_fft)
    hx64, hx32 = prefix(n_fft)
    early = [i for i, c in enumerate(d["cps"]) if c < PREFIX_HOPS]
    assert len(early) >= 4
    for i in early:
        assert np.array_equal(hx64[d["cps"][i]], d["hx64"][i]), f"checkpoint {d['cps'][i]}"
    e = np.stack([lc.hx_error(hx32[f], hx64[f]) for f in range(PREFIX_HOPS)])
    # the fp32 oracle's error depends on the torch build and its thread count, within rounding's own scatter
    assert e.max() <= 2.0 * d["e_ref"][:PREFIX_HOPS].max() and d["e_ref"][:PREFIX_HOPS].max() <= 2.0 * e.max()


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_reference_is_well_conditioned_over_the_run(n_fft):
    d = lc.load(n_fft)
    e = d["e_ref"].max(axis=1)
    run = lc.running_max(e)
    F = lc.HOPS[n_fft]
    print(f"n_fft {n_fft}: e_ref max over the first {lc.PREFIX} hops {run[lc.PREFIX - 1]:.3e}, over {F} hops {run[-1]:.3e} "
          f"(x{run[-1] / run[lc.PREFIX - 1]:.2f}); second half / first half {e[F // 2:].max() / e[:F // 2].max():.2f}; last hop {e[-1]:.3e}")
    assert run[-1] <= lc.CONDITIONING * run[lc.PREFIX - 1]
    assert np.abs(d["hx64"]).max() <= 1.0 and np.abs(d["hx64"]).max() > 0.99, "voiced speech saturates the state"


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_segment_table_is_what_the_signal_holds(n_fft):
    p = lc.geometry(n_fft)
    H, F = p.hop, lc.HOPS[n_fft]
    s16, s32 = lc.signal16(n_fft)[:3], lc.signal32(n_fft)[:3]              # (the shifted copies hold the segments elsewhere)
    hops = lambda x, s, n: x[:, s * H:(s + n) * H]  # noqa: E731
    segs = lc.segments(n_fft)
    assert [s for _, s, _, _ in segs] == list(np.cumsum([0] + [n for _, _, n, _ in segs])[:-1]) and sum(n for _, _, n, _ in segs) == F + 1
    kinds = {k for k, _, _, _ in segs}
    assert kinds == {"voiced", "unvoiced", "tone_bin", "tone_off", "dc", "silence", "onecount", "sub", "burst", "loud"}
    assert {n for k, _, n, _ in segs if k == "silence"} >= {1, n_fft // H, 40}
    zero_frames = 0
    for i, (kind, s, n, level) in enumerate(segs):
        a16, a32 = hops(s16, s, n), hops(s32, s, n)
        if kind == "silence":
            assert not a16.any() and not a32.any()
            zero_frames += max(n - 1, 0)
        elif kind == "onecount":
            assert (np.abs(a16).reshape(3, n, H).max(axis=2) == 1).all() and (np.abs(a32).max(axis=1) == np.float32(1) / np.float32(32767)).all()
        elif kind == "sub":
            half = a32.shape[1] // 2
            assert not a16.any() and (np.abs(a32[:, :half]) == np.float32(lc.SUB_LEVEL)).all() and (np.abs(a32[:, half:]) == lc.SUB_EDGE).all()
            assert lc.SUB_LEVEL < 1e-6 and not lc.SUB_EDGE > np.float32(1e-6) and not float(lc.SUB_EDGE) > 1e-6
        elif kind == "burst":
            assert segs[i - 1][0] == "silence" and ((np.abs(a16) == 32767).sum(axis=1) > H).all() and np.abs(a16[:, :H]).max() == 32767
        else:
            assert (np.abs(a16).reshape(3, n, H).max(axis=2) >= 1).all(), (kind, s)
    assert zero_frames >= 40
    # the trio: consecutive frames that are silent (peak stays 1), of peak 1 / 32767, and loud
    s = next(s for k, s, n, _ in segs if k == "onecount" and n == 1)
    peaks = [np.abs(lc.frame_of(s32, p, f)).max(axis=1) for f in (s - 2, s - 1, s)]
    assert (peaks[0] == 0).all() and (peaks[1] == np.float32(1) / np.float32(32767)).all() and (peaks[2] > 0.5).all()
    # both halves of the run hold every kind the fp32 yardstick is sensitive to, and checkpoints surround every special segment
    for kind in ("tone_bin", "tone_off", "silence", "onecount"):
        starts = [s for k, s, _, _ in segs if k == kind]
        assert min(starts) < F // 2 <= max(starts), kind
    cps = set(lc.checkpoints(n_fft))
    assert all({s - 1, s, s + n} & set(range(F)) <= cps for _, s, n, _ in lc.special_segments(n_fft))
    assert all(f0 >= 2 and f0 + lc.WINDOW_HOPS <= F for _, f0 in lc.windows(n_fft))


@pytest.mark.parametrize("n_fft", lc.N_FFTS)
def test_windows_follow_from_the_stored_state_and_keep_the_int16_cap(n_fft, prefix):
    d = lc.load(n_fft)
    p = lc.geometry(n_fft)
    for i, f0 in enumerate(d["win_f0"]):
        y64, hxs = lc.window64(n_fft, int(f0), d["win_hx64"][i], d["win_ola64"][i])
        assert y64.shape == (lc.B_REF, lc.WINDOW_HOPS, p.hop)
        hit = [j for j, c in enumerate(d["cps"]) if f0 <= c < f0 + lc.WINDOW_HOPS]
        for j in hit:                                                 # the restart lands on the chain's own checkpoints
            assert np.array_equal(hxs[d["cps"][j] - f0], d["hx64"][j])
        frac = float((d["win_s16_ref32"][i] != lc.s16_of(y64)).mean())
        print(f"n_fft {n_fft} window {str(d['win_label'][i])!r} at frame {f0}: e_ref_wave rel {d['win_e_rel'][i]:.3e} abs {d['win_e_abs'][i]:.3e}, "
              f"int16 of the fp32 oracle differs in {frac:.3%}")
        assert frac < lc.S16_CAP, "choose another window: the cap is a condition on the input"
        assert np.isfinite(d["win_e_rel"][i]) and 0 < d["win_e_abs"][i] < 1e-4
    # the first window's fp32 side again, from the regenerated prefix
    f0 = int(d["win_f0"][0])
    assert f0 + lc.WINDOW_HOPS <= PREFIX_HOPS
    hx64, hx32 = prefix(n_fft)
    assert np.array_equal(lc.ola_in_front_of(lc.run64(n_fft), n_fft, f0, hx64, np.float64), d["win_ola64"][0])
    y32, _ = lc.window32(n_fft, f0, hx32[f0 - 1], lc.ola_in_front_of(lc.run32(n_fft), n_fft, f0, hx32, np.float32))
    y64, _ = lc.window64(n_fft, f0, d["win_hx64"][0], d["win_ola64"][0])
    rel, err = lc.hop_errors(y32, y64)
    assert rel.max() <= 2.0 * d["win_e_rel"][0] and err.max() <= 2.0 * d["win_e_abs"][0]
