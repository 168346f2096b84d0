"""The any-length Griffin-Lim cases on the CPU, from the float64 reference alone (no kernel runs here): the conditioning table of
tests/glg_cases.py derived again, the reference's own properties the kernel tests lean on, the DN_GL_INIT_NORMALIZE case's planted bins, and
the bindings of the new entry points (which fail on a library without them)."""
import numpy as np
import pytest

import dsp_cases as dc
import glg_cases as gc
from oracle import dsp_np64


@pytest.mark.parametrize("key", gc.all_keys(), ids=lambda k: "-".join(str(v) for v in k))
def test_seed_table_holds_the_first_well_conditioned_candidate(key):
    """Fails when an entry of SEED_K is not what the rule gives (a stale table, or a case added without deriving its entry)."""
    assert gc.first_well_conditioned_k(*key) == gc.SEED_K[key]


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_normalize_case_is_well_conditioned_and_plants_its_bins(n_fft):
    mag, spec, unit, bins = gc.normalize_case(n_fft)
    assert gc.is_well_conditioned(mag, unit, n_fft, "asym", 4, gc.MOMENTUM)
    assert spec[0, bins[0], 1] == 0 and abs(spec[0, bins[2], 1] - (3e3 + 4e3j)) == 0 and np.allclose(np.abs(unit), 1.0, atol=1e-6)


@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_reference_with_three_columns_is_the_hop_reference_and_zero_iterations_is_the_istft(n_fft):
    """What the kernel tests take for granted of oracle/dsp_np64.griffinlim: any T, hop (T - 1) samples, n_iter = 0 is istft(init * mag), and
    the three-column case is the array the hop tests compare with."""
    for T in (3, 4, 9):
        mag, init = gc.magnitudes(2, n_fft, T, 9000 + n_fft + T)
        w = dc.window("asym", n_fft)
        y0 = dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=0, window=w)
        assert y0.shape == (2, (n_fft // 2) * (T - 1))
        assert np.array_equal(y0, dsp_np64.istft(init.astype(np.complex128) * mag, n_fft, n_fft // 2, w))
        y2 = dsp_np64.griffinlim(mag, n_fft, n_fft // 2, init, n_iter=2, window=w)
        assert 0.3 < float(np.sqrt(np.mean(y2 ** 2))) < 3.0          # the waveform bars' scale max(1, RMS) is about the RMS itself


def test_library_declares_the_new_entry_points():
    """Fails on a library (or a binding) without the any-length Griffin-Lim: the symbols, the flags and the ABI version."""
    from audio_denoising_amd import _lib
    for s in ("dn_griffinlim_general_whole_max", "dn_griffinlim_general_workspace_bytes", "dn_griffinlim_general", "dn_griffinlim_draw_phases_general",
              "dn_server_mag"):
        assert s in _lib.SYMBOLS
    assert (_lib.DN_GLG_WHOLE, _lib.DN_GLG_STEPS, _lib.DN_GL_INIT_NORMALIZE, _lib.ABI_VERSION) == (gc.WHOLE, gc.STEPS, gc.NORMALIZE, 9)
    assert _lib.DN_GL_INIT_NORMALIZE & (_lib.DN_GLG_WHOLE | _lib.DN_GLG_STEPS | _lib.DN_PHASE_FROM_INPUT) == 0
