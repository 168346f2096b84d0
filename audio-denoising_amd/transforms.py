"""Equivalents of the torchaudio transforms the reference constructs around the model
(app3.py:135-153, server.py:173-176), with the constructor keywords used at those sites:

    Spectrogram(power=None, n_fft, win_length, hop_length, window_fn)         app3.py:135-139
    MelScale(n_mels, n_stft, sample_rate)                                     app3.py:140-143
    InverseMelScale(n_mels, n_stft, sample_rate)                              app3.py:145-148
    GriffinLim(n_fft, win_length, hop_length, window_fn, power=1.0)           app3.py:149-153
    InverseSpectrogram(n_fft, win_length, hop_length)                         server.py:174
    Resample(orig_freq, new_freq)                                             utils.py:48-49 (app.py:181: librosa.resample)

Each ``forward`` is one HIP kernel launch through the C ABI; inputs must be float32 (complex64 for
InverseSpectrogram) CUDA tensors shaped as the reference shapes them.  Internally every spectral
tensor is stored [stream][column][bin]; the (.., bins, columns) tensors the reference's layout
calls for are returned as transposed views, which is also what MelScale returns in torchaudio.
No CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref

import torch
from torch import nn

from . import _lib
from ._glue import PCM, check_tensor, launch

_N_FFTS = (512, 1024, 1536)   # the one-wave FFT kernels: 256 = 4*4*4*4, 512 = 8*8*8 and 768 = 4*4*4*12 complex points (hop = n_fft/2)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """HTK triangular filterbank, norm=None, in float32 with the operation order of
    torchaudio.functional.melscale_fbanks.  (n_freqs, n_mels).
    Construction-time host code: runs once per transform object."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_min = 2595.0 * math.log10(1.0 + (f_min / 700.0))
    m_max = 2595.0 * math.log10(1.0 + (f_max / 700.0))
    m_pts = torch.linspace(m_min, m_max, n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down_slopes = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up_slopes = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1), torch.min(down_slopes, up_slopes))


class DspPlan:
    """Owns one ``dn_dsp*`` (twiddles, window, banded filterbank, pseudo-inverse) on one device."""

    def __init__(self, device: torch.device, sample_rate: int, n_fft: int, hop: int, n_mels: int = 0,
                 fb: torch.Tensor | None = None, window: torch.Tensor | None = None, pinv: torch.Tensor | None = None):
        if not torch.device(device).type == "cuda":
            raise RuntimeError("DSP plans live on a 'cuda' device; there is no CPU path in this package")
        self.lib = _lib.get_lib()
        self.device = torch.device(device)
        self.sample_rate, self.n_fft, self.hop, self.n_mels = sample_rate, n_fft, hop, n_mels
        self.n_stft = n_fft // 2 + 1
        cfg = _lib.DspCfg(int(sample_rate), int(n_fft), int(hop), int(n_mels))
        keep = []

        def host(t, shape):
            if t is None:
                return None
            t = t.detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"expected shape {shape}, got {tuple(t.shape)}")
            keep.append(t)
            return C.c_void_p(t.data_ptr())

        handle = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        with torch.cuda.device(idx):
            self.lib.check(self.lib.dn_dsp_create(C.byref(cfg), host(fb, (self.n_stft, n_mels)), host(pinv, (self.n_stft, n_mels)),
                                                  host(window, (n_fft,)), C.byref(handle)))
        self.handle = handle
        self._fin = weakref.finalize(self, self.lib.dn_dsp_destroy, handle)

    def tables(self):
        fb = torch.empty(self.n_stft, max(self.n_mels, 1))
        pinv = torch.empty(self.n_stft, max(self.n_mels, 1))
        win = torch.empty(self.n_fft)
        self.lib.check(self.lib.dn_dsp_get_tables(self.handle, fb.data_ptr(), pinv.data_ptr(), win.data_ptr()))
        return fb[:, :self.n_mels], pinv[:, :self.n_mels], win

    def workspace_bytes(self, batch: int, flags: int = 0) -> int:
        """Scratch of a fused call with ``flags`` (dn_workspace_bytes_ex: input-phase mode adds the phasor rows)."""
        return int(self.lib.dn_workspace_bytes_ex(self.handle, batch, flags))


def _require(t: torch.Tensor, dtypes, what: str):
    """the argument check of a transform: a CUDA tensor (else RuntimeError) of one of ``dtypes`` (else TypeError), any shape and strides"""
    check_tensor(t, what, None, dtypes, "cuda", RuntimeError, TypeError, contiguous=False)


class _PlanModule(nn.Module):
    """Lazily builds one DspPlan per device the module is called on."""

    def __init__(self):
        super().__init__()
        self._plans = {}

    def _plan_args(self):  # -> dict for DspPlan
        raise NotImplementedError

    def plan(self, device: torch.device) -> DspPlan:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        p = self._plans.get(idx)
        if p is None:
            p = DspPlan(torch.device("cuda", idx), **self._plan_args())
            self._plans[idx] = p
        return p

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        import copy
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_plans" else copy.deepcopy(v, memo)
        return new


def _check_fft_args(n_fft, win_length, hop_length):
    win_length = n_fft if win_length is None else win_length
    hop_length = win_length // 2 if hop_length is None else hop_length
    if n_fft not in _N_FFTS or win_length != n_fft or hop_length != n_fft // 2:
        raise NotImplementedError(f"the FFT kernels are built for n_fft=win_length in {_N_FFTS} with hop_length=n_fft/2; "
                                  f"got n_fft={n_fft}, win_length={win_length}, hop_length={hop_length}")
    return n_fft, win_length, hop_length


class Spectrogram(_PlanModule):
    """Spectrogram(power=None|1|2, center=True, pad_mode='reflect', onesided=True, normalized=False):
    (.., L) -> (.., n_fft/2+1, 1 + L // hop) for any L > n_fft/2 (dn_stft_general); a frame of exactly n_fft samples is the hop path's 3-column
    dn_stft.  app3.py:135-139,191."""

    def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, power=2.0,
                 normalized=False, wkwargs=None, center=True, pad_mode="reflect", onesided=True):
        super().__init__()
        self.n_fft, self.win_length, self.hop_length = _check_fft_args(n_fft, win_length, hop_length)
        if pad != 0 or normalized or not center or pad_mode != "reflect" or not onesided:
            raise NotImplementedError("only pad=0, normalized=False, center=True, pad_mode='reflect', onesided=True")
        self.power = power
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)

    def _plan_args(self):
        return dict(sample_rate=0, n_fft=self.n_fft, hop=self.hop_length, n_mels=0, window=self.window)

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        _require(waveform, (torch.float32,), "Spectrogram")
        L = waveform.shape[-1]
        if L <= self.n_fft // 2:
            raise RuntimeError(f"reflect padding needs more than n_fft/2 = {self.n_fft // 2} samples (as torch.stft); got {L}")
        T = 1 + L // self.hop_length
        lead = waveform.shape[:-1]
        x = waveform.reshape(-1, L).contiguous()
        B = x.shape[0]
        plan = self.plan(x.device)
        spec = torch.empty(B, T, plan.n_stft, 2, dtype=torch.float32, device=x.device)
        if L == self.n_fft:
            launch(plan.lib, x.device, plan.lib.dn_stft, plan.handle, x.data_ptr(), spec.data_ptr(), B, 0)
        else:
            launch(plan.lib, x.device, plan.lib.dn_stft_general, plan.handle, x.data_ptr(), spec.data_ptr(), None, B, L)
        out = torch.view_as_complex(spec).reshape(lead + (T, plan.n_stft)).transpose(-1, -2)
        if self.power is None:
            return out
        return out.abs() if self.power == 1.0 else out.abs().pow(self.power)


def _rows_layout(t: torch.Tensor) -> torch.Tensor:
    """(.., R, T) logical -> contiguous [.., T, R] storage (free when t is already a transposed view)."""
    return t.transpose(-1, -2).contiguous()


class MelScale(_PlanModule):
    """MelScale(n_mels, sample_rate, f_min=0, f_max=sr//2, n_stft, norm=None, mel_scale='htk'):
    (.., n_stft, T) -> (.., n_mels, T).  app3.py:140-143,193."""

    def __init__(self, n_mels=128, sample_rate=16000, f_min=0.0, f_max=None, n_stft=201, norm=None, mel_scale="htk"):
        super().__init__()
        if norm is not None or mel_scale != "htk":
            raise NotImplementedError("only norm=None, mel_scale='htk' (what the reference uses)")
        if 2 * (n_stft - 1) not in _N_FFTS:
            raise NotImplementedError(f"n_stft must be one of {[n // 2 + 1 for n in _N_FFTS]}")
        self.n_mels, self.sample_rate, self.n_stft = n_mels, sample_rate, n_stft
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        self.register_buffer("fb", melscale_fbanks(n_stft, self.f_min, self.f_max, n_mels, sample_rate))

    def _plan_args(self):
        n_fft = 2 * (self.n_stft - 1)
        return dict(sample_rate=self.sample_rate, n_fft=n_fft, hop=n_fft // 2, n_mels=self.n_mels, fb=self.fb)

    def forward(self, specgram: torch.Tensor) -> torch.Tensor:
        _require(specgram, (torch.float32,), "MelScale")
        if specgram.shape[-2] != self.n_stft:
            raise RuntimeError(f"expected {self.n_stft} frequency bins, got {specgram.shape[-2]}")
        rows = _rows_layout(specgram)                      # [.., T, K]
        lead, T = rows.shape[:-2], rows.shape[-2]
        B = rows.numel() // (T * self.n_stft)
        plan = self.plan(rows.device)
        mel = torch.empty(lead + (T, self.n_mels), dtype=torch.float32, device=rows.device)
        launch(plan.lib, rows.device, plan.lib.dn_mel_scale, plan.handle, rows.data_ptr(), mel.data_ptr(), B, T)
        return mel.transpose(-1, -2)


class InverseMelScale(_PlanModule):
    """InverseMelScale(n_stft, n_mels, sample_rate, f_min, f_max, norm=None, mel_scale='htk', driver='gels'):
    (.., n_mels, T) -> (.., n_stft, T) = relu(min-norm least squares).  app3.py:145-148,210."""

    def __init__(self, n_stft, n_mels=128, sample_rate=16000, f_min=0.0, f_max=None, norm=None, mel_scale="htk", driver="gels"):
        super().__init__()
        if norm is not None or mel_scale != "htk":
            raise NotImplementedError("only norm=None, mel_scale='htk' (what the reference uses)")
        if driver not in ("gels", "gelsy", "gelsd", "gelss"):
            raise ValueError(f'driver must be one of ["gels", "gelsy", "gelsd", "gelss"]. Found {driver}.')
        if 2 * (n_stft - 1) not in _N_FFTS:
            raise NotImplementedError(f"n_stft must be one of {[n // 2 + 1 for n in _N_FFTS]}")
        self.n_mels, self.sample_rate, self.n_stft, self.driver = n_mels, sample_rate, n_stft, driver
        self.f_min = f_min
        self.f_max = f_max if f_max is not None else float(sample_rate // 2)
        fb = melscale_fbanks(n_stft, self.f_min, self.f_max, n_mels, sample_rate)
        self.register_buffer("fb", fb)

    def _plan_args(self):
        n_fft = 2 * (self.n_stft - 1)
        return dict(sample_rate=self.sample_rate, n_fft=n_fft, hop=n_fft // 2, n_mels=self.n_mels, fb=self.fb)

    def forward(self, melspec: torch.Tensor) -> torch.Tensor:
        _require(melspec, (torch.float32,), "InverseMelScale")
        if melspec.shape[-2] != self.n_mels:
            raise ValueError(f"Expected an input with {self.n_mels} mel bins. Found: {melspec.shape[-2]}")
        rows = _rows_layout(melspec)                       # [.., T, M]
        lead, T = rows.shape[:-2], rows.shape[-2]
        B = rows.numel() // (T * self.n_mels)
        plan = self.plan(rows.device)
        lin = torch.empty(lead + (T, self.n_stft), dtype=torch.float32, device=rows.device)
        launch(plan.lib, rows.device, plan.lib.dn_invmel, plan.handle, rows.data_ptr(), lin.data_ptr(), B, T)
        return lin.transpose(-1, -2)


class GriffinLim(_PlanModule):
    """GriffinLim(n_fft, n_iter=32, win_length, hop_length, window_fn, power=2.0, momentum=0.99, length=None,
    rand_init=True): (.., n_fft/2+1, T) magnitude**power -> (.., hop*(T-1)) for any T >= 3.  T == 3 (one n_fft-sample frame) is the hop path's
    dn_griffinlim, app3.py:149-153,213; any other T runs dn_griffinlim_general (every iteration on chip up to
    dn_griffinlim_general_whole_max columns, two launches an iteration beyond; the same samples either way).

    ``rand_init=True`` draws the initial phases on the device from a counter-based generator whose
    seed comes from torch's global RNG (so ``torch.manual_seed`` makes runs repeatable); pass
    ``init_angles`` (complex64, same shape as the input) to ``forward`` to inject them instead --
    that is how parity with the reference's ``torch.rand`` draw is tested."""

    def __init__(self, n_fft=400, n_iter=32, win_length=None, hop_length=None, window_fn=torch.hann_window, power=2.0,
                 wkwargs=None, momentum=0.99, length=None, rand_init=True):
        super().__init__()
        if not (0 <= momentum < 1):
            raise ValueError("momentum must be in the range [0, 1). Found: {}".format(momentum))
        self.n_fft, self.win_length, self.hop_length = _check_fft_args(n_fft, win_length, hop_length)
        if length is not None and length != n_fft:
            raise NotImplementedError("length=None (T columns -> hop*(T-1) samples) is what the kernels produce")
        self.length = length
        self.n_iter, self.power, self.momentum, self.rand_init = n_iter, power, momentum, rand_init
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)

    def _plan_args(self):
        return dict(sample_rate=0, n_fft=self.n_fft, hop=self.hop_length, n_mels=0, window=self.window)

    def forward(self, specgram: torch.Tensor, init_angles: torch.Tensor | None = None) -> torch.Tensor:
        _require(specgram, (torch.float32,), "GriffinLim")
        K = self.n_fft // 2 + 1
        T = specgram.shape[-1]
        if self.length is not None and T != 3:
            raise NotImplementedError("length=None (T columns -> hop*(T-1) samples) is what the kernels produce")
        if specgram.shape[-2] != K or T < 3:
            raise RuntimeError(f"expected (.., {K}, T) with T >= 3 columns (reflect padding needs hop*(T-1) > n_fft/2); got {tuple(specgram.shape)}")
        if self.power != 1.0:
            specgram = specgram.pow(1.0 / self.power)
        rows = _rows_layout(specgram)                      # [.., T, K]
        lead = rows.shape[:-2]
        B = rows.numel() // (T * K)
        plan = self.plan(rows.device)
        ia_ptr, seed = None, 0
        if init_angles is not None:
            _require(init_angles, (torch.complex64,), "GriffinLim init_angles")
            if init_angles.shape != specgram.shape:
                raise ValueError("init_angles must have the shape of the spectrogram")
            ia = torch.view_as_real(_rows_layout(init_angles).resolve_conj()).contiguous()
            ia_ptr = ia.data_ptr()
        elif self.rand_init:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        else:   # angles = 1 + 1j?  torchaudio uses torch.full(.., 1, dtype=complex) = 1 + 0j
            ia = torch.zeros(rows.shape + (2,), dtype=torch.float32, device=rows.device)
            ia[..., 0] = 1.0
            ia_ptr = ia.data_ptr()
        wave = torch.empty(lead + (self.hop_length * (T - 1),), dtype=torch.float32, device=rows.device)
        if T == 3:
            launch(plan.lib, rows.device, plan.lib.dn_griffinlim, plan.handle, rows.data_ptr(), ia_ptr, seed, 0, None, wave.data_ptr(), B,
                   int(self.n_iter), float(self.momentum))
        else:
            ws = torch.empty(max(1, int(plan.lib.dn_griffinlim_general_workspace_bytes(plan.handle, B, T))), dtype=torch.uint8, device=rows.device)
            launch(plan.lib, rows.device, plan.lib.dn_griffinlim_general, plan.handle, rows.data_ptr(), ia_ptr, seed, 0, wave.data_ptr(), ws.data_ptr(),
                   B, T, int(self.n_iter), float(self.momentum), 0)
        return wave


class InverseSpectrogram(_PlanModule):
    """InverseSpectrogram(n_fft, win_length, hop_length): complex (.., n_fft/2+1, T) -> (.., hop*(T-1)) for any T >= 2 (dn_istft_general; 3 columns
    are the hop path's dn_istft).  server.py:174,216."""

    def __init__(self, n_fft=400, win_length=None, hop_length=None, pad=0, window_fn=torch.hann_window, normalized=False,
                 wkwargs=None, center=True, pad_mode="reflect", onesided=True):
        super().__init__()
        self.n_fft, self.win_length, self.hop_length = _check_fft_args(n_fft, win_length, hop_length)
        if pad != 0 or normalized or not center or not onesided:
            raise NotImplementedError("only pad=0, normalized=False, center=True, onesided=True")
        window = window_fn(self.win_length) if wkwargs is None else window_fn(self.win_length, **wkwargs)
        self.register_buffer("window", window)

    def _plan_args(self):
        return dict(sample_rate=0, n_fft=self.n_fft, hop=self.hop_length, n_mels=0, window=self.window)

    def forward(self, spectrogram: torch.Tensor, length=None) -> torch.Tensor:
        _require(spectrogram, (torch.complex64,), "InverseSpectrogram")
        K = self.n_fft // 2 + 1
        T = spectrogram.shape[-1]
        if length is not None and (length != self.n_fft or T != 3):
            raise NotImplementedError("length=None (T columns -> hop*(T-1) samples) is what the kernels produce")
        if spectrogram.shape[-2] != K or T < 2:
            raise RuntimeError(f"expected (.., {K}, T) with T >= 2 columns; got {tuple(spectrogram.shape)}")
        rows = torch.view_as_real(_rows_layout(spectrogram).resolve_conj()).contiguous()   # [.., T, K, 2]
        lead = rows.shape[:-3]
        B = rows.numel() // (T * K * 2)
        plan = self.plan(rows.device)
        wave = torch.empty(lead + (self.hop_length * (T - 1),), dtype=torch.float32, device=rows.device)
        if T == 3:
            launch(plan.lib, rows.device, plan.lib.dn_istft, plan.handle, rows.data_ptr(), wave.data_ptr(), B)
        else:
            launch(plan.lib, rows.device, plan.lib.dn_istft_general, plan.handle, rows.data_ptr(), wave.data_ptr(), B, T)
        return wave


class Resample(nn.Module):
    """Resample(orig_freq, new_freq, resampling_method, lowpass_filter_width, rolloff, beta, *, dtype): (.., L) -> (.., ceil(new L / orig)) with
    the rates reduced by their gcd, float32 or int16 PCM on the device, the dtype of the input (dn_resample: one launch, polyphase sinc filter).
    utils.py:48-49 (``Resample(44100, SR)``, ``Resample(SR, 44100)``), app.py:181 (``librosa.resample``).

    ``sinc_interp_hann`` is the table the library builds itself in double; ``sinc_interp_kaiser`` (``beta`` default 14.769656459379492) is built
    here with ``torch.i0`` in float64 and handed in.  Either way the table is rounded to float32 once; ``dtype`` (torchaudio's precision of the
    precomputed kernel) is accepted and changes nothing.  int16 is read as x / 32767 and written clip, * 32767, truncate, as everywhere in this
    package.  Rows that are contiguous in themselves go through their stride (a slice of a wider batch is not copied).  Equal rates return the input
    itself, as torchaudio does.  No CPU path."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = "sinc_interp_hann", lowpass_filter_width: int = 6,
                 rolloff: float = 0.99, beta: float | None = None, *, dtype: torch.dtype | None = None):
        super().__init__()
        if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
            raise ValueError(f"Invalid resampling method: {resampling_method}")
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
            raise ValueError("Frequencies must be of integer type to ensure quality resampling computation.")
        if dtype is not None and not dtype.is_floating_point:
            raise TypeError(f"dtype must be a floating point type, got {dtype}")
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.resampling_method, self.lowpass_filter_width, self.rolloff, self.beta = resampling_method, int(lowpass_filter_width), float(rolloff), beta
        if self.orig_freq < 1 or self.new_freq < 1 or self.lowpass_filter_width < 1 or not 0.0 < self.rolloff <= 1.0:
            raise ValueError("rates must be positive, lowpass_filter_width at least 1 and rolloff in (0, 1]")
        # the geometry, as torchaudio's _get_sinc_resample_kernel has it (the library computes the same and is asked when a handle is built)
        g = math.gcd(self.orig_freq, self.new_freq)
        self.o, self.n = self.orig_freq // g, self.new_freq // g
        self.width = math.ceil(self.lowpass_filter_width * self.o / (min(self.o, self.n) * self.rolloff))
        self.taps = 2 * self.width + self.o
        self.delay_blocks = -(-self.width // self.o)
        if self.orig_freq != self.new_freq and (max(self.o, self.n) > 1024 or self.n * self.taps > 2 ** 19):
            raise NotImplementedError(f"the kernels take reduced rates up to 1024 and tables of up to 2^19 floats; {self.orig_freq} -> {self.new_freq} is "
                                      f"{self.o} : {self.n} with {self.n} x {self.taps} floats")
        self._handles = {}

    @property
    def lib(self):
        """the product's library, loaded on first use (constructing the transform needs neither the library nor a device)"""
        return _lib.get_lib()

    def _create(self, table):
        h = C.c_void_p()
        cfg = _lib.ResampleCfg(self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff)
        self.lib.check(self.lib.dn_resample_create(C.byref(cfg), None if table is None else C.c_void_p(table.data_ptr()), C.byref(h)))
        v = [C.c_int32() for _ in range(5)]
        self.lib.check(self.lib.dn_resample_geometry(h, *[C.byref(x) for x in v]))
        if tuple(x.value for x in v) != (self.o, self.n, self.width, self.taps, self.delay_blocks):
            self.lib.dn_resample_destroy(h)
            raise RuntimeError("the library's resampler geometry differs from this module's")
        return h

    def _kaiser_table(self) -> torch.Tensor:
        """torchaudio's sinc_interp_kaiser kernel, (n, taps), in float64, rounded once"""
        beta = 14.769656459379492 if self.beta is None else float(self.beta)
        o, n, lpw = self.o, self.n, self.lowpass_filter_width
        base = min(o, n) * self.rolloff
        idx = torch.arange(-self.width, self.width + o, dtype=torch.float64)[None, :] / o
        t = (torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx) * base
        t = t.clamp(-lpw, lpw)
        window = torch.i0(beta * torch.sqrt(1 - (t / lpw) ** 2)) / torch.i0(torch.tensor(beta, dtype=torch.float64))
        t = t * math.pi
        sinc = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
        return (sinc * (window * (base / o))).to(torch.float32).contiguous()

    def handle(self, device: torch.device):
        """the dn_resampler of ``device`` (built on first use)"""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = self._handles.get(idx)
        if h is None:
            table = self._kaiser_table() if self.resampling_method == "sinc_interp_kaiser" else None
            with torch.cuda.device(idx):
                h = self._create(table)
            self._handles[idx] = h
            weakref.finalize(self, self.lib.dn_resample_destroy, h)
        return h

    def kernel(self, device: torch.device) -> torch.Tensor:
        """the float32 table (n, taps) as the library holds it"""
        k = torch.empty(self.n, self.taps)
        self.lib.check(self.lib.dn_resample_get_kernel(self.handle(torch.device(device)), k.data_ptr()))
        return k

    def out_len(self, length: int) -> int:
        return -(-self.n * int(length) // self.o)

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        import copy
        for k, v in self.__dict__.items():
            new.__dict__[k] = {} if k == "_handles" else copy.deepcopy(v, memo)
        return new

    @staticmethod
    def _rows(t: torch.Tensor):
        """(.., L) -> (a 2-D tensor whose rows are contiguous in themselves, its row stride): a view wherever the strides allow it"""
        L = t.shape[-1]
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() > 2:
            t = t.reshape(-1, L)          # (a view when the leading dimensions fold, else a copy)
        if L > 1 and t.stride(1) != 1:
            t = t.contiguous()
        stride = t.stride(0) if t.shape[0] > 1 else L
        if stride < L:                    # expanded or overlapping rows
            t = t.contiguous()
            stride = L
        return t, stride

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        _require(waveform, PCM, "Resample")
        if self.orig_freq == self.new_freq:
            return waveform
        L = waveform.shape[-1]
        lead = waveform.shape[:-1]
        Ly = self.out_len(L)
        out = torch.empty(lead + (Ly,), dtype=waveform.dtype, device=waveform.device)
        if L == 0 or out.numel() == 0:
            return out
        x, xs = self._rows(waveform)
        s16 = int(waveform.dtype == torch.int16)
        launch(self.lib, waveform.device, self.lib.dn_resample, self.handle(waveform.device), x.data_ptr(), s16, out.data_ptr(), s16, x.shape[0], L, xs, Ly)
        return out


class ResampleStream:
    """``batch`` live streams through one ``Resample`` (dn_resample_push).  ``push(chunk)`` takes (batch, k o) samples, whole blocks of
    ``resample.o``, float32 or int16 on the device, and returns the (batch, k n) samples they emit (k = 0: an empty tensor, nothing changes).
    The outputs lag the input by ``delay`` output samples (D n, D = ceil(width / o) blocks): the concatenation of everything pushed and then ``flush()`` -- D blocks of zeros --, from sample
    ``delay`` on, is ``resample(whole signal)`` bit for bit, however the signal was cut into pushes.  The first ``delay`` samples of a fresh stream
    are the filter's pre-ringing against the silence before it, not zeros: a caller that lines outputs up with inputs drops them.  The state is
    the last D o + width input samples of every stream; ``reset()`` makes the streams fresh again."""

    def __init__(self, resample: Resample, batch: int):
        if resample.orig_freq == resample.new_freq:
            raise ValueError("equal rates need no stream")
        if batch < 1:
            raise ValueError("batch must be positive")
        self.resample, self.batch = resample, int(batch)
        self.history = resample.delay_blocks * resample.o + resample.width
        self.delay = resample.delay_blocks * resample.n
        self.state = None
        self._dtype = torch.float32

    def reset(self) -> None:
        if self.state is not None:
            self.state.zero_()

    def push(self, chunk: torch.Tensor) -> torch.Tensor:
        r = self.resample
        _require(chunk, PCM, "ResampleStream")
        if chunk.dim() != 2 or chunk.shape[0] != self.batch or chunk.shape[1] % r.o != 0:
            raise ValueError(f"a push is ({self.batch}, k * {r.o}) samples, whole blocks; got {tuple(chunk.shape)}")
        if chunk.shape[1] == 0:          # nothing arrived (a stream front end that is still priming emits (B, 0)): nothing is owed, the state stays
            return torch.empty(self.batch, 0, dtype=chunk.dtype, device=chunk.device)
        if self.state is None:
            self.state = torch.zeros(self.batch, self.history, dtype=torch.float32, device=chunk.device)
        elif self.state.device != chunk.device:
            raise RuntimeError(f"the streams live on {self.state.device}")
        self._dtype = chunk.dtype
        blocks = chunk.shape[1] // r.o
        x, xs = Resample._rows(chunk)
        out = torch.empty(self.batch, blocks * r.n, dtype=chunk.dtype, device=chunk.device)
        s16 = int(chunk.dtype == torch.int16)
        launch(r.lib, chunk.device, r.lib.dn_resample_push, r.handle(chunk.device), self.state.data_ptr(), x.data_ptr(), s16, out.data_ptr(), s16,
               self.batch, blocks, xs, blocks * r.n)
        return out

    def flush(self) -> torch.Tensor:
        """pushes D blocks of zeros (in the dtype of the last push): the samples still owed for what has been pushed"""
        if self.state is None:
            raise RuntimeError("nothing has been pushed")
        return self.push(torch.zeros(self.batch, self.resample.delay_blocks * self.resample.o, dtype=self._dtype, device=self.state.device))
