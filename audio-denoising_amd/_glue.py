"""What every Python front end does around a C call, once: the launch on the handle's device and current stream (``launch``), the argument
check of a tensor handed to the library (``check_tensor``), the storage of injected Griffin-Lim phases (``pack_phases``) and the schedule of
a ragged clip call over the frame cap (``ragged_rounds``).  ``check_tensor``, ``pack_phases`` and ``ragged_rounds`` need neither the
library nor a GPU."""
from __future__ import annotations

import ctypes as C

import torch

PCM = (torch.float32, torch.int16)          # the sample formats of the PCM convention: float32, or int16 read as x / 32767


def stream_ptr(device=None):
    """the pointer of the current stream of ``device`` (None: the current device), as the C ABI takes it"""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def launch(lib, device, fn, *args, after=()):
    """``fn(*args, stream, *after)`` with ``device`` current and ``stream`` the pointer of its current stream, through ``lib.check``: every
    launch of the package.  ``after``: what a C function takes behind its stream (the ticket of ``dn_pipe_stream_push_host``)."""
    with torch.cuda.device(device):
        lib.check(fn(*args, stream_ptr(), *after))


def record_on_stream(t: torch.Tensor, device) -> None:
    """keeps ``t`` alive until what ``device``'s current stream holds has run (the launch before copies it); nothing inside a capture"""
    with torch.cuda.device(device):
        if not torch.cuda.is_current_stream_capturing():
            t.record_stream(torch.cuda.current_stream())


def check_tensor(t: torch.Tensor, name: str, shape=None, dtypes=PCM, device=None, device_error=ValueError, dtype_error=ValueError,
                 min_width: int = 0, contiguous: bool = True) -> None:
    """Refuses ``t`` unless it lives on ``device`` (a ``torch.device``, or a device type such as ``"cuda"``; else ``device_error``), has one of
    ``dtypes`` (else ``dtype_error``), the shape ``shape`` -- an entry None takes any size, ``shape=None`` any shape --, a last dimension of
    at least ``min_width`` and, with ``contiguous``, contiguous storage (else ValueError)."""
    if device is not None and (t.device.type if isinstance(device, str) else t.device) != device:
        raise device_error(f"{name} must be a {device.upper()} tensor" if isinstance(device, str) else f"{name} must live on {device} (no CPU path)")
    if t.dtype not in dtypes:
        raise dtype_error(f"{name} must be {' or '.join(str(d) for d in dtypes)}; got {t.dtype}")
    if shape is not None and tuple(t.shape) != shape and (t.dim() != len(shape) or any(w is not None and w != s for w, s in zip(shape, t.shape))):
        raise ValueError(f"{name} must have shape {shape}; got {tuple(t.shape)}")
    if min_width and t.shape[-1] < min_width:
        raise ValueError(f"{name} must be at least {min_width} samples wide; got {tuple(t.shape)}")
    if contiguous and not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def pack_phases(init_angles: torch.Tensor, lead, bins: int, device, from_input: bool = False) -> torch.Tensor:
    """Initial Griffin-Lim phases as the reference draws them, complex64 ``(*lead, K, 3)`` -> the ``[*lead][3][K]`` interleaved float32 storage
    the library reads, ``(*lead, 3, K, 2)`` on ``device``.  ``from_input``: the denoiser runs ``phase="input"`` and takes none."""
    if from_input:
        raise ValueError("this denoiser takes its initial phases from the input (phase='input'): init_angles cannot be passed")
    shape = tuple(lead) + (bins, 3)
    if tuple(init_angles.shape) != shape or init_angles.dtype != torch.complex64:
        raise ValueError(f"init_angles must be complex64 of shape {shape}; got {init_angles.dtype} {tuple(init_angles.shape)}")
    return torch.view_as_real(init_angles.to(device).transpose(-1, -2).contiguous())


def ragged_rounds(n_hops, cap: int):
    """The calls a ragged clip of ``n_hops[b]`` hops a stream is cut into when one call carries at most ``cap`` frames: yields, per round, the
    hops each stream runs.  Everything in one round where it fits; else the streams with hops left share the cap equally (the first ``cap`` of
    them when more are live), each runs at most what it has left, every other stream 0."""
    left = list(n_hops)
    if 0 < sum(left) <= cap:
        yield left
        return
    while True:
        live = [b for b, v in enumerate(left) if v > 0][:cap]
        if not live:
            return
        n = [0] * len(left)
        for b in live:
            n[b] = min(left[b], cap // len(live))
            left[b] -= n[b]
        yield n
