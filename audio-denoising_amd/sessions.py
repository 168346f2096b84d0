"""Session pools: streams that join, leave and push hops on their own (``dn_sessions_*``).

``DenoiserStream`` and the pipes advance every stream of a batch by the same hop.  The reference serves one
``DenoisingAudioProcessor`` per WebRTC session instead (app3.py:123-133): sessions start and end at unrelated times and each
``recv()`` runs 0, 1 or 2 hops of its own (app3.py:167-178).  A ``SessionPool`` keeps ``capacity`` stream slots in HBM
(ring, overlap-add line, hx, frame counter, priming count, Griffin-Lim stream id) and runs one hop for any LIST of them per
launch, leaving every other slot untouched:

* slot and device layer: ``open`` / ``close`` / ``push(slots, hops)`` on device tensors;
* host layer: ``recv({slot: chunk})`` -- N concurrent ``recv`` calls of the reference, batched tick by tick.

A session's samples equal ``DenoiserStream(denoiser, 1, stream_id0=stream_id, seed=seed)`` fed the same hops, bit for bit, whatever
other sessions shared its pushes.  Not thread-safe (one host thread per pool) and not capturable into a hipGraph; issue every call
of a pool on one stream.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch

from . import _lib


class SessionPool:
    """``capacity`` stream slots bound to one ``Denoiser`` (its model, plan, ``n_iter`` and momentum).  Slot s's f-th frame (f counted
    from its ``open``) draws its Griffin-Lim phases from ``(seed + f, stream_id)``."""

    def __init__(self, denoiser, capacity: int, seed: int = 0):
        self.dn, self.capacity, self.seed = denoiser, int(capacity), int(seed)
        self.lib = denoiser.lib
        d = denoiser
        self.hop, self.n_fft = d.hop, d.n_fft
        self.prime = d.n_fft // d.hop - 1            # pushes of a new session that only fill its ring
        self._owner = d.model._native_owner(d.device)
        self._flags = d._flags()
        handle = C.c_void_p()
        with torch.cuda.device(d.device):
            self.lib.check(self.lib.dn_sessions_create(self._owner.handle, d.plan.handle, self.capacity, self._flags, C.byref(handle)))
        self.handle = handle
        self._fin = weakref.finalize(self, self.lib.dn_sessions_destroy, handle)
        self._open = np.zeros(self.capacity, dtype=bool)
        self._pushes = np.zeros(self.capacity, dtype=np.int64)       # pushes since the open (host mirror, for the priming rows recv drops)
        self._queue: dict[int, np.ndarray] = {}                       # recv: float32 samples of each open session not yet pushed

    # ------------------------------------------------------------------ slot and device layer
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dn.device).cuda_stream)

    def _ids(self, slots) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(slots, dtype=np.int64).reshape(-1).astype(np.int32))

    def open(self, stream_id: int | None = None) -> int:
        """Open the lowest free slot: zero ring, overlap-add line and hx, zero counters, Griffin-Lim stream id ``stream_id`` (None: the slot
        index).  Returns the slot; raises RuntimeError when the pool is full."""
        free = np.flatnonzero(~self._open)
        if free.size == 0:
            raise RuntimeError(f"session pool is full ({self.capacity} slots)")
        slot = int(free[0])
        ids = self._ids([slot])
        sid = None if stream_id is None else (C.c_uint64 * 1)(int(stream_id))
        with torch.cuda.device(self.dn.device):
            self.lib.check(self.lib.dn_sessions_open(self.handle, ids.ctypes.data_as(C.c_void_p), 1, sid, self._stream()))
        self._open[slot] = True
        self._pushes[slot] = 0
        self._queue[slot] = np.zeros(0, dtype=np.float32)
        return slot

    def close(self, slot: int) -> None:
        """Close a slot: it may not be pushed until it is opened again (its buffered samples are dropped)."""
        ids = self._ids([slot])
        self.lib.check(self.lib.dn_sessions_close(self.handle, ids.ctypes.data_as(C.c_void_p), 1))
        self._open[slot] = False
        self._queue.pop(int(slot), None)

    def set_schedule(self, schedule: int) -> None:
        """``_lib.DN_SESS_AUTO`` / ``DN_SESS_ONE_LAUNCH`` / ``DN_SESS_TWO_LAUNCHES`` (n_fft 1024): same samples, bit for bit."""
        self.lib.check(self.lib.dn_sessions_set_schedule(self.handle, int(schedule)))

    def counters(self, slot: int):
        """(frames since the open, pushes counted up to n_fft/hop - 1) of a slot.  Synchronises the current stream."""
        f, p = C.c_uint64(), C.c_int32()
        with torch.cuda.device(self.dn.device):
            self.lib.check(self.lib.dn_sessions_get_counters(self.handle, int(slot), C.byref(f), C.byref(p), self._stream()))
        return f.value, p.value

    def push(self, slots, hops: torch.Tensor, out: torch.Tensor | None = None, init_angles: torch.Tensor | None = None) -> torch.Tensor:
        """One hop for each listed slot.  ``hops`` (n, hop) float32 or int16 PCM (x / 32767) on the denoiser's device, rows in list order;
        ``out`` (n, hop) float32 or int16 (clip, * 32767, truncate), default: the dtype of ``hops``.  A session's first n_fft/hop - 1 pushes
        emit zeros (they only fill its ring).  ``init_angles``: (n, n_fft/2+1, 3) complex64 initial phases (default: the device generator)."""
        d = self.dn
        ids = self._ids(slots)
        n = ids.size
        if hops.device != d.device or hops.dtype not in (torch.float32, torch.int16) or tuple(hops.shape) != (n, self.hop) \
                or not hops.is_contiguous():
            raise ValueError(f"hops must be contiguous float32 or int16 of shape {(n, self.hop)} on {d.device}")
        if out is None:
            out = torch.empty(n, self.hop, dtype=hops.dtype, device=d.device)
        elif out.device != d.device or out.dtype not in (torch.float32, torch.int16) or tuple(out.shape) != (n, self.hop) \
                or not out.is_contiguous():
            raise ValueError(f"out must be contiguous float32 or int16 of shape {(n, self.hop)} on {d.device}")
        if d.model._native_owner(d.device) is not self._owner or d._flags() != self._flags:
            raise RuntimeError("the model's weights or conv_precision changed after the session pool was created; create a new pool")
        keep, ia_ptr = d._angles_ptr(init_angles, n)
        with torch.cuda.device(d.device):
            self.lib.check(self.lib.dn_sessions_push(self.handle, ids.ctypes.data_as(C.c_void_p), n, hops.data_ptr() if n else None,
                                                     int(hops.dtype == torch.int16), out.data_ptr() if n else None,
                                                     int(out.dtype == torch.int16), ia_ptr, self.seed, d.n_iter, d.momentum, self._stream()))
        self._pushes[ids] += 1
        return out

    # ------------------------------------------------------------------ host layer
    def recv(self, chunks: dict) -> dict:
        """N concurrent ``DenoisingAudioProcessor.recv`` calls (app3.py:167-250): ``{slot: chunk}`` with 1-D int16 PCM or float32 chunks of any
        length -> ``{slot: samples}``.  Samples queue per session on the host; a tick is ONE push over every session with a whole hop
        waiting, and as many ticks run as the longest queue needs.  Each session gets its emitted hops concatenated (the pushes that only
        fill a new session's ring are dropped, so the output lines up with ``DenoiserStream`` and the reference) -- or, when no hop ran for
        it, the passthrough of its own chunk (app3.py:228-241).  int16 chunks get int16 back, clipped and truncated as app3.py:244-245;
        float32 chunks get the float32 samples (passthrough: the chunk clipped to [-1, 1])."""
        s16, taken = {}, {}
        for slot, chunk in chunks.items():
            slot = int(slot)
            if not (0 <= slot < self.capacity) or not self._open[slot]:
                raise ValueError(f"slot {slot} is not open")
            a = np.asarray(chunk)
            if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
                raise ValueError("a chunk is a 1-D int16 or float32 array")
            s16[slot] = a.dtype == np.int16
            f = a.astype(np.float32) / np.iinfo(np.int16).max if s16[slot] else a        # app3.py:172
            taken[slot] = f
            self._queue[slot] = np.concatenate([self._queue[slot], f])
        emitted = {slot: [] for slot in chunks}
        dev = self.dn.device
        while True:
            ready = [s for s in sorted(taken) if self._queue[s].size >= self.hop]
            if not ready:
                break
            hops = np.stack([self._queue[s][:self.hop] for s in ready])
            for s in ready:
                self._queue[s] = self._queue[s][self.hop:]
            primed = self._pushes[ready] >= self.prime          # before this push: does it run a frame for the session?
            out = self.push(ready, torch.from_numpy(hops).to(dev))
            emitted_rows = out.cpu().numpy()
            for r, s in enumerate(ready):
                if primed[r]:
                    emitted[s].append(emitted_rows[r])
        res = {}
        for slot in chunks:
            slot = int(slot)
            if emitted[slot]:
                y = np.concatenate(emitted[slot])
                res[slot] = (np.clip(y, -1.0, 1.0) * np.iinfo(np.int16).max).astype(np.int16) if s16[slot] else y    # app3.py:244-245
            else:
                p = np.clip(taken[slot], -1.0, 1.0)                                                                   # app3.py:232
                res[slot] = (p * np.iinfo(np.int16).max).astype(np.int16) if s16[slot] else p
        return res
