"""Session pools: streams that join, leave and push hops on their own (``dn_sessions_*``).

``DenoiserStream`` and the pipes advance every stream of a batch by the same hop.  The reference serves one
``DenoisingAudioProcessor`` per WebRTC session instead (app3.py:123-133): sessions start and end at unrelated times and each
``recv()`` runs 0, 1 or 2 hops of its own (app3.py:167-178).  A ``SessionPool`` keeps ``capacity`` stream slots in HBM
(ring, overlap-add line, hx, frame counter, priming count, Griffin-Lim stream id) and runs one hop for any LIST of them per
launch, leaving every other slot untouched:

* slot and device layer: ``open`` / ``close`` / ``push(slots, hops)`` on device tensors;
* host layer: ``recv({slot: chunk})`` -- N concurrent ``recv`` calls of the reference, batched tick by tick;
* session state: ``export`` / ``suspend`` a list of slots into a ``SessionState`` (self-contained records, ``dn_sessions_export``),
  ``resume`` it in any pool of the same geometry and seed (``dn_sessions_import``), ``move`` sessions to another pool or device,
  ``resize`` a pool in place.  ``SessionState.save`` / ``load`` persist it across processes.

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

# the record layout of include/dn_denoise.h (DN_SESS_RECORD_MAGIC, DN_SESS_RECORD_VERSION, dn_session_record_header)
RECORD_MAGIC = 0x52534E44
RECORD_VERSION = 1
RECORD_HEAD = 64
HIDDEN = 17
_GEOMETRY = ("sample_rate", "n_fft", "hop", "n_mels", "hidden", "C")


def _a16(x: int) -> int:
    return (x + 15) & ~15


def record_layout(n_fft: int, C: int) -> dict:
    """Byte offsets of one record: ``ring``, ``ola``, ``hx`` and the ``stride`` (dn_sessions_record_bytes)."""
    ola = RECORD_HEAD + _a16(4 * n_fft)
    hx = ola + _a16(4 * n_fft)
    return dict(ring=RECORD_HEAD, ola=ola, hx=hx, stride=(hx + 4 * HIDDEN * C + 255) & ~255)


class SessionState:
    """The state of n sessions outside any pool: ``records`` (uint8 ``[n][stride]``, the layout of include/dn_denoise.h, on a device or
    the CPU), the pool's ``geometry`` (sample_rate, n_fft, hop, n_mels, hidden, C) and ``seed``, and per session the host side of
    ``SessionPool.recv``: the samples queued short of a whole hop and the push count that tells its priming rows.

    ``ring`` / ``ola`` / ``hx`` / ``frames`` / ``pushes`` (the record's priming count) / ``stream_ids`` are read-only numpy views decoded from
    the records."""

    def __init__(self, records: torch.Tensor, geometry: dict, seed: int, queues=None, host_pushes=None):
        n = int(records.shape[0]) if records.dim() == 2 else 0
        lay = record_layout(int(geometry["n_fft"]), int(geometry["C"]))
        if records.dtype != torch.uint8 or records.dim() != 2 or records.shape[1] != lay["stride"]:
            raise ValueError(f"records must be uint8 of shape (n, {lay['stride']})")
        self.records = records
        self.geometry = {k: int(geometry[k]) for k in _GEOMETRY}
        self.seed = int(seed)
        self.queues = [np.zeros(0, np.float32) for _ in range(n)] if queues is None else [np.asarray(q, np.float32) for q in queues]
        self.host_pushes = np.zeros(n, np.int64) if host_pushes is None else np.asarray(host_pushes, np.int64).copy()
        if len(self.queues) != n or self.host_pushes.shape != (n,):
            raise ValueError("one queue and one push count per record")
        self._host = None

    @classmethod
    def from_records(cls, records, seed: int = 0) -> "SessionState":
        """A state from bare records (e.g. written by the C API), geometry read from the first header."""
        t = torch.as_tensor(records)
        h = t[0, :32].cpu().numpy().view(np.uint32)
        return cls(t, dict(zip(_GEOMETRY, (int(v) for v in h[2:8]))), seed)

    def __len__(self) -> int:
        return len(self.queues)

    def to(self, device) -> "SessionState":
        return SessionState(self.records.to(device), self.geometry, self.seed, self.queues, self.host_pushes)

    # ---- decoded views
    def _decoded(self) -> np.ndarray:
        if self._host is None:
            self._host = self.records.cpu().numpy()
            self._host.flags.writeable = False
        return self._host

    def _field(self, off: int, count: int, dtype, shape=None) -> np.ndarray:
        r = self._decoded()
        size = np.dtype(dtype).itemsize
        v = np.ascontiguousarray(r[:, off:off + count * size]).view(dtype)
        v = v.reshape((len(self),) + (shape or (count,)))
        if shape is None and count == 1:
            v = v.reshape(len(self))
        v.flags.writeable = False
        return v

    @property
    def ring(self) -> np.ndarray:
        lay = record_layout(self.geometry["n_fft"], self.geometry["C"])
        return self._field(lay["ring"], self.geometry["n_fft"], np.float32)

    @property
    def ola(self) -> np.ndarray:
        lay = record_layout(self.geometry["n_fft"], self.geometry["C"])
        return self._field(lay["ola"], self.geometry["n_fft"], np.float32)

    @property
    def hx(self) -> np.ndarray:
        g = self.geometry
        return self._field(record_layout(g["n_fft"], g["C"])["hx"], HIDDEN * g["C"], np.float32, (HIDDEN, g["C"]))

    @property
    def pushes(self) -> np.ndarray:
        return self._field(32, 1, np.uint32)

    @property
    def frames(self) -> np.ndarray:
        return self._field(40, 1, np.uint64)

    @property
    def stream_ids(self) -> np.ndarray:
        return self._field(48, 1, np.uint64)

    # ---- persistence (.npz, no pickles)
    def save(self, path) -> None:
        q = self.queues
        np.savez(path, records=self.records.cpu().numpy(), geometry=np.array([self.geometry[k] for k in _GEOMETRY], np.int64),
                 seed=np.array(self.seed % (1 << 64), np.uint64), host_pushes=self.host_pushes,
                 queue_lengths=np.array([a.size for a in q], np.int64),
                 queue_samples=np.concatenate(q).astype(np.float32) if q else np.zeros(0, np.float32))

    @classmethod
    def load(cls, path) -> "SessionState":
        """A state saved by ``save``, on the CPU (``.to(device)`` or ``SessionPool.resume`` moves it)."""
        with np.load(path, allow_pickle=False) as z:
            lengths = z["queue_lengths"]
            cuts = np.cumsum(lengths)[:-1] if lengths.size else []
            queues = np.split(z["queue_samples"], cuts) if lengths.size else []
            return cls(torch.from_numpy(z["records"].copy()), dict(zip(_GEOMETRY, z["geometry"].tolist())), int(z["seed"]), queues,
                       z["host_pushes"])


class SessionPool:
    """``capacity`` stream slots bound to one ``Denoiser`` (its model, plan, ``n_iter`` and momentum).  Slot s's f-th frame (f counted
    from its ``open``) draws its Griffin-Lim phases from ``(seed + f, stream_id)``."""

    def __init__(self, denoiser, capacity: int, seed: int = 0):
        self.dn, self.capacity, self.seed = denoiser, int(capacity), int(seed)
        self.lib = denoiser.lib
        d = denoiser
        self.hop, self.n_fft = d.hop, d.n_fft
        self.prime = d.n_fft // d.hop - 1            # pushes of a new session that only fill its ring
        self.geometry = dict(sample_rate=d.sample_rate, n_fft=d.n_fft, hop=d.hop, n_mels=d.n_mels, hidden=HIDDEN, C=d.n_mels // 16)
        self._owner = d.model._native_owner(d.device)
        self._flags = d._flags()
        self._schedule = None
        self.handle, self._fin = self._create(self.capacity)
        self.record_bytes = int(self.lib.dn_sessions_record_bytes(self.handle))
        self._open = np.zeros(self.capacity, dtype=bool)
        self._pushes = np.zeros(self.capacity, dtype=np.int64)       # pushes since the open (host mirror, for the priming rows recv drops)
        self._queue: dict[int, np.ndarray] = {}                       # recv: float32 samples of each open session not yet pushed

    def _create(self, capacity: int):
        handle = C.c_void_p()
        with torch.cuda.device(self.dn.device):
            self.lib.check(self.lib.dn_sessions_create(self._owner.handle, self.dn.plan.handle, capacity, self._flags, C.byref(handle)))
        fin = weakref.finalize(self, self.lib.dn_sessions_destroy, handle)
        if self._schedule is not None:
            self.lib.check(self.lib.dn_sessions_set_schedule(handle, self._schedule))
        return handle, fin

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
        """``_lib.DN_SESS_AUTO`` / ``DN_SESS_ONE_LAUNCH`` / ``DN_SESS_TWO_LAUNCHES`` (n_fft 1024 only; refused at 512 and 1536): same samples, bit for bit."""
        self.lib.check(self.lib.dn_sessions_set_schedule(self.handle, int(schedule)))
        self._schedule = int(schedule)

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

    # ------------------------------------------------------------------ session state
    def _open_ids(self, slots) -> np.ndarray:
        ids = self._ids(slots)
        for s in ids:
            if not (0 <= s < self.capacity) or not self._open[s]:
                raise ValueError(f"slot {int(s)} is not open")
        if np.unique(ids).size != ids.size:
            raise ValueError("a slot appears twice in the list")
        return ids

    def export(self, slots) -> SessionState:
        """The state of the listed open slots as a ``SessionState`` (records on this pool's device, in list order).  The slots stay open
        and run on unchanged: exporting does not alter a session's samples."""
        ids = self._open_ids(slots)
        n = ids.size
        rec = torch.empty(n, self.record_bytes, dtype=torch.uint8, device=self.dn.device)
        if n:
            with torch.cuda.device(self.dn.device):
                self.lib.check(self.lib.dn_sessions_export(self.handle, ids.ctypes.data_as(C.c_void_p), n, rec.data_ptr(), self._stream()))
        return SessionState(rec, self.geometry, self.seed, [self._queue[int(s)].copy() for s in ids], self._pushes[ids])

    def suspend(self, slots) -> SessionState:
        """``export`` the listed slots, then close them."""
        st = self.export(slots)
        for s in self._ids(slots):
            self.close(int(s))
        return st

    def _check_compatible(self, geometry: dict, seed: int) -> None:
        if geometry != self.geometry:
            raise ValueError(f"the sessions' geometry {geometry} differs from this pool's {self.geometry}")
        if (seed - self.seed) % (1 << 64):
            raise ValueError(f"the sessions were recorded under seed {seed}, this pool runs seed {self.seed}: phases are keyed by "
                             "(seed + frame, stream id), so they would not continue bit for bit")

    def resume(self, state: SessionState, slots=None, stream_ids=None) -> list:
        """Open sessions with the state of ``state`` (from ``export`` / ``suspend`` / ``SessionState.load``) and return their slots:
        ``slots`` (free ones), default the lowest free.  ``stream_ids`` overrides the recorded Griffin-Lim stream ids.  Refused with
        ValueError, nothing changed, when the geometry or the seed differs or there are not enough free slots."""
        self._check_compatible(state.geometry, state.seed)
        n = len(state)
        if slots is None:
            free = np.flatnonzero(~self._open)
            if free.size < n:
                raise ValueError(f"{n} sessions for {free.size} free slots of {self.capacity}")
            ids = self._ids(free[:n])
        else:
            ids = self._ids(slots)
            if ids.size != n:
                raise ValueError(f"{ids.size} slots for {n} sessions")
            if np.unique(ids).size != n or np.any((ids < 0) | (ids >= self.capacity)):
                raise ValueError(f"slots must be distinct and in [0, {self.capacity})")
            if np.any(self._open[ids]):
                raise ValueError(f"slot {int(ids[self._open[ids]][0])} is open")
        sids = None
        if stream_ids is not None:
            sids = np.ascontiguousarray(np.asarray(stream_ids, dtype=np.uint64).reshape(-1))
            if sids.size != n:
                raise ValueError(f"{sids.size} stream ids for {n} sessions")
        if n == 0:
            return []
        rec = state.records.to(self.dn.device).contiguous()
        with torch.cuda.device(self.dn.device):
            self.lib.check(self.lib.dn_sessions_import(self.handle, ids.ctypes.data_as(C.c_void_p), n, rec.data_ptr(),
                                                       None if sids is None else sids.ctypes.data_as(C.c_void_p), self._stream()))
        self._open[ids] = True
        self._pushes[ids] = state.host_pushes
        for k, s in enumerate(ids):
            self._queue[int(s)] = state.queues[k].copy()
        return [int(s) for s in ids]

    def move(self, slots, other: "SessionPool") -> list:
        """Move the listed sessions to ``other`` (a pool of the same geometry and seed, on any device): they close here and continue
        there, bit for bit.  Returns their slots in ``other``.  Refused, nothing changed, as ``resume``."""
        ids = self._open_ids(slots)
        other._check_compatible(self.geometry, self.seed)
        if int((~other._open).sum()) < ids.size:
            raise ValueError(f"{ids.size} sessions for {int((~other._open).sum())} free slots of the other pool")
        st = self.export(ids)
        new = other.resume(st.to(other.dn.device))
        for s in ids:
            self.close(int(s))
        return new

    def resize(self, capacity: int) -> None:
        """Grow or shrink the pool in place: every open session keeps its slot number and continues bit for bit.  A shrink that would
        drop an open slot is refused with ValueError, nothing changed."""
        capacity = int(capacity)
        if capacity <= 0:
            raise ValueError("capacity must be positive")
        live = np.flatnonzero(self._open)
        if live.size and live[-1] >= capacity:
            raise ValueError(f"slot {int(live[-1])} is open: the pool cannot shrink to {capacity} slots")
        handle, fin = self._create(capacity)
        try:
            if live.size:
                ids = self._ids(live)
                rec = torch.empty(ids.size, self.record_bytes, dtype=torch.uint8, device=self.dn.device)
                with torch.cuda.device(self.dn.device):
                    st = self._stream()
                    self.lib.check(self.lib.dn_sessions_export(self.handle, ids.ctypes.data_as(C.c_void_p), ids.size, rec.data_ptr(), st))
                    self.lib.check(self.lib.dn_sessions_import(handle, ids.ctypes.data_as(C.c_void_p), ids.size, rec.data_ptr(), None, st))
        except Exception:
            fin()
            raise
        self._fin()                       # (waits for the launches that read the old pool)
        self.handle, self._fin, self.capacity = handle, fin, capacity
        keep = min(capacity, self._open.size)
        for name in ("_open", "_pushes"):
            old = getattr(self, name)
            new = np.zeros(capacity, dtype=old.dtype)
            new[:keep] = old[:keep]
            setattr(self, name, new)
