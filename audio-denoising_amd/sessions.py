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
  ``resize`` a pool in place.  ``SessionState.save`` / ``load`` persist it across processes;
* rates: ``SessionPool(..., rates=(8000, 48000))`` serves sessions at their own sample rates next to the plan's.  A ``RateBank``
  (``dn_ratebank_*``) converts every listed row at its session's rate in ONE launch on either side of the push and keeps each session's
  converter state; ``open(sample_rate=)``, ``push_rated``, ``recv`` and the session state carry the rate end to end.

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
from ._glue import PCM, check_tensor, launch, stream_ptr

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

    def __init__(self, records: torch.Tensor, geometry: dict, seed: int, queues=None, host_pushes=None, rates=None, adapter_in=None,
                 adapter_out=None):
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
        # sessions at another rate than the plan's (SessionPool(rates=...)): ``rates`` (n,) the sample rate of each session, ``adapter_in`` /
        # ``adapter_out`` per session the H(rate) floats of its two converter states (empty at the plan's rate).  All None: no session has a rate.
        self.rates = None if rates is None else np.asarray(rates, np.int64).copy()
        if self.rates is None:
            if adapter_in is not None or adapter_out is not None:
                raise ValueError("adapter states need the sessions' rates")
            self.adapter_in = self.adapter_out = None
        else:
            if adapter_in is None or adapter_out is None:
                raise ValueError("sessions with rates need both adapter states")
            self.adapter_in = [np.asarray(a, np.float32).copy() for a in adapter_in]
            self.adapter_out = [np.asarray(a, np.float32).copy() for a in adapter_out]
            if self.rates.shape != (n,) or len(self.adapter_in) != n or len(self.adapter_out) != n:
                raise ValueError("one rate and one pair of adapter states per record")
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
        return SessionState(self.records.to(device), self.geometry, self.seed, self.queues, self.host_pushes, self.rates, self.adapter_in,
                            self.adapter_out)

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

        def ragged(name, rows):
            return {name + "_lengths": np.array([a.size for a in rows], np.int64),
                    name + "_samples": np.concatenate(rows).astype(np.float32) if rows else np.zeros(0, np.float32)}
        extra = {}
        if self.rates is not None:          # (a state without rates writes exactly the keys it always wrote)
            extra = dict(rates=self.rates, **ragged("adapter_in", self.adapter_in), **ragged("adapter_out", self.adapter_out))
        np.savez(path, records=self.records.cpu().numpy(), geometry=np.array([self.geometry[k] for k in _GEOMETRY], np.int64),
                 seed=np.array(self.seed % (1 << 64), np.uint64), host_pushes=self.host_pushes,
                 queue_lengths=np.array([a.size for a in q], np.int64),
                 queue_samples=np.concatenate(q).astype(np.float32) if q else np.zeros(0, np.float32), **extra)

    @classmethod
    def load(cls, path) -> "SessionState":
        """A state saved by ``save``, on the CPU (``.to(device)`` or ``SessionPool.resume`` moves it)."""
        with np.load(path, allow_pickle=False) as z:
            def ragged(name):
                lengths = z[name + "_lengths"]
                cuts = np.cumsum(lengths)[:-1] if lengths.size else []
                return np.split(z[name + "_samples"], cuts) if lengths.size else []
            rated = {}
            if "rates" in z.files:
                rated = dict(rates=z["rates"], adapter_in=ragged("adapter_in"), adapter_out=ragged("adapter_out"))
            return cls(torch.from_numpy(z["records"].copy()), dict(zip(_GEOMETRY, z["geometry"].tolist())), int(z["seed"]), ragged("queue"),
                       z["host_pushes"], **rated)


def rate_index(plan_rate: int, rates, sample_rate) -> int:
    """The rate index of a session: -1 at the plan's rate (or None), else its position in ``rates``; ValueError names the accepted rates."""
    if sample_rate is None or int(sample_rate) == int(plan_rate):
        return -1
    rates = tuple(int(r) for r in rates or ())
    if int(sample_rate) not in rates:
        raise ValueError(f"sample rate {sample_rate} is not one of this pool's: the plan's {plan_rate}" +
                         (f" or rates={rates}" if rates else " (the pool was created without rates)"))
    return rates.index(int(sample_rate))


class RateBank:
    """The rate adapters of a pool (``dn_ratebank_*``): for each of ``rates`` the table rate -> plan and plan -> rate of a plan of
    ``plan_rate`` / ``hop``.  ``ingest`` and ``emit`` convert a list of rows, each at its own session's rate, in one launch each and update
    the listed slots' rows of the caller's state tensors (``new_state``).  Rates the kernels do not take (44100 on a 16 kHz plan) raise
    ``DnError`` naming the rule.  Not thread-safe, not capturable."""

    def __init__(self, plan_rate: int, hop: int, rates, device, lib=None, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.plan_rate, self.hop, self.rates, self.device = int(plan_rate), int(hop), tuple(int(r) for r in rates), torch.device(device)
        if not 1 <= len(self.rates) <= 8:
            raise ValueError("a rate bank holds 1 to 8 rates")
        self.lib = _lib.get_lib() if lib is None else lib
        cfg = _lib.RateBankCfg(self.plan_rate, self.hop, (C.c_int32 * 8)(*self.rates), len(self.rates), int(lowpass_filter_width), float(rolloff))
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            self.lib.check(self.lib.dn_ratebank_create(C.byref(cfg), C.byref(self.handle)))
        weakref.finalize(self, self.lib.dn_ratebank_destroy, self.handle)
        self.stride = (int(self.lib.dn_ratebank_state_stride(self.handle, _lib.DN_RATEBANK_IN)),
                       int(self.lib.dn_ratebank_state_stride(self.handle, _lib.DN_RATEBANK_OUT)))
        self._geo = []
        for k in range(len(self.rates)):
            v = [C.c_int32() for _ in range(6)]
            self.lib.check(self.lib.dn_ratebank_geometry(self.handle, k, *[C.byref(x) for x in v]))
            self._geo.append(dict(zip(("chunk_in", "chunk_out", "hist_in", "hist_out", "delay_in", "delay_out"), (x.value for x in v))))

    def index(self, sample_rate) -> int:
        return rate_index(self.plan_rate, self.rates, sample_rate)

    def geometry(self, sample_rate) -> dict:
        """chunk_in / chunk_out (samples per hop), hist_in / hist_out (state floats), delay_in (plan samples) / delay_out (session samples)"""
        k = self.index(sample_rate)
        if k < 0:
            return dict(chunk_in=self.hop, chunk_out=self.hop, hist_in=0, hist_out=0, delay_in=0, delay_out=0)
        return dict(self._geo[k])

    def new_state(self, capacity: int):
        """(state_in, state_out): zeros, (capacity, stride) float32 each -- every slot a fresh session"""
        return tuple(torch.zeros(int(capacity), s, dtype=torch.float32, device=self.device) for s in self.stride)

    def _lists(self, slots, rate_idx):
        ids = np.ascontiguousarray(np.asarray(slots, dtype=np.int64).reshape(-1).astype(np.int32))
        ridx = np.ascontiguousarray(np.asarray(rate_idx, dtype=np.int64).reshape(-1).astype(np.int32))
        if ids.size != ridx.size:
            raise ValueError("one rate index per slot")
        return ids, ridx

    def _check(self, t, what, dtypes, rows):
        check_tensor(t, what, (rows, None), dtypes, self.device)

    def ingest(self, slots, rate_idx, state_in: torch.Tensor, x: torch.Tensor, hop_in: torch.Tensor | None = None) -> torch.Tensor:
        """x (n, W) float32 or int16 at each row's rate -> hop_in (n, hop) float32 at the plan's; state_in (capacity, stride) advances"""
        ids, ridx = self._lists(slots, rate_idx)
        n = ids.size
        self._check(x, "x", PCM, n)
        self._check(state_in, "state_in", (torch.float32,), state_in.shape[0])
        if hop_in is None:
            hop_in = torch.empty(n, self.hop, dtype=torch.float32, device=self.device)
        self._check(hop_in, "hop_in", (torch.float32,), n)
        if state_in.shape[1] != self.stride[0] or hop_in.shape[1] != self.hop:
            raise ValueError(f"state_in rows are {self.stride[0]} floats, hop_in rows {self.hop}")
        launch(self.lib, self.device, self.lib.dn_ratebank_ingest, self.handle, ids.ctypes.data_as(C.c_void_p), ridx.ctypes.data_as(C.c_void_p), n,
               state_in.shape[0], state_in.data_ptr(), x.data_ptr() if n else None, int(x.dtype == torch.int16), x.shape[1],
               hop_in.data_ptr() if n else None)
        return hop_in

    def emit(self, slots, rate_idx, state_out: torch.Tensor, hop_out: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """hop_out (n, hop) float32 -> y (n, W) float32 or int16, row i valid up to its rate's chunk_out; state_out advances"""
        ids, ridx = self._lists(slots, rate_idx)
        n = ids.size
        self._check(hop_out, "hop_out", (torch.float32,), n)
        self._check(y, "y", PCM, n)
        self._check(state_out, "state_out", (torch.float32,), state_out.shape[0])
        if state_out.shape[1] != self.stride[1] or hop_out.shape[1] != self.hop:
            raise ValueError(f"state_out rows are {self.stride[1]} floats, hop_out rows {self.hop}")
        launch(self.lib, self.device, self.lib.dn_ratebank_emit, self.handle, ids.ctypes.data_as(C.c_void_p), ridx.ctypes.data_as(C.c_void_p), n,
               state_out.shape[0], state_out.data_ptr(), hop_out.data_ptr() if n else None, y.data_ptr() if n else None,
               int(y.dtype == torch.int16), y.shape[1])
        return y


class SessionPool:
    """``capacity`` stream slots bound to one ``Denoiser`` (its model, plan, ``n_iter`` and momentum).  Slot s's f-th frame (f counted
    from its ``open``) draws its Griffin-Lim phases from ``(seed + f, stream_id)``.

    ``rates``: sample rates other than the plan's that sessions may be opened at (``open(sample_rate=)``): such a session brings
    ``chunk(slot)[0]`` samples a hop at its own rate and gets ``chunk(slot)[1]`` back (``push_rated``, ``recv``), converted by a ``RateBank``
    in one launch on either side of the push.  Its samples equal ``ResampleStream(rate -> plan, 1)`` -> a one-session pool ->
    ``ResampleStream(plan -> rate, 1)`` bit for bit, so they lag the input by ``delay(slot)`` samples, which nothing compensates."""

    def __init__(self, denoiser, capacity: int, seed: int = 0, rates=None):
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
        self.rates = tuple(int(r) for r in rates) if rates else ()
        self._rate = np.full(self.capacity, -1, dtype=np.int32)       # rate index of each slot: -1 the plan's, else into self.rates
        self.bank = RateBank(d.sample_rate, d.hop, self.rates, d.device, lib=self.lib) if self.rates else None
        self._adapt = self.bank.new_state(self.capacity) if self.bank else None          # (state_in, state_out) [capacity][stride]
        # (samples in, samples out) of a hop by rate index, the plan's rate last
        self._chunks = np.array([[g["chunk_in"], g["chunk_out"]] for g in (self.bank.geometry(r) for r in self.rates)] + [[self.hop, self.hop]])

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
        """the pointer of the pool's current stream, for a caller that makes a ``dn_sessions_*`` call of its own on the pool's handle"""
        return stream_ptr(self.dn.device)

    def _ids(self, slots) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(slots, dtype=np.int64).reshape(-1).astype(np.int32))

    def open(self, stream_id: int | None = None, sample_rate: int | None = None) -> int:
        """Open the lowest free slot: zero ring, overlap-add line and hx, zero counters, Griffin-Lim stream id ``stream_id`` (None: the slot
        index).  ``sample_rate``: the plan's (default) or one of the pool's ``rates`` (anything else: ValueError); the slot's two converter
        states start at zero.  Returns the slot; raises RuntimeError when the pool is full."""
        rate = rate_index(self.geometry["sample_rate"], self.rates, sample_rate)
        free = np.flatnonzero(~self._open)
        if free.size == 0:
            raise RuntimeError(f"session pool is full ({self.capacity} slots)")
        slot = int(free[0])
        ids = self._ids([slot])
        sid = None if stream_id is None else (C.c_uint64 * 1)(int(stream_id))
        launch(self.lib, self.dn.device, self.lib.dn_sessions_open, self.handle, ids.ctypes.data_as(C.c_void_p), 1, sid)
        self._open[slot] = True
        self._pushes[slot] = 0
        self._queue[slot] = np.zeros(0, dtype=np.float32)
        self._rate[slot] = rate
        if self._adapt is not None:
            for t in self._adapt:
                t[slot].zero_()
        return slot

    def close(self, slot: int) -> None:
        """Close a slot: it may not be pushed until it is opened again (its buffered samples are dropped)."""
        ids = self._ids([slot])
        self.lib.check(self.lib.dn_sessions_close(self.handle, ids.ctypes.data_as(C.c_void_p), 1))
        self._open[slot] = False
        self._rate[slot] = -1
        self._queue.pop(int(slot), None)

    def set_schedule(self, schedule: int) -> None:
        """``_lib.DN_SESS_AUTO`` / ``DN_SESS_ONE_LAUNCH`` / ``DN_SESS_TWO_LAUNCHES`` (n_fft 1024 only; refused at 512 and 1536): same samples, bit for bit."""
        self.lib.check(self.lib.dn_sessions_set_schedule(self.handle, int(schedule)))
        self._schedule = int(schedule)

    def counters(self, slot: int):
        """(frames since the open, pushes counted up to n_fft/hop - 1) of a slot.  Synchronises the current stream."""
        f, p = C.c_uint64(), C.c_int32()
        launch(self.lib, self.dn.device, self.lib.dn_sessions_get_counters, self.handle, int(slot), C.byref(f), C.byref(p))
        return f.value, p.value

    def push(self, slots, hops: torch.Tensor, out: torch.Tensor | None = None, init_angles: torch.Tensor | None = None) -> torch.Tensor:
        """One hop for each listed slot.  ``hops`` (n, hop) float32 or int16 PCM (x / 32767) on the denoiser's device, rows in list order;
        ``out`` (n, hop) float32 or int16 (clip, * 32767, truncate), default: the dtype of ``hops``.  A session's first n_fft/hop - 1 pushes
        emit zeros (they only fill its ring).  ``init_angles``: (n, n_fft/2+1, 3) complex64 initial phases (default: the device generator)."""
        ids = self._ids(slots)
        if self.bank is not None and ids.size and np.all((ids >= 0) & (ids < self.capacity)) and np.any(self._rate[ids] >= 0):
            rated = ids[self._rate[ids] >= 0]
            raise ValueError(f"slot {int(rated[0])} was opened at {self.rates[self._rate[rated[0]]]} Hz: push takes hops at the plan's rate, "
                             "use push_rated or recv")
        return self._push(ids, hops, out, init_angles)

    def _push(self, ids, hops, out, init_angles=None) -> torch.Tensor:
        d = self.dn
        n = ids.size
        check_tensor(hops, "hops", (n, self.hop), PCM, d.device)
        if out is None:
            out = torch.empty(n, self.hop, dtype=hops.dtype, device=d.device)
        else:
            check_tensor(out, "out", (n, self.hop), PCM, d.device)
        if d.model._native_owner(d.device) is not self._owner or d._flags() != self._flags:
            raise RuntimeError("the model's weights or conv_precision changed after the session pool was created; create a new pool")
        keep, ia_ptr = d._angles_ptr(init_angles, n)
        launch(self.lib, d.device, self.lib.dn_sessions_push, self.handle, ids.ctypes.data_as(C.c_void_p), n, hops.data_ptr() if n else None,
               int(hops.dtype == torch.int16), out.data_ptr() if n else None, int(out.dtype == torch.int16), ia_ptr, self.seed, d.n_iter,
               d.momentum)
        self._pushes[ids] += 1
        return out

    # ------------------------------------------------------------------ rates
    def sample_rate(self, slot: int) -> int:
        k = self._rate[int(slot)]
        return self.geometry["sample_rate"] if k < 0 else self.rates[k]

    def chunk(self, slot: int):
        """(samples in, samples out) of a hop of this slot, at its session's rate"""
        k = self._rate[int(slot)]
        if k < 0:
            return self.hop, self.hop
        g = self.bank.geometry(self.rates[k])
        return g["chunk_in"], g["chunk_out"]

    def delay(self, slot: int) -> int:
        """The round-trip lag the two converters add, in samples at the session's rate: the D_d n_d plan samples of the way in, scaled to the
        session's rate, plus the D_u n_u samples of the way out (48 kHz on a 16 kHz plan: 21 + 21 = 42).  Not compensated."""
        k = self._rate[int(slot)]
        if k < 0:
            return 0
        g = self.bank.geometry(self.rates[k])
        return g["delay_in"] * self.rates[k] // self.geometry["sample_rate"] + g["delay_out"]

    def push_rated(self, slots, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """One hop for each listed slot at its session's own rate.  ``x`` (n, W) float32 or int16 PCM on the denoiser's device, row i holding
        ``chunk(slot_i)[0]`` samples (W at least the longest); returns ``out`` (n, W_out) float32 or int16 (default: the dtype of ``x``; W_out
        at least the longest ``chunk(slot_i)[1]``, default exactly that), row i valid up to ``chunk(slot_i)[1]``, the rest untouched.
        Three launches: ingest, the push (float32 both ways), emit -- priming pushes included, whose rows come out exactly zero."""
        if self.bank is None:
            raise RuntimeError("this pool was created without rates")
        ids = self._open_ids(slots)
        n = ids.size
        ridx = self._rate[ids]
        ch = self._chunks[ridx]          # (index -1, the plan's rate: the last row)
        w_in, w_out = (int(ch[:, 0].max()), int(ch[:, 1].max())) if n else (0, 0)
        dev = self.dn.device
        check_tensor(x, "x", (n, None), PCM, dev, min_width=w_in)
        if out is None:
            out = torch.empty(n, w_out, dtype=x.dtype, device=dev)
        else:
            check_tensor(out, "out", (n, None), PCM, dev, min_width=w_out)
        if n == 0:
            return out
        hop_in = self.bank.ingest(ids, ridx, self._adapt[0], x)
        hop_out = self._push(ids, hop_in, torch.empty_like(hop_in))
        return self.bank.emit(ids, ridx, self._adapt[1], hop_out, out)

    # ------------------------------------------------------------------ host layer
    def recv(self, chunks: dict) -> dict:
        """N concurrent ``DenoisingAudioProcessor.recv`` calls (app3.py:167-250): ``{slot: chunk}`` with 1-D int16 PCM or float32 chunks of any
        length, at each session's own rate -> ``{slot: samples}``.  Samples queue per session on the host; a tick is ONE push over every session with a whole hop
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
            ready = [s for s in sorted(taken) if self._queue[s].size >= self.chunk(s)[0]]
            if not ready:
                break
            primed = self._pushes[ready] >= self.prime          # before this push: does it run a frame for the session?
            if self.bank is None:
                hops = np.stack([self._queue[s][:self.hop] for s in ready])
                for s in ready:
                    self._queue[s] = self._queue[s][self.hop:]
                out = self.push(ready, torch.from_numpy(hops).to(dev))
            else:          # a session's whole hop is chunk(s)[0] samples at its own rate; one push_rated over all of them
                x = np.zeros((len(ready), max(self.chunk(s)[0] for s in ready)), dtype=np.float32)
                for r, s in enumerate(ready):
                    cin = self.chunk(s)[0]
                    x[r, :cin] = self._queue[s][:cin]
                    self._queue[s] = self._queue[s][cin:]
                out = self.push_rated(ready, torch.from_numpy(x).to(dev))
            emitted_rows = out.cpu().numpy()
            for r, s in enumerate(ready):
                if primed[r]:
                    emitted[s].append(emitted_rows[r][:self.chunk(s)[1]])
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
            launch(self.lib, self.dn.device, self.lib.dn_sessions_export, self.handle, ids.ctypes.data_as(C.c_void_p), n, rec.data_ptr())
        return SessionState(rec, self.geometry, self.seed, [self._queue[int(s)].copy() for s in ids], self._pushes[ids], **self._export_rates(ids))

    def _export_rates(self, ids) -> dict:
        """the rate fields of a SessionState for the listed slots: empty when none of them has a rate of its own"""
        if self.bank is None or not np.any(self._rate[ids] >= 0):
            return {}
        idx = torch.from_numpy(ids.astype(np.int64)).to(self.dn.device)
        rows = [t.index_select(0, idx).cpu().numpy() for t in self._adapt]
        rates = [self.sample_rate(s) for s in ids]
        geo = [self.bank.geometry(r) for r in rates]          # (no state floats at the plan's rate)
        return dict(rates=rates, adapter_in=[rows[0][i, :g["hist_in"]] for i, g in enumerate(geo)],
                    adapter_out=[rows[1][i, :g["hist_out"]] for i, g in enumerate(geo)])

    def _check_rates(self, rates):
        """the rate index of each session of a state in THIS pool (None: no session has a rate); ValueError when the pool lacks one"""
        if rates is None:
            return None
        return np.array([rate_index(self.geometry["sample_rate"], self.rates, r) for r in rates], dtype=np.int32)

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
        ridx = self._check_rates(state.rates)
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
        launch(self.lib, self.dn.device, self.lib.dn_sessions_import, self.handle, ids.ctypes.data_as(C.c_void_p), n, rec.data_ptr(),
               None if sids is None else sids.ctypes.data_as(C.c_void_p))
        self._open[ids] = True
        self._pushes[ids] = state.host_pushes
        for k, s in enumerate(ids):
            self._queue[int(s)] = state.queues[k].copy()
        self._rate[ids] = -1 if ridx is None else ridx
        if self._adapt is not None:          # each session's H(rate) leading floats into this pool's rows (another rate set: another stride)
            idx = torch.from_numpy(ids.astype(np.int64)).to(self.dn.device)
            for t, rows in zip(self._adapt, (state.adapter_in, state.adapter_out)):
                host = np.zeros((n, t.shape[1]), dtype=np.float32)
                for k in range(n if rows is not None else 0):
                    host[k, :rows[k].size] = rows[k]
                t.index_copy_(0, idx, torch.from_numpy(host).to(self.dn.device))
        return [int(s) for s in ids]

    def move(self, slots, other: "SessionPool") -> list:
        """Move the listed sessions to ``other`` (a pool of the same geometry and seed, on any device): they close here and continue
        there, bit for bit.  Returns their slots in ``other``.  Refused, nothing changed, as ``resume``."""
        ids = self._open_ids(slots)
        other._check_compatible(self.geometry, self.seed)
        other._check_rates([self.sample_rate(s) for s in ids])
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
                launch(self.lib, self.dn.device, self.lib.dn_sessions_export, self.handle, ids.ctypes.data_as(C.c_void_p), ids.size, rec.data_ptr())
                launch(self.lib, self.dn.device, self.lib.dn_sessions_import, handle, ids.ctypes.data_as(C.c_void_p), ids.size, rec.data_ptr(), None)
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
        rate = np.full(capacity, -1, dtype=np.int32)
        rate[:keep] = self._rate[:keep]
        self._rate = rate
        if self._adapt is not None:
            grown = self.bank.new_state(capacity)
            for new, old in zip(grown, self._adapt):
                new[:keep] = old[:keep]
            self._adapt = grown
