"""A dn_pipe that changes mode while it carries a stream, on the MI355X (``pytest -m gpu``): head start, Griffin-Lim schedule and split switched
with a hop in flight; depth, hop groups and a restored state switched after a drain.  The header promises the same frames, hx and samples bit
for bit across every such switch, and every test before this one built a fresh pipe, put it in one mode and kept it there.

Cases, the model that places every emitted hop and the yardstick: tests/pipe_cases.py.  Every compared hop is ``torch.equal`` to the hop of a
pipe that is never reconfigured (yardstick A: wave per column, no head start, one flush at the end); the only tolerances are A's own against
float64 over its 20 frames (test_the_never_reconfigured_pipe_against_float64), at the bars of tests/test_gpu_windows.py: waveform
TOL_WAVE_RMS / TOL_WAVE_MAX at scale max(1, RMS of the float64 waveform), hx TOL_RESIDUAL.  Those figures are printed first
(`window-margin ...`, visible with -s; recorded in profiles/pipe_switch_margins.txt).  Batch 5 (four streams a chain workgroup and a tail) and 3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import dsp_cases as dc
import pipe_cases as pc
from test_gpu_parity import TOL_RESIDUAL, _model, dev  # noqa: F401  (dev: the module's fixture)
from test_gpu_windows import check, check_wave

pytestmark = pytest.mark.gpu

F = pc.FRAMES
BATCHES = (5, 3)
SEED = 77                         # of the device-RNG variant of the frame-mode test
DEFAULT_HEAD_START = {512: 8, 1024: 8, 1536: 12}


def _denoiser(dev, n_fft, n_iter=pc.N_ITER):
    from audio_denoising_amd.pipeline import Denoiser
    p = pc.geometry(n_fft)
    return Denoiser(_model(dev, p.num_compressed_bins), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter,
                    window=torch.from_numpy(dc.window(pc.WINDOW, n_fft)))


class Case:
    """the input of one (n_fft, B, sample type) on the device and its yardstick A: E[f], the state and the frame count after the drain"""

    def __init__(self, dev, n_fft, B, s16):
        from audio_denoising_amd import _lib
        from audio_denoising_amd.pipeline import PipelinedStream
        self.n_fft, self.hop, self.B, self.s16 = n_fft, n_fft // 2, B, s16
        self.dn = _denoiser(dev, n_fft)
        sig, inits = pc.stream_input(n_fft)
        sig = sig[:B]
        self.sig = torch.from_numpy(pc.to_s16(sig) if s16 else sig.copy()).to(dev)
        self.inits = [torch.from_numpy(a[:B].copy()).to(dev) for a in inits]
        st = PipelinedStream(self.dn, B)
        st.set_gl_schedule(_lib.DN_GL_WAVE_PER_COLUMN)
        st.set_head_start(0)
        outs = [st.push(self.hop_in(h), init_angles=self.phases(h)) for h in range(F + 1)]
        outs.append(st.flush(s16=s16))
        self.state = st.state()
        torch.cuda.synchronize()
        assert not outs[0].any() and not outs[1].any()           # the priming push; the push that delivers frame 0
        self.E = outs[2:]
        assert len(self.E) == F and not self.E[0].any() and all(bool(e.any()) for e in self.E[1:]) and self.state[3] == F
        assert all(e.dtype == (torch.int16 if s16 else torch.float32) for e in self.E)

    def hop_in(self, h):
        return self.sig[:, h * self.hop:(h + 1) * self.hop].contiguous()

    def phases(self, h):
        """of the frame hop h delivers: frame h - 1 (a priming push draws nothing: any)"""
        return self.inits[max(h - 1, 0)]


@pytest.fixture(scope="module")
def cases(dev):
    made = {}

    def get(n_fft, B, s16=False):
        key = (n_fft, B, s16)
        if key not in made:
            made[key] = Case(dev, n_fft, B, s16)
        return made[key]
    return get


@pytest.fixture(scope="module")
def float64():
    """n_fft -> (emitted (5, F * hop), hx) of pipe_cases.stream64, computed once per geometry; streams are independent: batch 3 is its first rows"""
    made = {}

    def get(n_fft):
        if n_fft not in made:
            made[n_fft] = pc.stream64(n_fft)
        return made[n_fft]
    return get


class GpuStream:
    """pipe_cases.run_script's driver on a PipelinedStream"""

    def __init__(self, case, stream=None):
        from audio_denoising_amd.pipeline import PipelinedStream
        self.c = case
        self.st = PipelinedStream(case.dn, case.B) if stream is None else stream

    def push(self, h):
        return [self.st.push(self.c.hop_in(h), init_angles=self.c.phases(h))]

    def flush(self):
        return list(self.st.flush(s16=self.c.s16).split(self.c.hop, dim=1))

    def push_group(self, idx):
        hops = torch.stack([self.c.hop_in(h) for h in idx])
        return list(self.st.push_group(hops, init_angles=torch.stack([self.c.phases(h) for h in idx])))

    def flush_group(self):
        out, valid = self.st.flush_group(s16=self.c.s16)
        return list(out), valid

    def set_head_start(self, v):
        self.st.set_head_start(v)

    def set_gl_schedule(self, v):
        self.st.set_gl_schedule(v)

    def set_split(self, v):
        self.st.set_split(v)

    def set_depth(self, v):
        self.st.set_depth(v)

    def set_group(self, v):
        self.st.set_group(v)

    def refuse(self, setter, value):
        from audio_denoising_amd._lib import DnError
        with pytest.raises(DnError):
            getattr(self.st, setter)(value)

    def state(self):
        return self.st.state()

    def round_trip(self):
        from audio_denoising_amd.pipeline import PipelinedStream
        ring, ola, hx, frames = self.st.state()
        self.st = PipelinedStream(self.c.dn, self.c.B)
        self.st.load_state(ring, ola, hx, frames)
        return frames


def _check(case, labels, hops, frames):
    torch.cuda.synchronize()
    pc.check_emitted(labels, hops, case.E, frames, equal=torch.equal, nonzero=lambda t: bool(t.any()))


def _same_state(got, want):
    for name, a, b in zip(("ring", "ola", "hx"), got, want):
        assert torch.equal(a, b), name
    assert got[3] == want[3], "frames"


# ------------------------------------------------------------------ yardstick A against float64
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_fft", dc.N_FFTS)
def test_the_never_reconfigured_pipe_against_float64(cases, float64, n_fft, B):
    """Yardstick A, 20 frames of a streaming pipe with six Griffin-Lim iterations each, against the float64 stream: what bit-identity to A is
    worth.  (The existing stream tests run 2 to 4 hops.)"""
    c = cases(n_fft, B)
    ref, hx = float64(n_fft)
    got = torch.cat(c.E, dim=1).cpu().numpy()
    assert np.abs(ref[:B, c.hop:]).max() > 0.1
    check_wave("stream", got, ref[:B], n_fft, n_fft=n_fft, B=B, frames=F)
    check("switch_hx", float(np.abs(c.state[2].cpu().numpy() - hx[:B]).max()), TOL_RESIDUAL, n_fft=n_fft, B=B, frames=F)


# ------------------------------------------------------------------ a. streaming, n_fft 1024: one stream through every mode
@pytest.mark.parametrize("s16", [False, True], ids=["float32", "int16"])
@pytest.mark.parametrize("B", BATCHES)
def test_one_stream_through_every_mode(cases, B, s16):
    """pipe_cases.script_1024 on ONE PipelinedStream: head start 8 -> 0 -> 3 and wave per column <-> wave per stream with a hop in flight (a
    chain parked under one schedule is resumed under the other, both ways); depth 3 and back; groups of four and of two behind single pushes
    (*hops_valid 4 and 2: the ring was primed long before), the wave-per-column schedule refused on the group pipe; split hops switched on and
    off with a hop in flight.  Every filler hop exactly zero, every other hop E[f], every frame once, the same state after the last drain."""
    from audio_denoising_amd import _lib
    c = cases(1024, B, s16)
    d = GpuStream(c)
    labels, hops, kept = pc.run_script(pc.script_1024(_lib), d, pc.EmitModel(1))
    _check(c, labels, hops, range(F))
    _same_state(d.state(), c.state)
    assert kept[pc.SNAPSHOT][1] == 10 and kept[pc.SNAPSHOT][0][3] == 9


# ------------------------------------------------------------------ c. resume into another mode
@pytest.mark.parametrize("order", ["set_group first", "load_state first"])
@pytest.mark.parametrize("B", BATCHES)
def test_resume_into_a_group_pipe(cases, B, order):
    """The snapshot behind script_1024's deep pipe, loaded into a FRESH pipe that is (or then becomes) a group pipe: the rest of the script emits
    the same hops and ends in the same state, and the first group flush reports 4 valid hops (a restored ring counts as primed on either path)."""
    from audio_denoising_amd import _lib
    c = cases(1024, B)
    first = GpuStream(c)
    _, _, kept = pc.run_script(pc.script_1024_head(_lib), first, pc.EmitModel(1))
    (ring, ola, hx, frames), delivered = kept[pc.SNAPSHOT]
    assert (frames, delivered) == (9, 10)
    d = GpuStream(c)
    if order == "set_group first":
        d.set_group(4)
        d.st.load_state(ring, ola, hx, frames)
    else:
        d.st.load_state(ring, ola, hx, frames)
        d.set_group(4)
    model = pc.EmitModel(1)
    model.load_state(frames)
    labels, hops, _ = pc.run_script(pc.script_1024_tail(_lib), d, model, hop0=delivered)       # (its first call, set_group(4), changes nothing)
    _check(c, labels, hops, range(frames, F))
    _same_state(d.state(), c.state)


# ------------------------------------------------------------------ d. n_fft 512 and 1536
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n_fft", [512, 1536])
def test_head_start_toggles_refusals_and_a_round_trip_where_only_the_per_column_form_exists(cases, n_fft, B):
    """pipe_cases.script_per_column_only: default head start -> 0 -> 5 -> default with a hop in flight (at 1536 the front workgroup's spare wave
    draws the head start's phases into the slot), set_depth(2) / set_group(2) / wave per stream / split refused in mid-stream without a trace,
    one state() / load_state round trip into a fresh pipe."""
    from audio_denoising_amd import _lib
    c = cases(n_fft, B)
    d = GpuStream(c)
    labels, hops, _ = pc.run_script(pc.script_per_column_only(_lib, DEFAULT_HEAD_START[n_fft]), d, pc.EmitModel(1))
    _check(c, labels, hops, range(F))
    _same_state(d.state(), c.state)


# ------------------------------------------------------------------ b. frame mode, n_fft 1024
def _frame_script(lib):
    col, per = lib.DN_GL_WAVE_PER_COLUMN, lib.DN_GL_WAVE_PER_STREAM
    return [("submit",), ("set_head_start", 0), ("submit",), ("set_gl_schedule", per), ("submit",), ("set_head_start", 3), ("submit",),
            ("set_gl_schedule", col), ("submit",), ("set_gl_schedule", per), ("flush",),                               # frames 0 .. 4
            ("set_depth", 3), ("submit",), ("submit",), ("submit",), ("submit",), ("flush",), ("set_depth", 1),          # 5 .. 8
            ("set_group", 4), ("refuse", "set_gl_schedule", col), ("submit_group", 4), ("submit",), ("flush",),          # 9 .. 13: submit = a group of one
            ("set_group", 2), ("submit_group", 2), ("submit_group", 1), ("flush",), ("set_group", 0),                    # 14 .. 16
            ("set_head_start", 0), ("set_gl_schedule", per), ("set_split", lib.DN_SPLIT_ON), ("submit",), ("submit",),
            ("set_split", lib.DN_SPLIT_OFF), ("submit",), ("set_split", lib.DN_SPLIT_ON), ("flush",)]                    # 17 .. 19


@pytest.mark.parametrize("phases", ["device RNG", "injected"])
@pytest.mark.parametrize("B", BATCHES)
def test_frame_mode_through_every_mode(dev, B, phases):
    """The same kinds of switch on one HopPipeline (submit / submit_group / flush), 20 frames: out and hx of a never-reconfigured wave-per-column
    pipe bit for bit and the same counters().  With device-RNG phases (n_iter 5) that also says that frame f drew from seed + f across every
    switch: one frame off and its waveform differs."""
    from audio_denoising_amd import _lib
    from audio_denoising_amd._lib import DnError
    from audio_denoising_amd.pipeline import HopPipeline
    rng = phases == "device RNG"
    dn = _denoiser(dev, 1024, 5 if rng else pc.N_ITER)
    sig, inits = pc.stream_input(1024)
    frames = torch.from_numpy(np.stack([sig[:B, f * 512:f * 512 + 1024] for f in range(F)])).to(dev)
    ia = None if rng else torch.from_numpy(np.stack([a[:B] for a in inits])).to(dev)

    def angles(f, n=None):
        return None if ia is None else (ia[f] if n is None else ia[f:f + n])

    want, want_hx = torch.empty(F, B, 1024, device=dev), dn.init_hx(B)
    ref = HopPipeline(dn, B)
    ref.set_gl_schedule(_lib.DN_GL_WAVE_PER_COLUMN)
    ref.set_head_start(0)
    for f in range(F):
        ref.submit(frames[f], want_hx, want[f], seed=SEED, init_angles=angles(f))
    ref.flush()
    got, hx = torch.full((F, B, 1024), float("nan"), device=dev), dn.init_hx(B)
    pipe = HopPipeline(dn, B)
    f = 0
    for op in _frame_script(_lib):
        if op[0] == "submit":
            pipe.submit(frames[f], hx, got[f], seed=SEED, init_angles=angles(f))
            f += 1
        elif op[0] == "submit_group":
            pipe.submit_group(frames[f:f + op[1]], hx, got[f:f + op[1]], seed=SEED, init_angles=angles(f, op[1]))
            f += op[1]
        elif op[0] == "flush":
            pipe.flush()
        elif op[0] == "refuse":
            with pytest.raises(DnError):
                getattr(pipe, op[1])(op[2])
        else:
            getattr(pipe, op[0])(op[1])
    assert f == F
    torch.cuda.synchronize()
    assert float(want.abs().max()) > 0.1
    for k in range(F):
        assert torch.equal(got[k], want[k]), f"frame {k}"
    assert torch.equal(hx, want_hx)
    assert pipe.counters() == ref.counters() and ref.counters()[1:] == (F, False)
    if rng:          # (the seed sequence is really in the result: frame 1 of a pipe that starts at seed + 1 is not frame 1 above)
        other, o_hx, o = HopPipeline(dn, B), dn.init_hx(B), torch.empty(2, B, 1024, device=dev)
        for k in range(2):
            other.submit(frames[k], o_hx, o[k], seed=SEED + 1)
        other.flush()
        torch.cuda.synchronize()
        assert not torch.equal(o[1], want[1])


# ------------------------------------------------------------------ e. strides of the group calls
def _spread(rows, stride, fill):
    """rows (H, ...) -> a flat buffer with row h at h * stride and `fill` everywhere else"""
    H, n = rows.shape[0], rows[0].numel()
    assert stride >= n
    flat = torch.full((H * stride,), fill, dtype=rows.dtype, device=rows.device)
    flat.view(H, stride)[:, :n] = rows.reshape(H, n)
    return flat


def _gather(flat, H, n, stride, fill):
    """-> the rows of such a buffer; the gaps must still hold `fill`"""
    v = flat.view(H, stride)
    assert bool((v[:, n:] == fill).all()), "a gap between two rows of a group was written"
    return v[:, :n]


def _packed(dn, angles, B):
    """(H, B, K, 3) complex64 -> (H, B, 3, K, 2) float32 as the C ABI takes it"""
    return torch.stack([dn._angles_ptr(a, B)[0] for a in angles])


def test_frame_groups_with_rows_that_are_not_back_to_back(dev):
    """dn_pipe_submit_group called on the C ABI with frames, out and init_angles rows 64, 128 and 192 floats further apart than a row is long
    (the Python layer only ever passes the stride of a contiguous stack): the contiguous call's frames and hx bit for bit, the gaps untouched.
    The gaps of the inputs hold NaN: a read that lands there shows."""
    from audio_denoising_amd.pipeline import HopPipeline
    B, H, n_groups = 5, 4, 2
    dn = _denoiser(dev, 1024)
    sig, inits = pc.stream_input(1024)
    frames = torch.from_numpy(np.stack([sig[:B, f * 512:f * 512 + 1024] for f in range(H * n_groups)])).to(dev)
    ia = torch.from_numpy(np.stack([a[:B] for a in inits[:H * n_groups]])).to(dev)
    want, want_hx = torch.empty_like(frames), dn.init_hx(B)
    a = HopPipeline(dn, B)
    a.set_group(H)
    for g in range(n_groups):
        a.submit_group(frames[g * H:(g + 1) * H], want_hx, want[g * H:(g + 1) * H], init_angles=ia[g * H:(g + 1) * H])
    a.flush()
    row, arow = B * 1024, B * 3 * 513 * 2
    s_in, s_out, s_ia = row + 64, row + 128, arow + 192
    b, hx, outs, keep = HopPipeline(dn, B), dn.init_hx(B), [], []
    b.set_group(H)
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for g in range(n_groups):
            fin = _spread(frames[g * H:(g + 1) * H], s_in, float("nan"))
            ain = _spread(_packed(dn, ia[g * H:(g + 1) * H], B), s_ia, float("nan"))
            out = torch.full((H * s_out,), 12345.0, device=dev)
            b.lib.check(b.lib.dn_pipe_submit_group(b.handle, fin.data_ptr(), s_in, hx.data_ptr(), out.data_ptr(), s_out, ain.data_ptr(), s_ia, 0, 0,
                                                   H, dn.n_iter, dn.momentum, st))
            outs.append(out)
            keep += [fin, ain]
    b.flush()
    torch.cuda.synchronize()
    assert float(want.abs().max()) > 0.1
    for g in range(n_groups):
        assert torch.equal(_gather(outs[g], H, row, s_out, 12345.0), want[g * H:(g + 1) * H].reshape(H, row)), f"group {g}"
    assert torch.equal(hx, want_hx)


@pytest.mark.parametrize("B,H,s16", [(5, 4, False), (3, 2, True)], ids=["float32-B5-H4", "int16-B3-H2"])
def test_streaming_groups_with_rows_that_are_not_back_to_back(cases, dev, B, H, s16):
    """dn_pipe_stream_push_group / _flush_group on the C ABI with hop_in, hop_out and init_angles rows 64, 128 and 192 elements (of their type)
    further apart than B * hop: the contiguous calls' hops and state bit for bit, the gaps of the outputs untouched."""
    from audio_denoising_amd.pipeline import PipelinedStream
    c = cases(1024, B, s16)
    dn, n_groups = c.dn, 2
    groups = [list(range(g * H, (g + 1) * H)) for g in range(n_groups)]
    a = GpuStream(c)
    a.set_group(H)
    want = [a.push_group(idx) for idx in groups]
    tail, valid = a.flush_group()
    want_state = a.state()
    row, arow = B * c.hop, B * 3 * 513 * 2
    s_in, s_out, s_ia = row + 64, row + 128, arow + 192
    fill_in, fill_out = (32000, -12345) if s16 else (float("nan"), 12345.0)
    b = PipelinedStream(dn, B)
    b.set_group(H)
    got, keep = [], []
    with torch.cuda.device(dev):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for idx in groups:
            hin = _spread(torch.stack([c.hop_in(h) for h in idx]), s_in, fill_in)
            ain = _spread(_packed(dn, [c.phases(h) for h in idx], B), s_ia, float("nan"))
            out = torch.full((H * s_out,), fill_out, dtype=hin.dtype, device=dev)
            b.lib.check(b.lib.dn_pipe_stream_push_group(b.handle, hin.data_ptr(), s_in, int(s16), out.data_ptr(), s_out, int(s16), ain.data_ptr(), s_ia,
                                                        b.seed, b.stream_id0, dn.n_iter, dn.momentum, st))
            got.append(out)
            keep += [hin, ain]
        out = torch.full((H * s_out,), fill_out, dtype=got[0].dtype, device=dev)
        n_valid = C.c_int32(-1)
        b.lib.check(b.lib.dn_pipe_stream_flush_group(b.handle, out.data_ptr(), s_out, int(s16), C.byref(n_valid), st))
    torch.cuda.synchronize()
    assert valid == H and n_valid.value == H
    for g, w in zip(got + [out], want + [tail]):
        assert torch.equal(_gather(g, H, row, s_out, fill_out), torch.stack(w).reshape(H, row))
    assert bool(torch.stack(tail).any())
    _same_state(b.state(), want_state)
