"""Shared cases of the pipe-switch tests (tests/test_emu_pipe_switch.py, tests/test_gpu_pipe_switch.py, the seed table's check in
tests/test_oracle_dsp.py): a dn_pipe that changes mode -- head start, Griffin-Lim schedule, split, depth, hop groups, a restored state -- while it
carries a stream.  TEST INFRASTRUCTURE; nothing here touches a kernel.

Three parts:
  * the input: B streams of noise at dsp_cases.HOP_LEVEL, window "asym", geometry dsp_cases.HOP_GEOMETRY[n_fft], injected phases from a
    seeded numpy generator; F = 20 frames = 21 pushes (stream_input);
  * EmitModel: what every call on a streaming pipe emits -- for each emitted hop a frame index or FILLER -- written from the rules of
    include/dn_denoise.h, not from any output;
  * run_script / check_emitted: a script of calls walked through a pipe (the `driver` the test supplies) and through the model side by side,
    and the comparison of what came out with the yardstick's hops E[f].

The yardstick (A) is one pipe that is never reconfigured: wave per column, no head start, one flush at the end.  Frame f's hop E[f] is
what push f + 2 emits (push 0 primes the ring at n_fft = 2 hop, push f + 1 delivers frame f, the next launch finishes it); the flush emits
E[F - 1].  E[0] is the overlap-add line before any frame was added: zeros.  A is itself held to float64 (dsp_cases.stream64) by the GPU
tier, once per geometry, which is what makes twenty hops of bit-identity to A mean something.

Conditioning.  Six Griffin-Lim iterations already amplify rounding by a frame-dependent factor with a heavy tail (dsp_cases.GL32_SEED_K has the
long form of this).  A batch is used only if the float64 stream alone moves no stream by more than 1e-4 RMS (at scale max(1, RMS of the
stream)) when the signal is perturbed by 1e-7 x N(0, 1) relative, in two draws: SEED_K holds, per n_fft, the first k = 0, 1, 2 .. whose batch
does (first_well_conditioned_k).  Computed from the reference alone; tests/test_oracle_dsp.py derives it again on the CPU.
"""
import numpy as np

import dsp_cases as dc

WINDOW = "asym"
BATCH, FRAMES, N_ITER = 5, 20, 6
# n_fft -> k of the first well-conditioned candidate batch (noise seed 900 + k, phases from default_rng(901 + k))
SEED_K = {512: 0, 1024: 0, 1536: 0}
FILLER = None
SNAPSHOT = "after the deep pipe"          # the state script_1024 keeps: 10 hops delivered, 9 frames done


def geometry(n_fft):
    from oracle import pipeline_ref
    sr, n_mels = dc.HOP_GEOMETRY[n_fft]
    return pipeline_ref.Params(sr, n_fft, n_fft // 2, n_mels)


def stream_input(n_fft, k=None, B=BATCH, F=FRAMES):
    """-> (signal (B, (F + 1) * hop) fp32, F arrays (B, K, 3) complex64 of initial phases) of candidate batch k (default: the table's)"""
    k = SEED_K[n_fft] if k is None else k
    sig = dc.noise((B, (F + 1) * (n_fft // 2)), 900 + k, dc.HOP_LEVEL)
    rg = np.random.default_rng(901 + k)
    K = n_fft // 2 + 1
    return sig, [(rg.random((B, K, 3)) + 1j * rg.random((B, K, 3))).astype(np.complex64) for _ in range(F)]


def to_s16(sig):
    """the same streams as int16 PCM at RMS ~ 3000 (the int16 runs have a yardstick A of their own)"""
    return np.clip(np.rint(sig * (3000.0 / dc.HOP_LEVEL)), -32767, 32767).astype(np.int16)


def stream64(n_fft, k=None, signal=None):
    """dsp_cases.stream64 of the batch -> (emitted (B, F * hop) float64: frame f's hop E[f] at [f * hop, (f + 1) * hop), hx float64)"""
    sig, inits = stream_input(n_fft, k)
    return dc.stream64(sig if signal is None else signal, inits, geometry(n_fft), dc.window(WINDOW, n_fft), N_ITER)


def conditioning(n_fft, k, trials=2, relative=1e-7):
    """-> (worst move of a stream of the float64 emitted samples in RMS at scale max(1, RMS of the stream), worst move of hx in max-abs) when the
    signal is perturbed by `relative` x N(0, 1), over `trials` draws"""
    sig, _ = stream_input(n_fft, k)
    ref, hx = stream64(n_fft, k)
    scale = np.maximum(1.0, np.sqrt(np.mean(ref ** 2, axis=1)))
    rg = np.random.default_rng(1)
    worst, worst_hx = 0.0, 0.0
    for _ in range(trials):
        y, h = stream64(n_fft, k, signal=sig.astype(np.float64) * (1.0 + relative * rg.standard_normal(sig.shape)))
        worst = max(worst, float((np.sqrt(np.mean((y - ref) ** 2, axis=1)) / scale).max()))
        worst_hx = max(worst_hx, float(np.abs(h - hx).max()))
    return worst, worst_hx


def batch_is_well_conditioned(n_fft, k, limit=1e-4):
    return conditioning(n_fft, k)[0] <= limit


def first_well_conditioned_k(n_fft, k_max=8):
    return next(k for k in range(k_max) if batch_is_well_conditioned(n_fft, k))


# ------------------------------------------------------------------ what each call emits
class EmitModel:
    """The emitted hops of a streaming dn_pipe by the header's rules.  Every method returns the list of hops its call emits: a frame index
    (that frame's hop E[f]) or FILLER (a zero hop).
      * the first n_fft / hop - 1 pushes only fill the ring; a restored ring counts as primed (load_state);
      * at depth D the hop of a frame is complete after the D-th launch that follows the one that delivered it (pushes and single flushes are
        launches): a push emits the frame delivered D pushes earlier if it is still pending, zeros otherwise; dn_pipe_stream_flush likewise
        emits the oldest pending hop once it is due, or zeros;
      * push_group on a pipe with P frames pending emits H - P zero hops first, then the P hops in order;
      * flush_group emits the P pending hops first and zeros behind them, and *hops_valid == P;
      * set_depth / set_group want a drained pipe."""

    def __init__(self, prime):
        self.prime, self.pushes, self.next, self.launch = prime, 0, 0, 0
        self.depth, self.group = 1, 0
        self.flight = []                  # (frame, launch that delivered it), oldest first

    def _deliver(self):
        if self.pushes >= self.prime:
            self.flight.append((self.next, self.launch))
            self.next += 1
        self.pushes += 1

    def _due(self):
        if self.flight and self.flight[0][1] + self.depth <= self.launch:
            return self.flight.pop(0)[0]
        return FILLER

    def push(self):
        assert self.group == 0
        self.launch += 1
        out = [self._due()]
        self._deliver()
        return out

    def flush(self):
        """PipelinedStream.flush: `depth` calls of dn_pipe_stream_flush"""
        assert self.group == 0
        out = []
        for _ in range(self.depth):
            self.launch += 1
            out.append(self._due())
        return out

    def push_group(self):
        H, pending = self.group, [f for f, _ in self.flight]
        assert 0 < H and len(pending) <= H
        self.flight = []
        self.launch += 1
        for _ in range(H):
            self._deliver()
        return [FILLER] * (H - len(pending)) + pending

    def flush_group(self):
        """-> (hops, hops_valid)"""
        H, pending = self.group, [f for f, _ in self.flight]
        assert 0 < H and len(pending) <= H
        self.flight = []
        self.launch += 1
        return pending + [FILLER] * (H - len(pending)), len(pending)

    def set_depth(self, depth):
        assert not self.flight and self.group == 0
        self.depth = depth

    def set_group(self, hops):
        assert not self.flight and self.depth == 1
        self.group = hops

    def load_state(self, frames):
        self.pushes, self.next, self.flight = self.prime, frames, []


SETTERS = ("set_head_start", "set_gl_schedule", "set_split", "set_depth", "set_group")


def run_script(script, driver, model, hop0=0):
    """Walks `script` through `driver` (the pipe under test) and `model` side by side.  Operations:
         ("push",)               one hop in, one hop out            ("flush",)              PipelinedStream.flush (`depth` hops out)
         ("push_group",)         H hops in, H out                   ("flush_group", valid)  H hops out; *hops_valid must be `valid`
         (setter, value)         one of SETTERS, must succeed       ("refuse", setter, value)  must raise the library's error
         ("state", key)          driver.state() kept under `key` with the number of hops delivered so far
         ("round_trip",)         driver.round_trip(): state() -> a fresh pipe -> load_state()
       The driver's push(h) / push_group([h ..]) take indices of hops of the input, counted from `hop0`; its calls return one array per emitted hop.
       -> (labels, hops, kept): the model's label and the pipe's array for every emitted hop, in order, and the kept states"""
    labels, hops, kept = [], [], {}
    h = hop0
    for op in script:
        name = op[0]
        if name == "push":
            labels += model.push()
            hops += driver.push(h)
            h += 1
        elif name == "flush":
            labels += model.flush()
            hops += driver.flush()
        elif name == "push_group":
            H = model.group
            labels += model.push_group()
            hops += driver.push_group(list(range(h, h + H)))
            h += H
        elif name == "flush_group":
            want, valid = model.flush_group()
            assert valid == op[1], "the script's own count disagrees with the model"
            got, got_valid = driver.flush_group()
            assert got_valid == valid, f"*hops_valid is {got_valid}; {valid} hops of this flush carry samples (after {h - hop0} hops)"
            labels += want
            hops += got
        elif name in SETTERS:
            getattr(driver, name)(op[1])
            if name in ("set_depth", "set_group"):
                getattr(model, name)(op[1])
        elif name == "refuse":
            driver.refuse(op[1], op[2])
        elif name == "state":
            kept[op[1]] = (driver.state(), h)
        elif name == "round_trip":
            model.load_state(driver.round_trip())
        else:
            raise AssertionError(op)
        assert len(labels) == len(hops), op
    return labels, hops, kept


def check_emitted(labels, hops, E, frames, equal=np.array_equal, nonzero=lambda a: bool(np.asarray(a).any())):
    """every filler hop exactly zero, every other hop E[f] bit for bit, every frame of `frames` emitted exactly once"""
    for i, (f, y) in enumerate(zip(labels, hops)):
        if f is FILLER:
            assert not nonzero(y), f"emitted hop {i} is a filler by the header's rules and is not zero"
        else:
            assert equal(y, E[f]), f"emitted hop {i} is frame {f}'s by the header's rules and is not the never-reconfigured pipe's"
    assert sorted(f for f in labels if f is not FILLER) == list(frames), "every frame's hop comes out exactly once"


# ------------------------------------------------------------------ the scripts
def script_1024_head(lib):
    """n_fft 1024, hops 0 .. 9 = frames 0 .. 8 of script_1024, up to the snapshot (batch <= 256: the pipe starts with head start 8, wave per column)"""
    col, per = lib.DN_GL_WAVE_PER_COLUMN, lib.DN_GL_WAVE_PER_STREAM
    return [
        # with a hop in flight: head start and Griffin-Lim schedule (frames 0 .. 4)
        ("push",), ("push",),                                          # frame 0 parked after 8 iterations by the default pipe
        ("set_head_start", 0), ("push",),                              # ... resumed by a launch that parks nothing
        ("set_gl_schedule", per), ("push",),                           # frame 1: a whole chain, a wavefront per stream
        ("set_head_start", 3), ("push",),                              # frame 3 parked after 3 iterations under the per-stream schedule
        ("set_gl_schedule", col), ("push",),                           # ... resumed a wavefront per column; frame 4 parked by that launch
        ("set_gl_schedule", per), ("flush",),                          # ... and resumed by the per-stream chain
        # a deep pipe (frames 5 .. 8)
        ("set_depth", 3), ("push",), ("push",), ("push",), ("push",), ("flush",), ("set_depth", 1),
        ("state", SNAPSHOT),
    ]


def script_1024(lib):
    """n_fft 1024, 21 hops = frames 0 .. 19 through every mode of a streaming pipe"""
    return script_1024_head(lib) + script_1024_tail(lib)


def script_1024_tail(lib):
    """the rest of script_1024 from the snapshot on: hops 10 .. 20, frames 9 .. 19"""
    col, per = lib.DN_GL_WAVE_PER_COLUMN, lib.DN_GL_WAVE_PER_STREAM
    return [
        # groups after single pushes (frames 9 .. 16): every hop of both flushes carries samples
        ("set_group", 4), ("refuse", "set_gl_schedule", col), ("push_group",), ("flush_group", 4),
        ("set_group", 2), ("push_group",), ("refuse", "set_gl_schedule", col), ("push_group",), ("flush_group", 2),
        ("set_group", 0),
        # split hops, switched with a hop in flight (frames 17 .. 19)
        ("set_head_start", 0), ("set_gl_schedule", per), ("set_split", lib.DN_SPLIT_ON), ("push",), ("push",),
        ("set_split", lib.DN_SPLIT_OFF), ("push",),
        ("set_split", lib.DN_SPLIT_ON), ("flush",),
    ]


def script_per_column_only(lib, default_head_start):
    """n_fft 512 and 1536: the head start toggled with a hop in flight, the schedules these sizes refuse asked for in mid-stream, one
    state() / load_state round trip into a fresh pipe; 21 hops = frames 0 .. 19"""
    refusals = [("refuse", "set_depth", 2), ("refuse", "set_group", 2), ("refuse", "set_gl_schedule", lib.DN_GL_WAVE_PER_STREAM),
                ("refuse", "set_split", lib.DN_SPLIT_ON)]
    return ([("push",), ("push",), ("set_head_start", 0), ("push",), ("push",), ("set_head_start", 5), ("push",), ("push",),
             ("set_head_start", default_head_start), ("push",)] + refusals + [("push",), ("push",), ("push",), ("push",), ("flush",),
            ("round_trip",), ("push",), ("set_head_start", 0), ("push",)] + refusals + [("push",), ("set_head_start", 5), ("push",),
            ("push",), ("set_head_start", default_head_start)] + [("push",)] * 5 + [("flush",)])
