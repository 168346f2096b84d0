"""Rate banks on the MI355X (``pytest -m gpu``): the cases of tests/ratebank_cases.py on the device (both sides, float32 and int16, bit for bit
against dn_resample_push per session; float64 within the resampler's bound; fresh state; refusals), then ``SessionPool(rates=...)`` end to end:
``recv`` against the manual composition ResampleStream -> one-session pool -> ResampleStream per session, and the session state across
suspend / save / load / resume, resize and a refused resume.  Plan: n_fft 512 / hop 256 / 64 mels at 16 kHz, n_iter 2."""
import ctypes as C

import numpy as np
import pytest
import torch

import ratebank_cases as rb
from oracle import pipeline_ref
from test_gpu_sessions import _denoiser

pytestmark = pytest.mark.gpu

N_ITER = 2


class DevMem:
    """the memory adapter of ratebank_cases on the device: torch tensors"""

    def dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()

    def ptr(self, h):
        return None if h is None else C.c_void_p(h.data_ptr())

    def host(self, h):
        torch.cuda.synchronize()
        return h.cpu().numpy()


MEM = DevMem()


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from audio_denoising_amd import _lib
    return _lib.get_lib()


@pytest.fixture(scope="module")
def dev(lib):
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def float32_runs(lib):
    return {(name, side): rb.run_script(lib, MEM, bank, side, False) for name, bank in rb.BANKS.items() for side in (rb.SIDE_IN, rb.SIDE_OUT)}


@pytest.mark.parametrize("name", sorted(rb.BANKS))
@pytest.mark.parametrize("side", [rb.SIDE_IN, rb.SIDE_OUT])
def test_float32_rows_and_state_equal_resample_push_bit_for_bit(float32_runs, name, side):
    assert set(float32_runs[(name, side)]) == set(rb.BANKS[name].slots)


@pytest.mark.parametrize("name", sorted(rb.BANKS))
@pytest.mark.parametrize("side", [rb.SIDE_IN, rb.SIDE_OUT])
def test_int16_rows_and_state_equal_resample_push_bit_for_bit(lib, name, side):
    rb.run_script(lib, MEM, rb.BANKS[name], side, True)


@pytest.mark.parametrize("name", sorted(rb.BANKS))
@pytest.mark.parametrize("side", [rb.SIDE_IN, rb.SIDE_OUT])
def test_against_float64(float32_runs, name, side):
    rb.check_float64(rb.BANKS[name], side, float32_runs[(name, side)])


@pytest.mark.parametrize("name", sorted(rb.BANKS))
def test_geometry(lib, name):
    rb.check_geometry(lib, rb.BANKS[name])


@pytest.mark.parametrize("name", sorted(rb.BANKS))
def test_fresh_state_emits_zeros_and_plan_rows_are_the_conversion_copy(lib, name):
    rb.check_fresh(lib, MEM, rb.BANKS[name])


def test_create_refusals_name_the_rule(lib):
    rb.check_create_refusals(lib)


def test_call_refusals_change_nothing(lib):
    rb.check_call_refusals(lib, MEM)


# ---------------------------------------------------------------------------------------------------------------- the pool, end to end
P512 = pipeline_ref.Params(16000, 512, 256, 64)
P1024 = pipeline_ref.PARAMS_S          # 16 kHz, n_fft 1024, hop 512, 80 mels
RATES = (8000, 48000)


def _dn(dev, p):
    dn = _denoiser(dev, p)
    dn.n_iter = N_ITER
    return dn


def _frames(rate, n_frames, seed):
    """int16 frames of 10 ms at `rate`"""
    rng = np.random.default_rng(seed)
    return [np.trunc(0.2 * rng.uniform(-1, 1, rate // 100) * 32767).astype(np.int16) for _ in range(n_frames)]


class Alone:
    """One session by the manual composition: ResampleStream(down, 1) -> a one-session pool of the same seed and stream id ->
    ResampleStream(up, 1), fed its samples alone through the same host conventions as ``SessionPool.recv`` (int16 / 32767 on the host, whole
    hops queued, priming rows dropped, clip * 32767 truncate on the host)."""

    def __init__(self, dn, rate, sid, seed):
        from audio_denoising_amd import SessionPool
        from audio_denoising_amd.transforms import Resample, ResampleStream
        self.dn, self.pool = dn, SessionPool(dn, 1, seed=seed)
        self.pool.open(sid)
        self.down = ResampleStream(Resample(rate, dn.sample_rate), 1)
        self.up = ResampleStream(Resample(dn.sample_rate, rate), 1)
        self.cin = dn.hop // self.down.resample.n * self.down.resample.o
        self.queue = np.zeros(0, np.float32)
        self.pushes = 0

    def recv(self, frame16):
        self.queue = np.concatenate([self.queue, frame16.astype(np.float32) / np.iinfo(np.int16).max])
        out = []
        while self.queue.size >= self.cin:
            x = torch.from_numpy(self.queue[:self.cin].copy()).to(self.dn.device)[None]
            self.queue = self.queue[self.cin:]
            y = self.up.push(self.pool.push([0], self.down.push(x)))
            if self.pushes >= self.pool.prime:
                out.append(y[0].cpu().numpy())
            self.pushes += 1
        if not out:
            return None
        return (np.clip(np.concatenate(out), -1.0, 1.0) * np.iinfo(np.int16).max).astype(np.int16)


def _run_pool(dev, p, joins, n_frames, seed=9):
    """joins: [(rate, stream id, the 10 ms tick it joins at)].  Feeds every live session one 10 ms int16 frame a tick through ONE recv call and
    the same frames through Alone (rated sessions) or a pool built without rates (plan-rate sessions); compares every returned chunk."""
    from audio_denoising_amd import SessionPool
    dn = _dn(dev, p)
    pool = SessionPool(dn, len(joins) + 1, seed=seed, rates=RATES)
    plain = SessionPool(dn, len(joins) + 1, seed=seed)
    frames = [_frames(rate, n_frames, 100 + k) for k, (rate, _, _) in enumerate(joins)]
    slot, ref, hops_run = {}, {}, 0
    for t in range(n_frames):
        for k, (rate, sid, join) in enumerate(joins):
            if join == t:
                slot[k] = pool.open(sid, sample_rate=rate)
                ref[k] = Alone(dn, rate, sid, seed) if rate != p.sample_rate else plain.open(sid)
        live = [k for k in slot if joins[k][2] <= t]
        got = pool.recv({slot[k]: frames[k][t] for k in live})
        for k in live:
            f = frames[k][t]
            if joins[k][0] == p.sample_rate:
                want = plain.recv({ref[k]: f})[ref[k]]
            else:
                want = ref[k].recv(f)
                if want is None:          # no hop ran for the session: the passthrough of its own chunk
                    want = (np.clip(f.astype(np.float32) / 32767, -1.0, 1.0) * 32767).astype(np.int16)
                else:
                    hops_run += 1
            assert got[slot[k]].dtype == np.int16 and np.array_equal(got[slot[k]], want), (k, t)
    return pool, slot, hops_run


def test_pool_recv_equals_the_manual_composition_per_session(dev):
    joins = [(48000, 31, 0), (16000, 32, 0), (8000, 33, 2), (48000, 34, 5), (16000, 35, 7)]
    n_frames = 12 * 256 * 100 // 16000 + 2          # about 12 hops of 256 samples at 16 kHz in 10 ms frames
    pool, slot, hops_run = _run_pool(dev, P512, joins, n_frames)
    assert hops_run >= 20
    assert pool.chunk(slot[0]) == (768, 768) and pool.chunk(slot[2]) == (128, 128) and pool.chunk(slot[1]) == (256, 256)
    assert pool.delay(slot[0]) == 42 and pool.delay(slot[1]) == 0
    with pytest.raises(ValueError, match="push_rated"):
        pool.push([slot[0]], torch.zeros(1, 256, device=dev))
    with pytest.raises(ValueError, match="rates="):
        pool.open(sample_rate=44100)


def test_pool_recv_at_n_fft_1024(dev):
    _, _, hops_run = _run_pool(dev, P1024, [(48000, 5, 0)], 4 * 512 * 100 // 16000 + 1)
    assert hops_run >= 2


# ---------------------------------------------------------------------------------------------------------------- session state
def _feed(pool, slots, frames, t0, t1):
    out = {s: [] for s in slots}
    for t in range(t0, t1):
        got = pool.recv({s: frames[s][t] for s in slots})
        for s in slots:
            out[s].append(got[s])
    return {s: np.concatenate(v) for s, v in out.items()}


def test_suspend_save_load_resume_into_a_larger_pool_with_more_rates(dev, tmp_path):
    from audio_denoising_amd import SessionPool, SessionState
    dn = _dn(dev, P512)
    seed = 4
    rates_of = [24000, 12000, 16000, 24000]
    never, a = SessionPool(dn, 4, seed=seed, rates=(24000, 12000)), SessionPool(dn, 4, seed=seed, rates=(24000, 12000))
    b = SessionPool(dn, 7, seed=seed, rates=(48000, 12000, 8000, 24000))          # a superset in another order: other indices, another stride
    assert b.bank.stride != a.bank.stride
    for pool in (never, a):
        for k, r in enumerate(rates_of):
            assert pool.open(50 + k, sample_rate=r) == k
    frames = {k: _frames(r, 14, 200 + k) for k, r in enumerate(rates_of)}
    first = _feed(never, range(4), frames, 0, 7)
    assert all(np.array_equal(first[k], v) for k, v in _feed(a, range(4), frames, 0, 7).items())
    st = a.suspend([3, 0, 1])
    assert any(q.size for q in st.queues) and st.rates.tolist() == [24000, 24000, 12000] and len(st.adapter_in[0]) == 22
    st.save(tmp_path / "rated.npz")
    b.open(999)          # (slot 0 of b is taken: the sessions land elsewhere)
    new = b.resume(SessionState.load(tmp_path / "rated.npz"))
    assert new == [1, 2, 3] and [b.sample_rate(s) for s in new] == [24000, 24000, 12000]
    want = _feed(never, [3, 0, 1], frames, 7, 14)
    got = _feed(b, new, {n: frames[o] for n, o in zip(new, [3, 0, 1])}, 7, 14)
    for n, o in zip(new, [3, 0, 1]):
        assert np.array_equal(got[n], want[o]), o
    assert max(np.abs(v.astype(np.int32)).max() for v in want.values()) > 0


def test_resize_keeps_rated_sessions_running(dev):
    from audio_denoising_amd import SessionPool
    dn = _dn(dev, P512)
    pool, twin = SessionPool(dn, 3, seed=2, rates=RATES), SessionPool(dn, 3, seed=2, rates=RATES)
    rates_of = [8000, 16000, 48000]
    for q in (pool, twin):
        for k, r in enumerate(rates_of):
            q.open(70 + k, sample_rate=r)
    frames = {k: _frames(r, 12, 300 + k) for k, r in enumerate(rates_of)}
    _feed(pool, range(3), frames, 0, 6)
    _feed(twin, range(3), frames, 0, 6)
    pool.resize(6)
    assert pool.open(sample_rate=48000) == 3 and pool.chunk(3) == (768, 768)
    got, want = _feed(pool, range(3), frames, 6, 12), _feed(twin, range(3), frames, 6, 12)
    for k in range(3):
        assert np.array_equal(got[k], want[k]), k


def test_resume_into_a_pool_without_the_rate_changes_nothing(dev, tmp_path):
    from audio_denoising_amd import SessionPool
    dn = _dn(dev, P512)
    a, b = SessionPool(dn, 2, seed=1, rates=RATES), SessionPool(dn, 3, seed=1, rates=(8000,))
    a.open(5, sample_rate=48000)
    keep = b.open(6, sample_rate=8000)
    frames = {0: _frames(48000, 4, 1)}
    _feed(a, [0], frames, 0, 4)
    b.recv({keep: _frames(8000, 4, 2)[0]})
    st = a.export([0])
    before = (b._open.copy(), b._pushes.copy(), b._rate.copy(), b.export([keep]).records.cpu(), [t.clone() for t in b._adapt], b.counters(keep))
    with pytest.raises(ValueError, match="48000"):
        b.resume(st)
    with pytest.raises(ValueError, match="48000"):
        a.move([0], b)
    assert a._open[0]
    after = (b._open, b._pushes, b._rate, b.export([keep]).records.cpu(), b._adapt, b.counters(keep))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    assert torch.equal(before[3], after[3]) and all(torch.equal(x, y) for x, y in zip(before[4], after[4])) and before[5] == after[5]
    # a state without rates saved to a file has exactly the keys it always had
    plain = SessionPool(dn, 1, seed=1)
    plain.open(3)
    plain.export([0]).save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as z:
        assert sorted(z.files) == ["geometry", "host_pushes", "queue_lengths", "queue_samples", "records", "seed"]
    b.export([keep]).save(tmp_path / "rated.npz")
    with np.load(tmp_path / "rated.npz") as z:
        assert {"rates", "adapter_in_lengths", "adapter_in_samples", "adapter_out_lengths", "adapter_out_samples"} <= set(z.files)
