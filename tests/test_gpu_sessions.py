"""Session pools on the MI355X (``pytest -m gpu``): slots that open, push and close on their own, against DenoiserStream at B = 1 per
session (bit for bit), the two-launch schedule against the one-launch one, the host layer ``recv`` against DenoiserStream.push, a pool
whose every slot pushes every tick against DenoiserStream(dn, capacity), four int16 sessions against oracle/pipeline_ref.StreamRef, and
the bf16 conv tiles at the restated config-3 tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu

CFG = dict(in_size=1, hidden_sizes=(17, 17, 17, 17), kernel_sizes=(3, 3, 3, 3), strides=(2, 2, 2, 2), paddings=(1, 1, 1, 1), num_gaussians=6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


def _state_dict(short="dari_tult"):
    from oracle import model_ref
    return model_ref.unflatten_weights(np.fromfile(os.path.join(GOLDEN, f"weights_{short}.bin"), dtype=np.float32))


def _denoiser(dev, p, precision="fp32"):
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser
    m = GRUUNet2(num_compressed_bins=p.num_compressed_bins, **CFG)
    m.load_state_dict(_state_dict())
    m = m.eval().to(dev)
    m.conv_precision = precision
    return Denoiser(m, p.sample_rate, p.n_fft, p.hop, p.n_mels)


def _open_all(pool, sids=None):
    """Open every slot of a pool at once (the C call takes a list; SessionPool.open takes one slot)."""
    ids = np.arange(pool.capacity, dtype=np.int32)
    s = None if sids is None else np.ascontiguousarray(sids, dtype=np.uint64)
    with torch.cuda.device(pool.dn.device):
        pool.lib.check(pool.lib.dn_sessions_open(pool.handle, ids.ctypes.data_as(C.c_void_p), ids.size,
                                                 None if s is None else s.ctypes.data_as(C.c_void_p), pool._stream()))
    pool._open[:] = True
    pool._pushes[:] = 0
    for k in range(pool.capacity):
        pool._queue[k] = np.zeros(0, dtype=np.float32)


# tick -> (sessions opened: (slot, stream id), slots closed, slots pushed in this order)
RAGGED = [
    ([(0, 100), (1, 7)], [], [0]),
    ([(2, 12)], [], [1, 0, 2]),
    ([(3, 55)], [], [3, 1]),
    ([], [], [0, 3, 1, 2]),
    ([(1, 9)], [1], [1, 0]),            # slot 1 closed and reopened as another session
    ([], [], [3, 1, 0]),
    ([], [2], [1, 3]),
    ([(2, 77)], [], [2, 1, 0]),
    ([], [], [0, 2, 1, 3]),
]


@pytest.mark.parametrize("tag", ["S", "R1"])
def test_ragged_sessions_equal_denoiser_stream_per_session_bit_for_bit(dev, tag):
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd.pipeline import DenoiserStream
    from oracle import pipeline_ref
    p = {"S": pipeline_ref.PARAMS_S, "R1": pipeline_ref.PARAMS_R1}[tag]
    dn = _denoiser(dev, p)
    seed = 1000
    pool = SessionPool(dn, 6, seed=seed)
    g = torch.Generator().manual_seed(5)
    sig = (0.1 * torch.randn(8, 12 * p.hop, generator=g)).to(dev)
    sess, refs, n_frames = {}, {}, 0
    for opened, closed, pushed in RAGGED:
        for s in closed:
            pool.close(s)
        for s, sid in opened:
            assert pool.open(sid) == s                        # the lowest free slot
            sess[s] = [len(refs), 0]
            refs[len(refs)] = DenoiserStream(dn, 1, stream_id0=sid, seed=seed)
        hops = torch.stack([sig[sess[s][0], sess[s][1] * p.hop:(sess[s][1] + 1) * p.hop] for s in pushed]).contiguous()
        out = pool.push(pushed, hops)
        for r, s in enumerate(pushed):
            want = refs[sess[s][0]].push(hops[r:r + 1].contiguous())
            if sess[s][1] == 0:
                assert want.shape[1] == 0 and torch.all(out[r] == 0)
            else:
                assert torch.equal(out[r], want[0]), (tag, s)
                n_frames += 1
            sess[s][1] += 1
    assert n_frames >= 12
    for s, (k, h) in sess.items():
        assert pool.counters(s) == (h - 1, p.n_fft // p.hop - 1)


def test_two_launches_equal_one_launch_at_1024_scattered_slots(dev):
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd._lib import DN_SESS_ONE_LAUNCH, DN_SESS_TWO_LAUNCHES
    from oracle import pipeline_ref
    p = pipeline_ref.PARAMS_S
    dn = _denoiser(dev, p)
    cap, n = 4096, 1024
    pools = []
    for sch in (DN_SESS_ONE_LAUNCH, DN_SESS_TWO_LAUNCHES):
        pool = SessionPool(dn, cap, seed=3)
        pool.set_schedule(sch)
        _open_all(pool, sids=np.arange(cap) * 3 + 1)
        pools.append(pool)
    rng = np.random.default_rng(11)
    g = torch.Generator().manual_seed(8)
    lists = [rng.choice(cap, n, replace=False) for _ in range(2)]
    # ticks: list 0 three times (priming, then frames), then list 1 (half of it new sessions), then list 0 again
    for t, li in enumerate([0, 0, 0, 1, 0]):
        hops = (0.1 * torch.randn(n, p.hop, generator=g)).to(dev)
        a = pools[0].push(lists[li], hops)
        b = pools[1].push(lists[li], hops)
        torch.cuda.synchronize()
        assert torch.equal(a, b), t
        if t in (2, 4):                                          # (a session's first frame emits the still-zero ola[:hop])
            assert float(a.abs().max()) > 0
    with pytest.raises(Exception, match="1024"):
        SessionPool(_denoiser(dev, pipeline_ref.PARAMS_R1), 4).set_schedule(DN_SESS_TWO_LAUNCHES)


def test_recv_ragged_chunks_equal_denoiser_stream(dev):
    """recv() with 441 / 960 / 1,000-sample chunks, sessions present in some calls only: float32 chunks give DenoiserStream.push's samples
    of the same chunks bit for bit, int16 chunks the same quantised as app3.py:244-245; no hop run -> the chunk's passthrough."""
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd.pipeline import DenoiserStream
    from oracle import pipeline_ref
    p = pipeline_ref.PARAMS_S
    dn = _denoiser(dev, p)
    pool = SessionPool(dn, 4, seed=21)
    kinds = {pool.open(50): "f32", pool.open(51): "s16", pool.open(52): "f32"}
    refs = {s: DenoiserStream(dn, 1, stream_id0=50 + s, seed=21) for s in kinds}
    rng = np.random.default_rng(2)
    sizes = [441, 960, 1000]
    ran = passthrough = 0
    for call in range(14):
        chunks = {}
        for s, kind in kinds.items():
            if (call + s) % 4 == 3:
                continue                                     # this session sent nothing in this round
            nsz = sizes[(call + s) % 3]
            x = (0.2 * rng.standard_normal(nsz)).astype(np.float32)
            chunks[s] = (np.clip(x, -1, 1) * 32767).astype(np.int16) if kind == "s16" else x
        res = pool.recv(chunks)
        for s, c in chunks.items():
            f = c.astype(np.float32) / np.iinfo(np.int16).max if kinds[s] == "s16" else c
            want = refs[s].push(torch.from_numpy(f[None]).to(dev))[0].cpu().numpy()
            if want.size == 0:
                want = np.clip(f, -1.0, 1.0)
                passthrough += 1
            else:
                ran += 1
            if kinds[s] == "s16":
                want = (np.clip(want, -1.0, 1.0) * 32767).astype(np.int16)
            assert res[s].dtype == want.dtype and np.array_equal(res[s], want), (call, s)
    assert ran >= 20 and passthrough >= 3


def test_all_slots_every_tick_equal_denoiser_stream_batch(dev):
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd.pipeline import DenoiserStream
    from oracle import pipeline_ref
    p = pipeline_ref.PARAMS_S
    dn = _denoiser(dev, p)
    cap = 64
    pool = SessionPool(dn, cap, seed=9)
    for s in range(cap):
        assert pool.open() == s                               # stream id = the slot index
    ref = DenoiserStream(dn, cap, stream_id0=0, seed=9)
    g = torch.Generator().manual_seed(3)
    for t in range(5):
        hops = (0.1 * torch.randn(cap, p.hop, generator=g)).to(dev)
        a = pool.push(range(cap), hops)
        b = ref.push(hops)
        if t == 0:
            assert b.shape[1] == 0 and torch.all(a == 0)
        else:
            assert torch.equal(a, b), t


def test_four_int16_sessions_match_stream_ref(dev):
    """Four sessions opened at different ticks, int16 in and int16 out, golden initial phases per frame injected through the push:
    against oracle/pipeline_ref.StreamRef on the same quantised input at the streaming bands (RMS 1e-3, max-abs 2e-2)."""
    from audio_denoising_amd import SessionPool
    from oracle import pipeline_ref
    p = pipeline_ref.PARAMS_S
    g = load_golden("stream_S.npz")
    sig, inits = g["signal"], g["init_angles"]                   # (4, 5632), (10, 4, K, 3)
    q = np.clip(np.round(sig * 32767), -32768, 32767).astype(np.int16)
    dn = _denoiser(dev, p)
    pool = SessionPool(dn, 4)
    start = [0, 1, 3, 4]                                          # the tick each session joins
    n_hops = 8
    outs = {k: [] for k in range(4)}
    for t in range(max(start) + n_hops):
        for k in range(4):
            if t == start[k]:
                assert pool.open(k) == k
        live = [k for k in range(4) if start[k] <= t < start[k] + n_hops][::-1]
        hops = torch.from_numpy(np.stack([q[k, (t - start[k]) * p.hop:(t - start[k] + 1) * p.hop] for k in live])).to(dev)
        ia = [inits[max(t - start[k] - 1, 0)][k] for k in live]   # frame f of a session runs on its (f+1)-th push
        o = pool.push(live, hops, init_angles=torch.from_numpy(np.stack(ia)).to(dev)).cpu().numpy()
        for r, k in enumerate(live):
            if t > start[k]:
                outs[k].append(o[r])
    got = np.stack([np.concatenate(outs[k]) for k in range(4)])
    sr = pipeline_ref.StreamRef(_state_dict(), p, 4)
    with torch.no_grad():
        ref = sr.push(torch.from_numpy(q[:, :n_hops * p.hop].astype(np.float32) / np.float32(32767)),
                      init_angles_per_hop=[torch.from_numpy(inits[f]) for f in range(n_hops - 1)]).numpy()
    want = (np.clip(ref, -1, 1) * 32767).astype(np.int16)
    assert got.shape == want.shape
    err = (got.astype(np.float64) - want.astype(np.float64)) / 32767
    rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    print(f"int16 sessions vs StreamRef: RMS {rms:.2e} max-abs {mx:.2e}")
    assert rms <= 1e-3 and mx <= 2e-2 and np.abs(want).max() > 100


def test_bf16_sessions_close_to_fp32_at_the_restated_config3_tolerance(dev):
    from audio_denoising_amd import SessionPool
    from oracle import pipeline_ref
    p = pipeline_ref.PARAMS_S
    pools = [SessionPool(_denoiser(dev, p, prec), 32, seed=4) for prec in ("fp32", "bf16")]
    for pool in pools:
        for _ in range(32):
            pool.open()
    g = torch.Generator().manual_seed(6)
    rng = np.random.default_rng(4)
    ids = rng.permutation(32)[:24]
    res = [[], []]
    for t in range(4):
        hops = (0.1 * torch.randn(24, p.hop, generator=g)).to(dev)
        for j, pool in enumerate(pools):
            res[j].append(pool.push(ids, hops).cpu())
    a, b = torch.cat(res[0][1:], 1), torch.cat(res[1][1:], 1)
    w = (b - a).numpy()
    w_rms, w_max = float(np.sqrt(np.mean(w ** 2))), float(np.abs(w).max())
    print(f"bf16 sessions vs fp32: waveform RMS {w_rms:.2e} max-abs {w_max:.3f} (signal RMS {float(a.pow(2).mean().sqrt()):.3f})")
    assert w_rms <= 5e-3 and w_max <= 5e-2
    assert not torch.equal(a, b)                                # (the bf16 tiles are in use)
