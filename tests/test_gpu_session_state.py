"""Session state on the MI355X (``pytest -m gpu``): 1,024 scattered sessions of a pool of 8,192 exported and imported into a pool of 2,048 at
permuted slots continue bit for bit under DN_SESS_AUTO; decoded records against DenoiserStream's tensors; resize in place; suspend -> save
-> load -> resume in a new Denoiser's pool through recv with samples queued on the host; refusals; move to another pool and device."""
import numpy as np
import pytest
import torch

from test_gpu_sessions import _denoiser, _open_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return torch.device("cuda:0")


def _params(tag):
    from oracle import pipeline_ref
    return {"S": pipeline_ref.PARAMS_S, "R1": pipeline_ref.PARAMS_R1}[tag]


@pytest.mark.parametrize("tag", ["S", "R1"])
def test_1024_scattered_sessions_continue_bit_for_bit_in_a_smaller_pool(dev, tag):
    from audio_denoising_amd import SessionPool
    p = _params(tag)
    dn = _denoiser(dev, p)
    seed = 77
    a, b = SessionPool(dn, 8192, seed=seed), SessionPool(dn, 2048, seed=seed)
    _open_all(a, sids=np.arange(8192) * 5 + 3)
    rng = np.random.default_rng(13)
    src = rng.choice(8192, 1024, replace=False)
    dst = rng.permutation(2048)[:1024]
    g = torch.Generator().manual_seed(21)
    # staggered ages: group k of the listed sessions has had max(4 - k, 0) pushes (group 4: open, still priming)
    group = np.arange(1024) % 5
    for t in range(4):
        live = src[group <= t]
        a.push(live, (0.1 * torch.randn(live.size, p.hop, generator=g)).to(dev))
    st = a.export(src)
    assert sorted(set(st.pushes.tolist())) == [0, 1] and st.frames.max() == 3
    assert b.resume(st, slots=dst) == dst.tolist()
    ran = 0
    for t in range(6):
        hops = (0.1 * torch.randn(1024, p.hop, generator=g)).to(dev)
        oa = a.push(src, hops)
        ob = b.push(dst, hops)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob), (tag, t)
        ran += int(float(oa.abs().max()) > 0)
    assert ran >= 5
    for k in (0, 4, 517):
        assert a.counters(int(src[k])) == b.counters(int(dst[k]))


def test_decoded_records_equal_denoiser_stream_tensors(dev):
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd.pipeline import DenoiserStream
    p = _params("S")
    dn = _denoiser(dev, p)
    seed, sids, pushes = 5, [41, 42, 2 ** 33 + 1, 7], [5, 3, 1, 0]
    pool = SessionPool(dn, 8, seed=seed)
    slots = [pool.open(s) for s in sids]
    refs = [DenoiserStream(dn, 1, stream_id0=s, seed=seed) for s in sids]
    g = torch.Generator().manual_seed(4)
    for t in range(max(pushes)):
        live = [k for k in range(4) if t < pushes[k]]
        hops = (0.1 * torch.randn(len(live), p.hop, generator=g)).to(dev)
        pool.push([slots[k] for k in live], hops)
        for r, k in enumerate(live):
            refs[k].push(hops[r:r + 1].contiguous())
    st = pool.export(slots)
    for k, ref in enumerate(refs):
        assert np.array_equal(st.ring[k], ref.ring[0].cpu().numpy()), k
        assert np.array_equal(st.ola[k], ref.ola[0].cpu().numpy()), k
        assert np.array_equal(st.hx[k], ref.hx[0].cpu().numpy()), k
        assert (int(st.frames[k]), int(st.pushes[k]), int(st.stream_ids[k])) == (ref.hops, min(pushes[k], 1), sids[k]), k
    assert np.abs(st.ola[0]).max() > 0


def test_resize_keeps_every_slot_and_its_samples(dev):
    from audio_denoising_amd import SessionPool
    p = _params("S")
    dn = _denoiser(dev, p)
    cap = 8
    pool, twin = SessionPool(dn, cap, seed=3), SessionPool(dn, cap, seed=3)
    for q in (pool, twin):
        for s in range(cap):
            assert q.open(100 + s) == s
    g = torch.Generator().manual_seed(9)
    order = np.random.default_rng(2).permutation(cap)

    def tick(ids):
        hops = (0.1 * torch.randn(len(ids), p.hop, generator=g)).to(dev)
        assert torch.equal(pool.push(ids, hops), twin.push(ids, hops))

    tick(order)
    tick(order[:5])
    with pytest.raises(RuntimeError, match="full"):
        pool.open()
    pool.resize(2 * cap)
    assert pool.capacity == 2 * cap and pool._open[:cap].all() and not pool._open[cap:].any()
    for t in range(3):
        tick(order[t:])
    assert pool.open(9) == cap
    with pytest.raises(ValueError, match="open"):
        pool.resize(cap)                                       # slot 8 is open
    assert pool.capacity == 2 * cap
    tick(order)
    pool.close(cap)
    pool.resize(cap)                                           # a shrink that drops no open slot
    tick(order[::-1].copy())
    assert [pool.counters(s) for s in range(cap)] == [twin.counters(s) for s in range(cap)]


def test_suspend_save_load_resume_through_recv(dev, tmp_path):
    from audio_denoising_amd import SessionPool, SessionState
    p = _params("S")
    dn = _denoiser(dev, p)
    pool, ref = SessionPool(dn, 4, seed=21), SessionPool(dn, 4, seed=21)
    slots = [pool.open(60 + k) for k in range(3)]
    for k in range(3):
        ref.open(60 + k)
    rng = np.random.default_rng(8)
    sizes = [441, 959, 1001, 333]

    def chunks(call):
        return {s: (0.2 * rng.standard_normal(sizes[(call + s) % 4])).astype(np.float32) for s in slots}

    got = {s: [] for s in slots}
    want = {s: [] for s in slots}
    for call in range(3):
        c = chunks(call)
        for s, y in pool.recv(c).items():
            got[s].append(y)
        for s, y in ref.recv(c).items():
            want[s].append(y)
    st = pool.suspend(slots)
    assert not pool._open[slots].any()
    assert all(q.size > 0 for q in st.queues) and len(st) == 3
    path = tmp_path / "sessions.npz"
    st.save(path)
    loaded = SessionState.load(path)
    assert torch.equal(loaded.records, st.records.cpu()) and loaded.seed == 21
    dn2 = _denoiser(dev, p)                                    # a new Denoiser with the same weights (a new process would build one)
    pool2 = SessionPool(dn2, 6, seed=21)
    pool2.open(999)
    new = pool2.resume(loaded)
    assert new == [1, 2, 3]
    to_new = dict(zip(slots, new))
    for call in range(3, 7):
        c = chunks(call)
        res = pool2.recv({to_new[s]: x for s, x in c.items()})
        for s in slots:
            got[s].append(res[to_new[s]])
        for s, y in ref.recv(c).items():
            want[s].append(y)
    for s in slots:
        assert np.array_equal(np.concatenate(got[s]), np.concatenate(want[s])), s


def test_resume_refuses_another_seed_or_geometry_and_changes_nothing(dev):
    from audio_denoising_amd import SessionPool
    dn = _denoiser(dev, _params("S"))
    pool = SessionPool(dn, 4, seed=1)
    pool.open()
    pool.push([0], torch.zeros(1, dn.hop, device=dev))
    st = pool.export([0])
    other_seed = SessionPool(dn, 4, seed=2)
    with pytest.raises(ValueError, match="seed"):
        other_seed.resume(st)
    r1 = SessionPool(_denoiser(dev, _params("R1")), 4, seed=1)
    with pytest.raises(ValueError, match="geometry"):
        r1.resume(st)
    full = _full(SessionPool(dn, 1, seed=1))
    with pytest.raises(ValueError, match="free"):
        full.resume(st)
    for q in (other_seed, r1):
        assert not q._open.any()
    assert pool._open[0]


def _full(pool):
    while not pool._open.all():
        pool.open()
    return pool


def _move_and_compare(dev_a, dev_b):
    from audio_denoising_amd import SessionPool
    p = _params("S")
    dn_a, dn_b = _denoiser(dev_a, p), _denoiser(dev_b, p)
    a, twin, b = SessionPool(dn_a, 6, seed=4), SessionPool(dn_a, 6, seed=4), SessionPool(dn_b, 3, seed=4)
    for q in (a, twin):
        for s in range(6):
            q.open(200 + s)
    g = torch.Generator().manual_seed(1)
    for t in range(2):
        hops = 0.1 * torch.randn(6, p.hop, generator=g)
        assert torch.equal(a.push(range(6), hops.to(dev_a)), twin.push(range(6), hops.to(dev_a)))
    new = a.move([4, 1], b)
    assert new == [0, 1] and not a._open[[4, 1]].any()
    for t in range(3):
        hops = 0.1 * torch.randn(6, p.hop, generator=g)
        ob = b.push(new, hops[[4, 1]].to(dev_b)).cpu()
        ot = twin.push([4, 1], hops[[4, 1]].to(dev_a)).cpu()
        assert torch.equal(ob, ot), t
        assert float(ot.abs().max()) > 0


def test_move_to_another_pool(dev):
    _move_and_compare(dev, dev)


def test_move_across_devices():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    _move_and_compare(torch.device("cuda:0"), torch.device("cuda:1"))
