"""The glue the Python front ends share (audio_denoising_amd/_glue.py), without a GPU and without the library: the phase packer against an
element-by-element loop, the tensor check and its exception types, and the schedule of a ragged clip call over the frame cap."""
import random

import pytest
import torch

from audio_denoising_amd._glue import PCM, check_tensor, pack_phases, ragged_rounds

K = 5
CPU = torch.device("cpu")


# ------------------------------------------------------------------ the phase packer
@pytest.mark.parametrize("lead", [(2,), (2, 3), (4,), (3, 2)])
def test_pack_phases_equals_the_loop(lead):
    g = torch.Generator().manual_seed(sum(lead))
    z = torch.rand(*lead, K, 3, dtype=torch.complex64, generator=g)
    got = pack_phases(z, lead, K, CPU)
    assert got.shape == lead + (3, K, 2) and got.dtype == torch.float32 and got.is_contiguous()
    flat, zf = got.reshape(-1, 3, K, 2), z.reshape(-1, K, 3)
    for i in range(flat.shape[0]):
        for c in range(3):
            for k in range(K):
                assert flat[i, c, k, 0] == zf[i, k, c].real and flat[i, c, k, 1] == zf[i, k, c].imag, (i, c, k)
    # a view that is already [..][3][K] underneath (draw_phases returns one) packs to the same bytes
    assert torch.equal(pack_phases(z.transpose(-1, -2).contiguous().transpose(-1, -2), lead, K, CPU), got)


@pytest.mark.parametrize("lead", [(2,), (2, 3), (4,), (3, 2)])
def test_pack_phases_refusals(lead):
    z = torch.zeros(*lead, K, 3, dtype=torch.complex64)
    with pytest.raises(ValueError):
        pack_phases(z.to(torch.complex128), lead, K, CPU)
    with pytest.raises(ValueError):
        pack_phases(torch.zeros(*lead, K, 3), lead, K, CPU)
    with pytest.raises(ValueError):
        pack_phases(z, lead, K + 1, CPU)
    with pytest.raises(ValueError):
        pack_phases(z, lead[:-1] + (lead[-1] + 1,), K, CPU)
    with pytest.raises(ValueError):
        pack_phases(z, (1,) + lead, K, CPU)
    with pytest.raises(ValueError, match="init_angles"):
        pack_phases(z, lead, K, CPU, from_input=True)


# ------------------------------------------------------------------ the tensor check
def test_check_tensor_accepts_and_refuses():
    for dtype in PCM:
        check_tensor(torch.zeros(3, 8, dtype=dtype), "hop", (3, 8), PCM, CPU)
        check_tensor(torch.zeros(3, 8, dtype=dtype), "hop", (3, None), PCM, "cpu", min_width=8)
    check_tensor(torch.zeros(3, 16)[:, ::2], "hop", (3, 8), PCM, CPU, contiguous=False)
    check_tensor(torch.zeros(2, 3, 4), "anything", None, (torch.float32,))
    for bad in (torch.zeros(3, 8, dtype=torch.float64), torch.zeros(3, 7), torch.zeros(8, 3), torch.zeros(3, 8, 1), torch.zeros(24),
                torch.zeros(3, 16)[:, ::2], torch.zeros(8, 3).t()):
        with pytest.raises(ValueError):
            check_tensor(bad, "hop", (3, 8), PCM, CPU)
    with pytest.raises(ValueError):
        check_tensor(torch.zeros(3, 7), "x", (3, None), PCM, CPU, min_width=8)
    with pytest.raises(ValueError):
        check_tensor(torch.zeros(4, 9), "x", (3, None), PCM, CPU, min_width=8)
    with pytest.raises(ValueError):
        check_tensor(torch.zeros(3), "x", (3, None), PCM, CPU)
    with pytest.raises(TypeError, match="float32"):
        check_tensor(torch.zeros(3, 8, dtype=torch.float64), "x", None, PCM, dtype_error=TypeError)


@pytest.mark.parametrize("error", [ValueError, RuntimeError])
def test_check_tensor_wrong_device_raises_the_callers_type(error):
    t = torch.zeros(3, 8)
    for device in (torch.device("cuda:0"), "cuda"):
        with pytest.raises(error) as e:
            check_tensor(t, "hop", (3, 8), PCM, device, error)
        assert type(e.value) is error and "hop" in str(e.value)
    with pytest.raises(error):          # the device comes first: a tensor wrong in every way raises the call site's device type
        check_tensor(torch.zeros(2, dtype=torch.float64), "hop", (3, 8), PCM, torch.device("cuda:0"), error)


# ------------------------------------------------------------------ the ragged schedule
def _rounds(n_hops, cap):
    return [tuple(r) for r in ragged_rounds(n_hops, cap)]


def test_ragged_rounds_known_schedules():
    assert _rounds((1, 0, 2, 9, 3), 4) == [(1, 0, 1, 1, 1), (0, 0, 1, 1, 1), (0, 0, 0, 2, 1), (0, 0, 0, 4, 0), (0, 0, 0, 1, 0)]
    # more streams than the cap: the first three live ones take part, one hop each
    assert _rounds((2, 2, 2, 2, 2), 3) == [(1, 1, 1, 0, 0), (1, 1, 1, 0, 0), (0, 0, 0, 1, 1), (0, 0, 0, 1, 1)]
    for cap in (8, 9, 65536):
        assert _rounds((3, 5), cap) == [(3, 5)]
    assert _rounds((3, 5), 7) == [(3, 3), (0, 2)]
    assert _rounds((0, 0, 0), 4) == [] and _rounds((0,), 1) == []
    n = [2, 7]
    list(ragged_rounds(n, 3))
    assert n == [2, 7], "the caller's list is left alone"


def test_ragged_rounds_properties():
    rng = random.Random(20)
    for _ in range(400):
        B, cap = rng.randint(1, 6), rng.randint(1, 9)
        n_hops = [rng.randint(0, 7) for _ in range(B)]
        left = list(n_hops)
        rounds = _rounds(n_hops, cap)
        if sum(n_hops) <= cap:
            assert rounds == ([tuple(n_hops)] if sum(n_hops) else []), (n_hops, cap, rounds)
        for r in rounds:
            assert len(r) == B and 0 < sum(r) <= cap and min(r) >= 0, (n_hops, cap, r)
            live = [b for b in range(B) if left[b] > 0]
            if sum(n_hops) > cap:
                share = cap // min(len(live), cap)
                for i, b in enumerate(live):
                    # the first `cap` live streams share the cap equally, each at most what it has left; a live stream runs nothing only
                    # where `cap` live streams stand before it
                    assert r[b] == (min(left[b], share) if i < cap else 0), (n_hops, cap, r)
            assert all(r[b] == 0 for b in range(B) if b not in live)
            left = [left[b] - r[b] for b in range(B)]
        assert left == [0] * B, (n_hops, cap, rounds)
        assert len(rounds) <= max(1, sum(n_hops)), "every round runs at least one hop"
