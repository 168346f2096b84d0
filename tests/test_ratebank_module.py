"""The Python side of the rate banks without any library: the rate index and its refusal, and the optional rate fields of ``SessionState`` --
their checks, ``to``, and file compatibility both ways (a state without rates writes exactly the keys it always wrote; such a file loads)."""
import numpy as np
import pytest
import torch

from audio_denoising_amd.sessions import SessionState, rate_index, record_layout

GEO = dict(sample_rate=16000, n_fft=512, hop=256, n_mels=64, hidden=17, C=4)
OLD_KEYS = ["geometry", "host_pushes", "queue_lengths", "queue_samples", "records", "seed"]


def _records(n):
    g = torch.Generator().manual_seed(n)
    return torch.randint(0, 255, (n, record_layout(GEO["n_fft"], GEO["C"])["stride"]), dtype=torch.uint8, generator=g)


def test_rate_index_and_its_refusal():
    assert rate_index(16000, (8000, 48000), None) == -1 and rate_index(16000, (8000, 48000), 16000) == -1
    assert rate_index(16000, (8000, 48000), 48000) == 1 and rate_index(16000, [8000, 48000], 8000) == 0
    with pytest.raises(ValueError, match=r"44100 .*16000.*rates=\(8000, 48000\)"):
        rate_index(16000, (8000, 48000), 44100)
    with pytest.raises(ValueError, match="without rates"):
        rate_index(16000, None, 48000)


def test_a_state_without_rates_writes_the_keys_it_always_wrote(tmp_path):
    st = SessionState(_records(2), GEO, 7, [np.arange(3, dtype=np.float32), np.zeros(0, np.float32)], [4, 0])
    assert st.rates is None and st.adapter_in is None and st.adapter_out is None
    st.save(tmp_path / "plain.npz")
    with np.load(tmp_path / "plain.npz") as z:
        assert sorted(z.files) == OLD_KEYS
    back = SessionState.load(tmp_path / "plain.npz")
    assert back.rates is None and back.adapter_in is None and torch.equal(back.records, st.records)
    assert back.seed == 7 and back.host_pushes.tolist() == [4, 0] and [q.tolist() for q in back.queues] == [[0.0, 1.0, 2.0], []]
    assert st.to("cpu").rates is None


def test_a_file_written_before_the_rate_fields_loads(tmp_path):
    rec = _records(1)
    np.savez(tmp_path / "old.npz", records=rec.numpy(), geometry=np.array([GEO[k] for k in ("sample_rate", "n_fft", "hop", "n_mels", "hidden", "C")], np.int64),
             seed=np.array(3, np.uint64), host_pushes=np.array([2], np.int64), queue_lengths=np.array([2], np.int64),
             queue_samples=np.array([0.5, -0.5], np.float32))
    st = SessionState.load(tmp_path / "old.npz")
    assert len(st) == 1 and st.rates is None and st.queues[0].tolist() == [0.5, -0.5] and st.geometry == GEO


def test_rate_fields_round_trip(tmp_path):
    ain = [np.arange(40, dtype=np.float32), np.zeros(0, np.float32), np.arange(14, dtype=np.float32) - 3]
    aout = [np.ones(14, np.float32), np.zeros(0, np.float32), np.full(27, 0.25, np.float32)]
    st = SessionState(_records(3), GEO, 1, None, None, rates=[48000, 16000, 8000], adapter_in=ain, adapter_out=aout)
    st.save(tmp_path / "rated.npz")
    with np.load(tmp_path / "rated.npz") as z:
        assert sorted(z.files) == sorted(OLD_KEYS + ["rates", "adapter_in_lengths", "adapter_in_samples", "adapter_out_lengths", "adapter_out_samples"])
    for back in (SessionState.load(tmp_path / "rated.npz"), st.to("cpu")):
        assert back.rates.tolist() == [48000, 16000, 8000]
        assert all(np.array_equal(a, b) for a, b in zip(back.adapter_in, ain)) and all(np.array_equal(a, b) for a, b in zip(back.adapter_out, aout))
        assert [a.dtype for a in back.adapter_in] == [np.float32] * 3


def test_rate_fields_are_checked():
    with pytest.raises(ValueError, match="rates"):
        SessionState(_records(1), GEO, 0, adapter_in=[np.zeros(4, np.float32)])
    with pytest.raises(ValueError, match="both adapter states"):
        SessionState(_records(1), GEO, 0, rates=[48000], adapter_in=[np.zeros(4, np.float32)])
    with pytest.raises(ValueError, match="one rate"):
        SessionState(_records(2), GEO, 0, rates=[48000], adapter_in=[np.zeros(4, np.float32)], adapter_out=[np.zeros(4, np.float32)])
