"""The model half of the oracle is PINNED: oracle/model_ref.py must reproduce
golden vectors produced by the reference's own gruunet2.GRUUNet2
(oracle/make_golden.py; gruunet2.py:246-306)."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
from oracle import model_ref

CASES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "cell_dari_tult*_B*_T*_F*.npz")))


def _sd(short):
    return model_ref.unflatten_weights(np.fromfile(os.path.join(GOLDEN, f"weights_{short}.bin"), dtype=np.float32))


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference_golden(name):
    short = "dari_tult2" if "dari_tult2" in name else "dari_tult"
    g = load_golden(name)
    out, hx = model_ref.forward(_sd(short), torch.from_numpy(g["x"]), torch.from_numpy(g["hx0"]))
    # tolerance: fp32 conv summation order differs between runs/threads (~1e-6)
    assert np.abs(out.numpy() - g["out"]).max() <= 1e-5
    assert np.abs(hx.numpy() - g["hx1"]).max() <= 1e-5


def test_intermediates_match_reference_hooks():
    g = load_golden("cell_dari_tult_B4_T3_F80.npz")
    inter = {}
    model_ref.cell_step(_sd("dari_tult"), torch.from_numpy(g["x"][:, 0]), torch.from_numpy(g["hx0"]), inter)
    for k in ("d0", "d1", "d2", "d3", "gate_h"):
        assert np.abs(inter[k].numpy() - g[k]).max() <= 1e-5, k


def test_conventions_2d_input_and_default_hx():
    g = load_golden("cell_dari_tult_conventions.npz")
    sd = _sd("dari_tult")
    o2, h2 = model_ref.forward(sd, torch.from_numpy(g["x2"]))
    assert o2.shape == (3, 64) and h2.shape == (1, 17, 4)       # gruunet2.py:291-293,304-305
    assert np.abs(o2.numpy() - g["out2"]).max() <= 1e-5
    o3, h3 = model_ref.forward(sd, torch.from_numpy(g["x3"]))
    assert np.abs(o3.numpy() - g["out3"]).max() <= 1e-5 and np.abs(h3.numpy() - g["hx3"]).max() <= 1e-5


def test_chain_of_20_hops_carries_state():
    g = load_golden("cell_dari_tult_chain20_F80.npz")
    sd = _sd("dari_tult")
    hx = None
    for h in range(20):
        o, hx = model_ref.forward(sd, torch.from_numpy(g["x"][h]), hx, num_compressed_bins=5)
        assert np.abs(o.numpy() - g["out"][h]).max() <= 2e-5
    assert np.abs(hx.numpy() - g["hx_final"]).max() <= 2e-5


def test_smear_tables_match_reference():
    g = load_golden("smear.npz")
    off = torch.linspace(0, 1, 6)
    for L in (80, 64, 40, 32, 20, 16, 10, 8, 5, 4):
        assert np.abs(model_ref.smear_table(off, L).numpy() - g[f"L{L}"]).max() <= 1e-7


# ------------------------------------------------------------------ sibling model MOMO3
MOMO_CASES = ["momo3_B1_T3_F22.npz", "momo3_B4_T3_F22.npz", "momo3_B256_T3_F22.npz", "momo3_B3_T7_F24.npz", "momo3_B2_T1_F23.npz"]


def _momo_sd():
    import os
    from conftest import GOLDEN
    from oracle import momo_ref
    return momo_ref.unflatten_weights(np.fromfile(os.path.join(GOLDEN, "weights_momo3_4d4ea0.bin"), dtype=np.float32))


@pytest.mark.parametrize("name", MOMO_CASES)
def test_momo3_restatement_matches_reference_golden(name):
    """oracle/momo_ref.py against vectors produced by the reference's own momo3.MOMO3 (oracle/make_momo_golden.py): PINNED."""
    from oracle import momo_ref
    g = load_golden(name)
    prev = torch.from_numpy(g["prev"]) if "prev" in g.files else None
    with torch.no_grad():
        out, hx = momo_ref.forward(_momo_sd(), torch.from_numpy(g["x"]), torch.from_numpy(g["hx0"]), prev)
    assert np.abs(out.numpy() - g["out"]).max() <= 1e-5 and np.abs(hx.numpy() - g["hx1"]).max() <= 1e-5


def test_momo3_conventions_and_carried_prev():
    from oracle import momo_ref
    g = load_golden("momo3_conventions.npz")
    sd = _momo_sd()
    with torch.no_grad():
        o2, h2 = momo_ref.forward(sd, torch.from_numpy(g["x2"]))             # (T,F) input, hx=None
        assert o2.shape == (3, 22) and h2.shape == (1, 16, 3)
        assert np.abs(o2.numpy() - g["out2"]).max() <= 1e-5
        hx, prev = None, None
        for h in range(12):
            x = torch.from_numpy(g["xs"][h])
            o, hx = momo_ref.forward(sd, x, hx, prev)
            prev = x[:, -1:, :].clone()
            assert np.abs(o.numpy() - g["outs"][h]).max() <= 1e-5
    assert np.abs(hx.numpy() - g["hx_final"]).max() <= 1e-5


# ------------------------------------------------------------------ synthetic weights (oracle/synth_weights.py, tests/model_cases.py)
@pytest.mark.parametrize("name", ["cell_synth_B2_T3_F80.npz", "momo3_synth_B2_T3_F22.npz"])
def test_restatements_match_the_reference_class_on_a_synthetic_blob_with_other_offset_spacings(name):
    """The reference's own classes, loaded with a blob whose offset buffers differ per gate and are spaced 0.15 / 0.25 / 0.3 apart, on signed
    inputs (oracle/make_golden.py, oracle/make_momo_golden.py): PINS the coeff semantics -- the constructor's -0.5 / 0.2^2 survives
    load_state_dict (gruunet2.py:62-63), the loaded offsets enter only in `dist - offset`.  fp32 to 1e-5, float64 (the class cast with
    .double()) to 1e-12.  A smear_table that recomputes coeff from the loaded buffer is 0.23 (GRUUNet2) and 0.07 (MOMO3) off on `out` here."""
    from oracle import momo_ref
    ref = momo_ref if name.startswith("momo3") else model_ref
    g = load_golden(name)
    sd = ref.unflatten_weights(g["blob"])
    offs = [v.numpy() for k, v in sd.items() if k.endswith("gs.offset")]
    assert all(abs(float(o[1] - o[0]) - 0.2) > 0.04 for o in offs) and not np.array_equal(offs[0], offs[1])
    assert g["x"].min() < -5 and g["x"].max() > 5                                      # signed inputs
    for dtype, tag, tol in ((torch.float32, "", 1e-5), (torch.float64, "_f64", 1e-12)):
        with torch.no_grad():
            out, hx = ref.forward({k: v.to(dtype) for k, v in sd.items()}, torch.from_numpy(g["x"]).to(dtype), torch.from_numpy(g["hx0"]).to(dtype))
        assert out.dtype == dtype and g["out" + tag].dtype == out.numpy().dtype
        assert np.abs(out.numpy() - g["out" + tag]).max() <= tol, (tag, np.abs(out.numpy() - g["out" + tag]).max())
        assert np.abs(hx.numpy() - g["hx1" + tag]).max() <= tol, (tag, np.abs(hx.numpy() - g["hx1" + tag]).max())


def test_synthetic_blobs_give_every_gate_its_own_offsets_and_come_from_numpy_alone():
    from oracle import momo_ref, synth_weights
    state = torch.get_rng_state()
    for seed, kind in ((0, "shifted"), (1, "uneven"), (2, "spacing")):
        assert synth_weights.offset_kind(seed) == kind
        for make, ref in ((synth_weights.gruunet2_blob, model_ref), (synth_weights.momo3_blob, momo_ref)):
            blob = make(seed)
            assert blob.dtype == np.float32 and np.array_equal(blob, make(seed)) and not np.array_equal(blob, make(seed + 3))
            offs = [v.numpy() for k, v in ref.unflatten_weights(blob).items() if k.endswith("gs.offset")]
            for a in range(len(offs)):
                for b in range(a + 1, len(offs)):
                    assert np.abs(offs[a] - offs[b]).max() > 0.02, (kind, a, b)
            spacing = [float(o[1] - o[0]) for o in offs]
            assert all(abs(s - 0.2) < 1e-6 for s in spacing) if kind != "spacing" else all(abs(s - 0.2) > 0.04 for s in spacing)
    std = [v for k, v in model_ref.unflatten_weights(synth_weights.gruunet2_blob(0, "standard")).items() if k.endswith("gs.offset")]
    assert all(torch.equal(o, torch.linspace(0, 1, 6)) for o in std)
    assert torch.equal(state, torch.get_rng_state())                                   # no torch RNG


def test_every_channel_is_live_in_every_synthetic_case():
    """The live-channel condition of tests/model_cases.py, no case left out: in the float64 oracle run every channel of d0..d3 / gate_h
    (GRUUNet2) and d0..d2 / gate_h (MOMO3) is nonzero at some stream, position or step.  Inputs are signed and reach +-6."""
    import model_cases as mc
    assert len(mc.GRU_CASES) == 25 and {(c.C, c.T) for c in mc.GRU_CASES} == {(C, T) for C in range(1, 6) for T in (1, 2, 3, 4, 7)}
    assert sum(c.hx_zero for c in mc.GRU_CASES) == 1
    kinds = {c.id.split("-")[2] for c in mc.GRU_CASES}
    assert kinds == {"shifted", "uneven", "spacing"}
    for c in mc.GRU_CASES:
        x, hx = c.inputs()
        assert x.shape == (mc.B, c.T, 16 * c.C) and x.min() < -5 and x.max() > 5 and (not hx.any()) == c.hx_zero
        assert mc.dead_channels(mc.gru_reference(c)["steps"], ("d0", "d1", "d2", "d3", "gate_h")) == {}, c.id
    for c in mc.GRU_BF16_CASES:
        assert mc.gru_case_is_usable(c, bf16=True), c.id
        assert 100 * mc.BF16_NO_FLIP < mc.bf16_yardstick_gap(c), c.id          # the bf16 yardstick is 5e-3 .. 1e-2 from the unrounded forward
    assert {(c.C, c.T) for c in mc.GRU_BF16_CASES} == {(4, 3), (4, 7), (5, 3), (5, 7)}
    for c in mc.MOMO_CASES:
        x, hx, prev = c.inputs()
        assert x.shape == (mc.B, c.T, c.F) and hx.shape == (mc.B, 16, c.C) and (prev is not None) == c.with_prev
        assert mc.dead_channels(mc.momo_reference(c)["steps"], ("d0", "d1", "d2", "gate_h")) == {}, c.id


def test_seed_tables_hold_the_first_usable_seed_of_every_case():
    """GRU_SEED_K, BF16_SEED_K and MOMO_SEED_K derived again from the oracles: each entry is the FIRST k whose seed leaves no channel dead (and,
    for the bf16 cases, no rounding flip between the fp32 and float64 runs of the yardstick), so the lists cannot go stale or be hand-picked."""
    import model_cases as mc
    assert mc.derive_seed_tables() == (mc.GRU_SEED_K, mc.BF16_SEED_K, mc.MOMO_SEED_K)


def test_momo3_cases_cover_every_padding_triple_and_both_output_paddings_and_nothing_accepted_is_refused():
    import model_cases as mc
    from oracle import momo_ref
    assert mc.momo_refusals() == []                 # 3 <= F <= 64 with a sample left at every level: the transposed convs always reach the skip
    for pads in mc.PADDING_TRIPLES:
        cases = [c for c in mc.MOMO_CASES if c.pads == pads]
        Fs = sorted(c.F for c in cases)
        assert Fs[-1] == 64 and mc.momo_lengths(Fs[0], pads) is not None and (Fs[0] == 3 or mc.momo_lengths(Fs[0] - 1, pads) is None)
        assert {(l, op) for c in cases for l, op in enumerate(mc.momo_output_paddings(c.F, pads))} == {(l, op) for l in range(3) for op in (0, 1)}
        assert {c.T for c in cases} == {1, 4} and {c.with_prev for c in cases} == {True, False}
        assert all(c.C == momo_ref.compressed_bins(c.F, pads) for c in cases)
