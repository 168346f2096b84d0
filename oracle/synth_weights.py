"""Synthetic weight blobs for the two model kernels (TEST INFRASTRUCTURE).

The trained checkpoints under tests/golden/ leave channels dead (3 of 17 of d0, 13 of 51 of d3 ... are zero at every stream and
position of the goldens) and hold the same Gaussian offsets [0, .2, .4, .6, .8, 1] in all three gates, so a kernel that mixes up
a weight row feeding a dead channel, or folds a bias table from the wrong gate's offset buffer, agrees with them.  The blobs here
are drawn so that neither can hide:

  * conv weights N(0, 1 / fan_in), fan_in = input channels x 3 taps (position-code channels included);
  * biases N(mean, 0.25), positive on average so that relu leaves the channels alive on signed inputs: mean BIAS_MEAN = 0.6 in the
    levels whose output feeds another conv, GATE_BIAS_MEAN = 1.0 in the two levels that produce the GRU gates (the last encoder
    level and the hidden-gate conv).  Tuned on the float64 oracle alone: 0.3 +- 0.2 left 1..9 of d3's 51 channels dead at batch 6;
    raising the mean EVERYWHERE makes it worse (0.9 -> 1.8: 63 -> 84 dead channels over the 25 GRUUNet2 cases), because a
    level's positive outputs times the random-sign row sums of the next level's weights shift whole channels below zero;
    raising it in the gate levels only, whose outputs feed no further relu, takes the count from 73 to 37, and relu still clips
    most channels somewhere.  The last dead channels of a case go with its seed: tests/model_cases.py takes, per case, the first
    seed of the case's offset kind whose float64 run has none (a condition on the input; a CPU test asserts it for every case);
  * every gate gets its OWN offset buffer, of one of three kinds:
      "shifted"  linspace(0, 1, 6) + a per-gate shift;
      "uneven"   offset[0], offset[0] + 0.2, then uneven increments;
      "spacing"  evenly spaced with a spacing that is NOT 0.2 (0.15 / 0.25 / 0.3): the reference keeps the constructor's
                 coeff = -0.5 / 0.2^2 after load_state_dict (gruunet2.py:62-63), so does every kernel, and so must the oracle;
      "standard" linspace(0, 1, 6) in every gate, as in the checkpoints (the control).

Everything is drawn from numpy's default_rng(seed): no torch RNG, so a blob is the same on every host.
The blobs are flat fp32 arrays in state_dict order (oracle/model_ref.STATE_KEYS, oracle/momo_ref.STATE_KEYS).
"""
from __future__ import annotations

import numpy as np

from . import model_ref, momo_ref

BIAS_MEAN, GATE_BIAS_MEAN, BIAS_STD = 0.6, 1.0, 0.25
OFFSET_KINDS = ("shifted", "uneven", "spacing", "standard")
SPACINGS = (0.15, 0.25, 0.3)


def offset_kind(seed: int) -> str:
    """The kind a seed draws when none is asked for: seeds 2, 5, 8 ... are the spacing != 0.2 ones."""
    return OFFSET_KINDS[seed % 3]


def _offsets(rng, kind: str, gate: int) -> np.ndarray:
    std = np.linspace(0.0, 1.0, 6, dtype=np.float32)
    if kind == "standard":
        return std
    if kind == "shifted":
        return (std + np.float32((-0.11, 0.07, 0.16)[gate] + 0.02 * rng.uniform(-1, 1))).astype(np.float32)
    if kind == "uneven":
        start = np.float32((0.05, -0.08, 0.0)[gate])
        steps = np.concatenate([[0.2], rng.uniform(0.08, 0.35, 4)])
        return (start + np.concatenate([[0.0], np.cumsum(steps)])).astype(np.float32)
    assert kind == "spacing", kind
    return (np.float32((0.1, -0.1, 0.0)[gate]) + np.float32(SPACINGS[gate]) * np.arange(6, dtype=np.float32)).astype(np.float32)


def _blob(state_keys, seed: int, offsets: str | None) -> np.ndarray:
    rng = np.random.default_rng(seed)
    kind = offset_kind(seed) if offsets is None else offsets
    assert kind in OFFSET_KINDS, kind
    parts, gate = [], 0
    last_down = max(key for key, _ in state_keys if key.startswith("cell.input_gate.downs") and key.endswith("bias"))
    for key, shape in state_keys:
        if key.endswith("conv.weight"):
            # Conv1d (out, in, k) and ConvTranspose1d (in, out, k): the reduction runs over `in` x k either way
            cin = shape[0] if ".ups." in key else shape[1]
            parts.append(rng.standard_normal(shape) / np.sqrt(3.0 * cin))
        elif key.endswith("conv.bias"):
            gates = key == last_down or key.startswith("cell.reset_gate")
            parts.append((GATE_BIAS_MEAN if gates else BIAS_MEAN) + BIAS_STD * rng.standard_normal(shape))
        else:
            assert key.endswith("gs.offset"), key
            parts.append(_offsets(rng, kind, gate))
            gate += 1
    return np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in parts])


def gruunet2_blob(seed: int, offsets: str | None = None) -> np.ndarray:
    """(15337,) fp32: a GRUUNet2 state_dict (4 levels, hidden 17, 6 gaussians) in key order."""
    blob = _blob(model_ref.STATE_KEYS, seed, offsets)
    assert blob.size == model_ref.N_WEIGHT_FLOATS
    return blob


def momo3_blob(seed: int, offsets: str | None = None) -> np.ndarray:
    """(9165,) fp32: a MOMO3 state_dict (3 levels, hidden 16, 6 gaussians; two offset buffers) in key order."""
    blob = _blob(momo_ref.STATE_KEYS, seed, offsets)
    assert blob.size == momo_ref.N_WEIGHT_FLOATS
    return blob
