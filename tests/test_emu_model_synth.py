"""The two model kernels with SYNTHETIC weights against float64, on the host emulation of the kernel sources (no GPU needed).
tests/model_cases.py holds the cases, the references and the checks, tests/model_abi.py the driver of the C ABI; oracle/synth_weights.py the blobs and what the
trained checkpoints of every other model test cannot see (dead channels, one offset buffer for three gates).  tests/test_gpu_model_synth.py
runs the same cases on the GPU.

  (a) dn_cell_forward, C = 1..5 x T in {1, 2, 3, 4, 7}                      against float64 oracle/model_ref.forward
  (b) dn_cell_forward_ex, hx_scale 0.9                                      against float64 times 0.9 on hx
  (c) dn_cell_forward_bf16, C = 4, 5 x T = 3, 7                             against the float64 forward with bf16-rounded MFMA conv operands
  (d) cell_body inside dn_process_frame (n_fft 512 / 1024 / 1536 x 80 / 32 mels) and, over four chained hops at n_fft 1024, inside the
      group pipe (H = 3), the split hop, the session pool and clip mode     against float64 oracle/pipeline_np64.process_frame64 (residual, hx)
  (e) dn_momo_forward, every padding triple, both values of every output_padding, T = 1 / 4, prev given / None
                                                                            against float64 oracle/momo_ref.forward(paddings=...)

Tolerance: R x e_ref, e_ref = the fp32 CPU oracle's own error against float64 on the case, R per family from this tier's measured ratios
(model_cases.R, profiles/model_synth_margins.txt); R x e_ref <= 1e-5 on every fp32 case.  Each test prints its figures before it asserts.
The emulator runs a work-item per OS thread: about 3 s a GRUUNet2 case, 2 s a MOMO3 case, 7 s a chain; the module takes about 3 minutes.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402
import model_abi  # noqa: E402
import model_cases as mc  # noqa: E402

TIER = "emu"


@pytest.fixture(scope="module")
def backend():
    return model_abi.Abi(emu.load())


@pytest.mark.parametrize("case", mc.GRU_CASES, ids=mc.GRU_IDS)
def test_cell_forward_with_synthetic_weights_against_float64(backend, case):
    mc.check_gru(backend, case, TIER)


def test_cell_forward_ex_scales_the_returned_state(backend):
    mc.check_gru_ex(backend, TIER)


@pytest.mark.parametrize("case", mc.GRU_BF16_CASES, ids=[c.id for c in mc.GRU_BF16_CASES])
def test_cell_forward_bf16_against_the_bf16_rounding_yardstick(backend, case):
    mc.check_gru_bf16(backend, case, TIER)


@pytest.mark.parametrize("n_fft,n_mels", mc.HOP_GEOMETRIES)
def test_process_frame_residual_and_hx_with_synthetic_weights(backend, n_fft, n_mels):
    mc.check_hop(backend, n_fft, n_mels, TIER)


@pytest.mark.parametrize("path", mc.CHAIN_PATHS)
def test_four_chained_hops_carry_hx_with_synthetic_weights(backend, path):
    mc.check_chain(backend, path, TIER)


@pytest.mark.parametrize("case", mc.MOMO_CASES, ids=mc.MOMO_IDS)
def test_momo3_with_synthetic_weights_and_every_padding_triple_against_float64(backend, case):
    mc.check_momo(backend, case, TIER)


DN_ERR_INVALID = -1


@pytest.mark.parametrize("pads", [p for p in mc.PADDING_TRIPLES if mc.momo_bins(p)[0] > mc.MOMO_MIN_F], ids=lambda p: "p" + "".join(map(str, p)))
def test_momo3_refuses_one_bin_under_the_smallest_input_of_a_padding_triple(backend, pads):
    """The library's own shape rules, not their restatement in model_cases.momo_lengths: dn_momo_forward takes the smallest F of the triple
    (the cases above run it) and answers DN_ERR_INVALID one bin under it -- a level is left without a sample, or, where C's truncating
    division still finds one, the transposed convs cannot reach the skip length, which is what the reference raises."""
    F = mc.momo_bins(pads)[0]
    assert backend.momo_status(pads, F, mc.momo_lengths(F, pads)[2])[0] == 0
    rc, msg = backend.momo_status(pads, F - 1, 1)
    assert rc == DN_ERR_INVALID and (b"too short" in msg or b"not reachable" in msg or b"compresses" in msg), (rc, msg)
