"""The two model kernels with SYNTHETIC weights against float64 on the GPU: the cases, references and checks of tests/model_cases.py
(tests/test_emu_model_synth.py lists the families), through the C ABI and through the Python front ends of tests/model_abi.py -- GRUUNet2.forward (Cb comes from
hx.shape[2]: the module is built for 5 compressed bins and run at 1..5), conv_precision "bf16", MOMO3.forward, Denoiser.process_frame.

Tolerance: R x e_ref, e_ref = the fp32 CPU oracle's own error against float64 on the case, R per family from one MI355X run of this module's
cases (model_cases.R["gpu"], profiles/model_synth_margins.txt); R x e_ref <= 1e-5 on every fp32 case.  Figures are printed before each assert.
"""
import pytest

import model_abi
import model_cases as mc

pytestmark = pytest.mark.gpu
TIER = "gpu"


@pytest.fixture(scope="module")
def backend():
    return model_abi.GpuBackend()


@pytest.mark.parametrize("case", mc.GRU_CASES, ids=mc.GRU_IDS)
def test_cell_forward_and_module_with_synthetic_weights_against_float64(backend, case):
    mc.check_gru(backend, case, TIER, modes=("fp32", "module"))


def test_cell_forward_ex_scales_the_returned_state(backend):
    mc.check_gru_ex(backend, TIER)


@pytest.mark.parametrize("case", mc.GRU_BF16_CASES, ids=[c.id for c in mc.GRU_BF16_CASES])
def test_cell_forward_bf16_against_the_bf16_rounding_yardstick(backend, case):
    mc.check_gru_bf16(backend, case, TIER, modes=("bf16", "module-bf16"))


@pytest.mark.parametrize("n_fft,n_mels", mc.HOP_GEOMETRIES)
def test_process_frame_residual_and_hx_with_synthetic_weights(backend, n_fft, n_mels):
    mc.check_hop(backend, n_fft, n_mels, TIER)


@pytest.mark.parametrize("path", mc.CHAIN_PATHS)
def test_four_chained_hops_carry_hx_with_synthetic_weights(backend, path):
    mc.check_chain(backend, path, TIER)


@pytest.mark.parametrize("case", mc.MOMO_CASES, ids=mc.MOMO_IDS)
def test_momo3_and_module_with_synthetic_weights_and_every_padding_triple_against_float64(backend, case):
    mc.check_momo(backend, case, TIER, vias=("abi", "module"))
