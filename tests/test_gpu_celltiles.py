"""The GRUUNet2 conv tiles on the GPU (``pytest -m gpu``), where v_mfma_f32_16x16x4_f32 is the real instruction and the VALU rows' fmaf chains have
to reproduce it.

1.  The cases of tests/celltile_cases.py at batch 3: dn_cell_forward (live rows only, lane geometry from compares) against
    dn_cell_forward_parent_tiles (the tiles as they were), bit for bit on `out` and `hx`.
2.  One group of four hops at batch 2 through the group kernel against the one-hop pipe: frames and hx, torch.equal (cell_body is shared, so the
    schedules keep agreeing by construction; this is the product's kernel running the new tiles)."""
import pytest
import torch

import celltile_cases as cc
import model_abi
from test_gpu_parity import _model, _params

pytestmark = pytest.mark.gpu

B_CELL, B_GROUP, N_ITER = 3, 2, 3


@pytest.fixture(scope="module")
def backend():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return model_abi.GpuBackend()


@pytest.mark.parametrize("case", cc.CASES, ids=cc.IDS)
def test_live_row_tiles_against_the_parent_tiles_bit_for_bit(backend, case):
    cc.check(backend, case, B_CELL)
    torch.cuda.synchronize()


def test_group_of_four_hops_against_the_one_hop_pipe(backend):
    from audio_denoising_amd.pipeline import Denoiser, HopPipeline
    dev, p = backend.device, _params("S")
    dn = Denoiser(_model(dev, 5), p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=N_ITER)
    frames = (0.1 * torch.randn(4, B_GROUP, p.n_fft, generator=torch.Generator().manual_seed(606))).to(dev)

    def run(group):
        pipe = HopPipeline(dn, B_GROUP)
        hx, out = dn.init_hx(B_GROUP), torch.empty_like(frames)
        if group:
            pipe.set_group(4)
            pipe.submit_group(frames, hx, out, seed=77, stream_id0=5)
        else:
            for i in range(4):
                pipe.submit(frames[i], hx, out[i], seed=77, stream_id0=5)
        pipe.flush()
        torch.cuda.synchronize()
        return out, hx

    ref_out, ref_hx = run(False)
    out, hx = run(True)
    assert torch.isfinite(ref_out).all() and ref_out.abs().max().item() > 1e-3 and ref_hx.abs().max().item() > 1e-3
    assert torch.equal(out, ref_out) and torch.equal(hx, ref_hx)
