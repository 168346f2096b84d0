// dn_cell.hip -- GRUUNet2.forward: Conv1d U-Net encoder / convolutional-GRU bottleneck /
// ConvTranspose1d decoder, T sequential time steps, persistent hidden state.
// Replaces gruunet2.py:127-156 (DownBlocks), 184-199 (UpBlocks), 228-244 (GRUUNetCell.forward),
// 266-306 (GRUUNet2._gruunet / forward); math restated in SURVEY.md Appendix A.
//
// The reference issues ~60 small tensor ops per time step.  Here ONE workgroup owns ONE stream
// and runs the whole forward out of LDS (activations of kCellChunk = 3 steps: ~34 KB at F = 80):
//   * the encoder does not depend on hx (gruunet2.py:231), so it runs batched over the chunk's
//     time steps; likewise the decoder after the recurrent part; only gh = relu(conv(hx)), the
//     GRU gates and h' are sequential in t;
//   * the 6 Gaussian position-code channels are input independent: their convolution is folded
//     into per-position bias tables at plan time (CellDev::bt_*), so kernels convolve data
//     channels only (-26 % MACs);
//   * every conv level is a small dense contraction  out[o][(t,p)] = sum_(c,tap) W[o][(c,tap)] *
//     im2col(x)[(c,tap)][(t,p)]  and runs on the matrix cores with v_mfma_f32_16x16x4_f32
//     (f32 in, f32 accumulate: bit-for-bit an fmaf chain, so the fp32 parity bar holds):
//     rows = 16 output channels, columns = 16 (t, position) items, K = 4 (channel, tap) pairs
//     per instruction.  The A (weight) fragments are pre-arranged on the host in lane order
//     ([m-tile][k-step][64 lanes], one coalesced 256-B load each); the B fragments are the
//     im2col view of the LDS activations -- one ds_read_b32 per lane per k-step at a computed
//     address, no staging copy.  1,024 MACs per instruction instead of 64: the per-stream
//     forward is latency-bound on instruction issue, so this is what shortens it.  The tiles cover
//     whole row tiles only: channel 16 of a 17-channel level (rows 48..50 of the 51-row encoder
//     level) is the same fmaf chain on VALU lanes, one lane per (row, item) -- a second row tile
//     spent as many MFMAs again on one live row in sixteen;
//   * bottleneck hidden gates (51 channels x C positions, N too small for a tile): lane =
//     (gate channel, position) on the VALU with that lane's 51 recurrent weights pinned in VGPRs
//     across time steps; the single-channel last decoder level: lane = (t, position), VALU.
#include "dn_cell_body.hpp"

namespace dn {

constexpr int kCellWaves = 4;

// CT / TC: the compressed bin count and the number of time steps when they are the usual ones (5 or 4 bins, the hop's 3 columns), 0 = run time
// TILES: the variant of the fp32 conv tiles (dn_cell_body.hpp); 0 = the tiles before the live-row / lane-geometry change (launch_cell_parent_tiles)
template <int CT, int TC, int TILES = DN_CELL_TILES>
__global__ __launch_bounds__(kCellWaves * 64) void cell_kernel(CellDev cd, const float* __restrict__ x,
                                                              const float* __restrict__ hx_in, float* __restrict__ out,
                                                              float* __restrict__ hx_out, int T, int C) {
    __shared__ __attribute__((aligned(16))) char smem[kCellSmem];
    cell_body<kCellWaves, false, CT, kCellStageDefault, TILES>(smem, cd, x, hx_in, out, hx_out, TC ? TC : T, C, blockIdx.x, threadIdx.x);
}

// BASELINE config 3: the same forward with bf16 MFMA conv tiles (v_mfma_f32_16x16x32_bf16; conv inputs and weights
// rounded to bf16, fp32 accumulate; the recurrent gate conv, the GRU math and the last decoder level stay fp32).
__global__ __launch_bounds__(kCellWaves * 64) void cell_kernel_bf16(CellDev cd, const float* __restrict__ x,
                                                                   const float* __restrict__ hx_in, float* __restrict__ out,
                                                                   float* __restrict__ hx_out, int T, int C) {
    __shared__ __attribute__((aligned(16))) char smem[kCellSmem];
    cell_body<kCellWaves, true>(smem, cd, x, hx_in, out, hx_out, T, C, blockIdx.x, threadIdx.x);
}

void launch_cell(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                 int C, hipStream_t st) {
    auto k = cell_kernel<0, 0>;
    if (C == 5) k = T == kCellChunk ? cell_kernel<5, kCellChunk> : cell_kernel<5, 0>;
    else if (C == 4) k = T == kCellChunk ? cell_kernel<4, kCellChunk> : cell_kernel<4, 0>;
    hipLaunchKernelGGL(k, dim3(B), dim3(kCellWaves * 64), 0, st, c, x, hx_in, out, hx_out, T, C);
}

// The same forward on the tiles as they were (comparison only: tests and tools/; nothing in the product calls it).
void launch_cell_parent_tiles(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                              int C, hipStream_t st) {
    auto k = cell_kernel<0, 0, 0>;
    if (C == 5) k = T == kCellChunk ? cell_kernel<5, kCellChunk, 0> : cell_kernel<5, 0, 0>;
    else if (C == 4) k = T == kCellChunk ? cell_kernel<4, kCellChunk, 0> : cell_kernel<4, 0, 0>;
    hipLaunchKernelGGL(k, dim3(B), dim3(kCellWaves * 64), 0, st, c, x, hx_in, out, hx_out, T, C);
}

__global__ __launch_bounds__(kCellWaves * 64) void cell_kernel_ex(CellDev cd, const float* __restrict__ x,
                                                                 const float* __restrict__ hx_in, float* __restrict__ out,
                                                                 float* __restrict__ hx_out, int T, int C, float hx_scale) {
    __shared__ __attribute__((aligned(16))) char smem[kCellSmem];
    cell_body<kCellWaves>(smem, cd, x, hx_in, out, hx_out, T, C, blockIdx.x, threadIdx.x, hx_scale);
}

void launch_cell_ex(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                    int C, float hx_scale, hipStream_t st) {
    hipLaunchKernelGGL(cell_kernel_ex, dim3(B), dim3(kCellWaves * 64), 0, st, c, x, hx_in, out, hx_out, T, C, hx_scale);
}

void launch_cell_bf16(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                      int C, hipStream_t st) {
    hipLaunchKernelGGL(cell_kernel_bf16, dim3(B), dim3(kCellWaves * 64), 0, st, c, x, hx_in, out, hx_out, T, C);
}

}  // namespace dn

#ifdef DN_PROBE
// diagnostic build only: the phase stamps of workgroup 0 of the stand-alone cell kernel
extern "C" int dn_probe_read_cell(unsigned long long* host32) {
    return (int)hipMemcpyFromSymbol(host32, HIP_SYMBOL(dn::g_cell_probe), sizeof(dn::g_cell_probe));
}
#endif
