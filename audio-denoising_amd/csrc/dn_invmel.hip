// dn_invmel.hip -- synthesis-side mel stages.  Replaces app3.py:203-211 (P8,P9,P10):
//   rec  = leaky_relu(model_input - predicted_diff, 0.2)
//   mmag = clamp(expm1(rec), min=0)
//   lin  = clamp(relu(lstsq(fb^T, mmag)), min=0)
// The reference solves an underdetermined full-rank least-squares problem per item
// (torch.linalg.lstsq, driver gels); its solution is the minimum-norm one, pinv(fb^T) @ mmag,
// so here it is ONE dense contraction against a pseudo-inverse computed once per plan.
//
// A workgroup handles kRows = 3 rows (the three columns of one stream): the mel rows sit in
// LDS and are broadcast; each lane owns output bins k, k+192, ... and streams the transposed
// pseudo-inverse ([M][K'], coalesced over k, L2-resident) exactly once for all three rows.
#include "dn_dispatch.hpp"
#include "dn_invmel_body.hpp"

namespace dn {

template <int NFFT, bool RESIDUAL>
__global__ __launch_bounds__(kInvThreads) void invmel_kernel(DspDev d, const float* __restrict__ x,
                                                             const float* __restrict__ diff, float* __restrict__ lin,
                                                             int rows) {
    __shared__ __attribute__((aligned(16))) char smem[kInvSmem];
    invmel_body<NFFT, RESIDUAL>(smem, d, x, diff, lin, rows, (size_t)blockIdx.x * kInvRows, threadIdx.x);
}

void launch_invmel(const DspDev& d, const float* x, const float* diff, float* lin, int rows, hipStream_t st) {
    with_nfft(d.n_fft, [&](auto n) {
        with_bool(diff != nullptr, [&](auto residual) {
            hipLaunchKernelGGL((invmel_kernel<decltype(n)::value, decltype(residual)::value>), dim3((rows + kInvRows - 1) / kInvRows), dim3(kInvThreads),
                               0, st, d, x, diff, lin, rows);
        });
    });
}

}  // namespace dn
