// the wavefront-per-frame chains of clip mode under iterative-ILP scheduling, as the other kernels built on glw_body (Makefile; see dn_clip_kernels.hpp)
#include "dn_clip_kernels.hpp"

namespace dn {

// ---- chains, n_fft 1024, a wavefront per frame: wave j of workgroup g runs the whole chain of frame 4 g + j from the linear magnitudes in its frame
// row and leaves frame x 1/envelope there (the wave read every magnitude in its prologue).  The last workgroup may be partly filled: its idle
// waves still fill their share of the window tables and reach the barrier.
__global__ __launch_bounds__(kHopPipeThreads, 2) void clip_chain_glw_kernel(DspDev d, ClipArgs a) {
    constexpr int kNR = 1024, kBins = Geo<1024>::kBins, kNV = Geo<1024>::kNV;
    __shared__ __attribute__((aligned(16))) char smem[glw_smem<1024>()];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t f = (size_t)blockIdx.x * kGlwWaves + wv;
    if (f >= a.frames) {
        glw_fill_tables<kNR, kHopPipeThreads>(smem, d, tid);
        DN_LDS_BARRIER();
        return;
    }
    const ClipFrame c = clip_frame(a, f);          // (f is the same for the whole wavefront: wv is a readfirstlane)
    float* row = a.fr + f * a.fr_stride;
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + f * 3 * kBins : nullptr;
    glw_body<kNR, kEmitStage>(smem, d, row, init, c.seed, a.sid0 + c.b, nullptr, nullptr, a.n_iter, a.mom, 0, lane, wv, nullptr, nullptr, 0, 0, -1,
                              kGlwFresh, nullptr, tid);
    // the wave's LDS line -> the frame row (every lane moves the sample pairs it wrote itself)
    const float* line = glw_signal_line<kNR>(smem, wv);
#pragma unroll
    for (int t = 0; t < kNV; ++t) {
        const int n = 2 * (lane + 64 * t);
        *reinterpret_cast<v2f*>(row + n) = *reinterpret_cast<const v2f*>(line + n);
    }
}

void launch_clip_chains_glw(const DspDev& d, const ClipArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(clip_chain_glw_kernel, dim3((unsigned)((a.frames + kGlwWaves - 1) / kGlwWaves)), dim3(kHopPipeThreads), 0, st, d, a);
}

}  // namespace dn
