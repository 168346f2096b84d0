// the two-launch form of the session pool under iterative-ILP scheduling, as the wavefront-per-stream hop kernels (Makefile; see dn_sess_kernels.hpp)
#include "dn_sess_kernels.hpp"

namespace dn {

// Second: wavefront j of workgroup g runs the whole Griffin-Lim chain of row 4 g + j (P11-P12) and emits its hop.
__global__ __launch_bounds__(kHopPipeThreads, 2) void sess_chain_kernel(DspDev d, SessArgs a) {
    constexpr int kNR = 1024, kHop = 512, kBins = Geo<1024>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[glw_smem<1024>()];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t i = (size_t)blockIdx.x * kGlwWaves + wv;
    const uint32_t* meta = a.meta + i * kSessMeta;
    const bool runs = i < (size_t)a.n && SessMeta::runs(meta);
    if (!runs) {
        // every wave meets the others at ONE LDS-only barrier: the ones with a chain inside glw_body, after their share of the window tables
        glw_fill_tables<kNR, kHopPipeThreads>(smem, d, tid);
        DN_LDS_BARRIER();
        return;
    }
    const size_t s = (size_t)a.ids[i];
    const uint64_t seed = SessMeta::load(meta).seed;
    const uint64_t sid = a.sids[s];
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + i * 3 * kBins : nullptr;
    glw_body<kNR, kEmitStream>(smem, d, a.lin + i * 3 * kBins, init, seed, sid, a.peak + i, nullptr, a.n_iter, a.mom, 0, lane, wv,
                               a.ola + s * kNR, sess_row(a.hop_out, a.out_s16, i, kHop), a.out_s16, 0, -1, kGlwFresh, nullptr, tid);
}

void launch_sess_split(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    // (input-phase pool: a.init is the phasor rows; the front halves store them and the chains start from them as from injected phases)
    with_bool(phase_in, [&](auto phin) {
        with_model<1024>(bf16, a.C, [&](auto bf, auto ct) {
            hipLaunchKernelGGL((sess_front_kernel<decltype(bf)::value, decltype(ct)::value, decltype(phin)::value>), dim3(a.n), dim3(kHopPipeThreads),
                               0, st, d, c, a);
        });
    });
    hipLaunchKernelGGL(sess_chain_kernel, dim3((a.n + kGlwWaves - 1) / kGlwWaves), dim3(kHopPipeThreads), 0, st, d, a);
}

}  // namespace dn
