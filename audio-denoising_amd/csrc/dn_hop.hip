// dn_hop.hip -- the whole hop as ONE launch: the dispatch over the hop units (dn_hop_kernels.hpp: which unit holds what, and why), the n_fft-1024
// wavefront-per-column instantiations (max-ILP scheduling, Makefile) and the small kernels around a pipe (control block, deferred host output).
#include "dn_hop_kernels.hpp"

namespace dn {

// The deferred host output of the LAST push (no further launch will carry it): copy, then publish (dn_pipe_stream_host_wait).
__global__ void host_copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, unsigned int n16) {
    for (unsigned int u = blockIdx.x * blockDim.x + threadIdx.x; u < n16; u += gridDim.x * blockDim.x) dst[u] = src[u];
}
__global__ void host_publish_kernel(unsigned long long* done, unsigned long long value) {
    __threadfence_system();
    __hip_atomic_store(done, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_host_copy(const uint4* src, uint4* dst, unsigned int n16, unsigned long long* done, unsigned long long value, hipStream_t st) {
    const unsigned int blocks = (n16 + 255) / 256;
    hipLaunchKernelGGL(host_copy_kernel, dim3(blocks < 1024 ? (blocks ? blocks : 1) : 1024), dim3(256), 0, st, src, dst, n16);
    hipLaunchKernelGGL(host_publish_kernel, dim3(1), dim3(1), 0, st, done, value);      // (stream order: the copy has completed)
}

__global__ void ctl_set_kernel(PipeCtl* ctl, unsigned long long pushes, unsigned long long frames, unsigned int pending) {
    ctl->pushes = pushes; ctl->frames = frames; ctl->pending = pending; ctl->done = 0;
    ctl->launches = 0; ctl->slot_next = 0;
    for (int i = 0; i < 8; ++i) ctl->front_launch[i] = 0;
}
void launch_ctl_set(PipeCtl* ctl, unsigned long long pushes, unsigned long long frames, unsigned int pending, hipStream_t st) {
    hipLaunchKernelGGL(ctl_set_kernel, dim3(1), dim3(1), 0, st, ctl, pushes, frames, pending);
}

// a.glw: the caller laid the grid out for a wavefront per stream and chain segment (n_fft 1024 only) instead of a wavefront per column
// (n_fft 512 and 1536 run a wavefront per column only: dn_api_pipe.hip never asks for another schedule at those sizes)
void launch_hop_unit(Size<1024>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) {
    if (a.glw) launch_hop_glw(d, c, a, bf16, st);
    else launch_hop_of<1024, false>(d, c, a, bf16, st);
}
void launch_frame_unit(Size<1024>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) {
    launch_frame_of<1024>(d, c, a, B, bf16, st);
}

void launch_hop(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) {
    if (a.split && a.glw && a.front_B > 0 && d.n_fft == 1024) {
        // a split hop: the chains of the hops in flight first (this launch is what a flush launch is), then the new hop's front halves
        HopArgs chains = a, fronts = a;
        chains.split = 0; chains.front_B = 0;
        chains.host_done = nullptr; chains.host_copy_src = nullptr;          // (the transport belongs to the launch that ends the hop)
        fronts.split = 0; fronts.front_only = 1; fronts.back_blocks = 0; fronts.gl_split = 0;
        launch_hop(d, c, chains, bf16, st);
        launch_hop(d, c, fronts, bf16, st);
        return;
    }
    with_nfft(d.n_fft, [&](auto n) { launch_hop_unit(n, d, c, a, bf16, st); });
}

void launch_frame(const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) {
    with_nfft(d.n_fft, [&](auto n) { launch_frame_unit(n, d, c, a, B, bf16, st); });
}

}  // namespace dn

#ifdef DN_PROBE
namespace dn {
// The stamped diagnostic build: the probe arrays are static __device__ per translation unit, so every hop kernel lives beside the readers below
// and this unit defines the side units' launchers (dn_hop1536.hip, dn_hop512.hip and dn_hop_glw.hip are empty in that build).
void launch_hop_unit(Size<1536>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) { launch_hop_of<1536, false>(d, c, a, bf16, st); }
void launch_hop_unit(Size<512>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) { launch_hop_of<512, false>(d, c, a, bf16, st); }
void launch_hop_glw(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) { launch_hop_of<1024, true>(d, c, a, bf16, st); }
void launch_frame_unit(Size<1536>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) { launch_frame_of<1536>(d, c, a, B, bf16, st); }
void launch_frame_unit(Size<512>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) { launch_frame_of<512>(d, c, a, B, bf16, st); }

}  // namespace dn

// the stamps of the Griffin-Lim workgroup 0 of hop_kernel / frame_kernel
extern "C" int dn_probe_read_hop(unsigned long long* host48) {
    return (int)hipMemcpyFromSymbol(host48, HIP_SYMBOL(dn::g_gl_probe), sizeof(dn::g_gl_probe));
}
extern "C" int dn_probe_read_blk_t(unsigned long long* host4096) {
    return (int)hipMemcpyFromSymbol(host4096, HIP_SYMBOL(dn::g_hop_blk_t), sizeof(dn::g_hop_blk_t));
}
extern "C" int dn_probe_read_blk_hw(unsigned int* host2048) {
    return (int)hipMemcpyFromSymbol(host2048, HIP_SYMBOL(dn::g_hop_blk_hw), sizeof(dn::g_hop_blk_hw));
}
extern "C" int dn_probe_read_glw(unsigned long long* host32) {
    return (int)hipMemcpyFromSymbol(host32, HIP_SYMBOL(dn::g_glw_probe), sizeof(dn::g_glw_probe));
}
extern "C" int dn_probe_read_hop_wg(unsigned long long* host8) {
    return (int)hipMemcpyFromSymbol(host8, HIP_SYMBOL(dn::g_hop_wg_probe), sizeof(dn::g_hop_wg_probe));
}
extern "C" int dn_probe_read_hop_stft(unsigned long long* host8) {
    return (int)hipMemcpyFromSymbol(host8, HIP_SYMBOL(dn::g_stft_probe), sizeof(dn::g_stft_probe));
}
extern "C" int dn_probe_read_hop_invmel(unsigned long long* host8) {
    return (int)hipMemcpyFromSymbol(host8, HIP_SYMBOL(dn::g_inv_probe), sizeof(dn::g_inv_probe));
}
#endif
