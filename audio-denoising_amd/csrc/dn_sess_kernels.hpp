// dn_sess_kernels.hpp -- the hop of a SESSION POOL (dn_sessions_*): the same bodies as dn_stream_step, for a list of n slots of a pool of `capacity`
// instead of a whole batch.  Workgroup (or wavefront) i serves row i of the call -- hop_in, hop_out, init_angles and the workspace are packed in list
// order -- and slot s = ids[i] of the pool: ring, overlap-add line, hx, frame counter, priming count and Griffin-Lim stream id are read and written at s.
// Every body is called with its pointers offset to the row / slot and b = 0 (sid0 = the slot's stream id), so stft_body, cell_body, invmel_body,
// gl_body and glw_body run unchanged: a session's samples are the bits dn_stream_step gives it at B = 1.
//
// Two schedules:
//   sess_frame_kernel   ONE launch, one workgroup per listed slot, P1-P12 back to back (frame_kernel's form; every built n_fft);
//   sess_front_kernel + sess_chain_kernel
//                       TWO launches (n_fft 1024): the front halves (P1-P10, stft -> GRUUNet2 -> inverse mel into a workspace row), then the
//                       Griffin-Lim chains a wavefront per session, four a workgroup, with the overlap-add and emit epilogue (the split hop of
//                       dn_pipe_set_split without the pipelining: no added latency).
// The library validates the id list on the host (in range, unique, open) before it enqueues anything: no kernel sees a bad index.
//
// Session records (dn_sessions_export / dn_sessions_import, layout in include/dn_denoise.h): sess_export_kernel gathers the listed slots
// into records and sess_import_kernel scatters records into slots, a workgroup a record; sess_check_kernel validates the headers of an
// import before anything is written.
//
// Four translation units, as the hop's (dn_hop_kernels.hpp; Makefile: the scheduling strategy of each kernel family):
//   dn_sessions.hip       n_fft 1024 one-launch form (max-ILP, as frame_kernel), the open and record kernels, the dispatch;
//   dn_sessions1536.hip   n_fft 1536 one-launch form (default strategy);
//   dn_sessions512.hip    n_fft 512 one-launch form (default strategy);
//   dn_sessions_glw.hip   the two-launch form (iterative-ILP, as the wavefront-per-stream hop kernels): sess_front_kernel's instantiations and
//                         sess_chain_kernel.
// Each unit defines the launcher declared here for its size, by instantiating launch_sess_frame_of below.  (No session kernel has probe arrays of
// its own, so the stamped diagnostic build keeps the same four units.)
#pragma once
#include "dn_dispatch.hpp"
#include "dn_hop_common.hpp"

namespace dn {

void launch_sess_frame_unit(Size<1024>, const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in);     // (dn_sessions.hip)
void launch_sess_frame_unit(Size<1536>, const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in);     // (dn_sessions1536.hip)
void launch_sess_frame_unit(Size<512>, const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in);      // (dn_sessions512.hip)

// the slot's input row and output row of the call (int16 or float32)
__device__ __forceinline__ const void* sess_row(const void* p, int s16, size_t i, int hop) {
    return s16 ? static_cast<const void*>(static_cast<const short*>(p) + i * hop) : static_cast<const void*>(static_cast<const float*>(p) + i * hop);
}
__device__ __forceinline__ void* sess_row(void* p, int s16, size_t i, int hop) {
    return s16 ? static_cast<void*>(static_cast<short*>(p) + i * hop) : static_cast<void*>(static_cast<float*>(p) + i * hop);
}

// ---- one launch: workgroup i runs the whole hop of slot ids[i] (frame_kernel with one level of indirection)
// PHIN (an input-phase pool: a.init is its phasor rows): as frame_kernel's -- the analysis stores the unit phasors of its STFT in row i and the chain starts
// from them; wave w / lane l reads back what wave w / lane l stored (every n_fft), behind two workgroup barriers.
template <int NFFT, bool BF16, int CT, bool PHIN = false>
__global__ __launch_bounds__(kHopPipeThreads, NFFT == 1536 ? 2 : 1) void sess_frame_kernel(DspDev d, CellDev cd, SessArgs a) {
    constexpr int kNR = NFFT, kHop = NFFT / 2, kBins = Geo<NFFT>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[hop_smem<NFFT>()];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    // the slot's counters as the previous push left them (read by every thread before the ring shift's barriers; written below by thread 0 only)
    const unsigned int pushed = a.pushes[s];
    const unsigned long long f = a.frames[s];
    const uint64_t sid = a.sids[s];
    float* ring = a.ring + s * kNR;
    void* out = sess_row(a.hop_out, a.out_s16, i, kHop);
    ring_shift<NFFT, kHopPipeThreads>(ring, sess_row(a.hop_in, a.in_s16, i, kHop), a.in_s16, 0, tid);
    if (pushed < (unsigned int)a.prime) {          // the slot's first n_fft/hop - 1 pushes only fill its ring
        pcm_zero_hop(out, a.out_s16, 0, kHop, tid, kHopPipeThreads);          // a priming push emits zeros
        if (tid == 0) a.pushes[s] = pushed + 1;
        return;
    }
    const int M = d.n_mels;
    float* mel = a.mel + i * 3 * M;
    float* diff = a.diff + i * 3 * M;
    float* peak = a.peak + i;
    float* hx = a.hx + s * kHidden * a.C;
    float2* phas = PHIN ? reinterpret_cast<float2*>(const_cast<float*>(a.init)) + i * 3 * kBins : nullptr;
    stft_body<NFFT, false, true, kHopPipeThreads, PHIN>(smem, d, ring, nullptr, mel, peak, DN_PEAK_NORMALIZE | DN_PRE_WINDOW, 0, tid, phas);   // P1-P6
    __syncthreads();
    cell_body<kHopPipeThreads / 64, BF16, CT, kCellStageDefault, DN_FRAME_TILES>(smem, cd, mel, hx, diff, hx, 3, a.C, 0, tid);     // P7
    __syncthreads();
    if (tid >= kHopThreads) return;
    const v2f* init = PHIN ? reinterpret_cast<const v2f*>(phas) : a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + i * 3 * kBins : nullptr;
    // P8-P12: the slot's f-th frame draws from (seed + f, the slot's stream id)
    gl_body<NFFT, true, true>(smem, d, mel, diff, init, a.seed + f, sid, peak, nullptr, a.n_iter, a.mom, 0, tid, a.ola + s * kNR, out, a.out_s16);
    if (tid == 0) a.frames[s] = f + 1;
}

template <int NFFT>
static void launch_sess_frame_of(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    with_bool(phase_in, [&](auto phin) {
        with_model<NFFT>(bf16, a.C, [&](auto bf, auto ct) {
            hipLaunchKernelGGL((sess_frame_kernel<NFFT, decltype(bf)::value, decltype(ct)::value, decltype(phin)::value>), dim3(a.n), dim3(kHopPipeThreads),
                               0, st, d, c, a);
        });
    });
}

// ---- two launches, n_fft 1024.  First: workgroup i runs P1-P10 of slot ids[i] into workspace row i and leaves the frame's seed in meta row i
// (0 in word 0: a priming push, no chain).  PHIN (an input-phase pool): it also stores the unit phasors of the row's STFT in phasor row i, which the chain
// launch takes as its init (a kernel boundary lies between).
template <bool BF16, int CT, bool PHIN = false>
__global__ __launch_bounds__(kHopPipeThreads, kFrontPerCu) void sess_front_kernel(DspDev d, CellDev cd, SessArgs a) {
    constexpr int kNR = 1024, kHop = 512, kBins = Geo<1024>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[front_smem<1024>()];
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    const unsigned int pushed = a.pushes[s];
    const unsigned long long f = a.frames[s];
    float* ring = a.ring + s * kNR;
    uint32_t* meta = a.meta + i * kSessMeta;
    ring_shift<kNR, kHopPipeThreads>(ring, sess_row(a.hop_in, a.in_s16, i, kHop), a.in_s16, 0, tid);
    if (pushed < (unsigned int)a.prime) {
        pcm_zero_hop(sess_row(a.hop_out, a.out_s16, i, kHop), a.out_s16, 0, kHop, tid, kHopPipeThreads);
        if (tid == 0) { SessMeta::store_idle(meta); a.pushes[s] = pushed + 1; }
        return;
    }
    const int M = d.n_mels;
    float* mel = a.mel + i * 3 * M;
    float* diff = a.diff + i * 3 * M;
    float* hx = a.hx + s * kHidden * a.C;
    stft_body<kNR, false, true, kHopPipeThreads, PHIN>(smem, d, ring, nullptr, mel, a.peak + i, DN_PEAK_NORMALIZE | DN_PRE_WINDOW, 0, tid,
                                                       PHIN ? reinterpret_cast<float2*>(const_cast<float*>(a.init)) + i * 3 * kBins : nullptr);   // P1-P6
    __syncthreads();
    cell_body<kHopPipeThreads / 64, BF16, CT, false>(smem, cd, mel, hx, diff, hx, 3, a.C, 0, tid);                                   // P7
    __syncthreads();
    invmel_body<kNR, true, kHopPipeThreads>(smem, d, mel, diff, a.lin + i * 3 * kBins, 3, 0, tid);                                   // P8-P10
    if (tid == 0) {
        SessMeta{a.seed + f}.store(meta);
        a.frames[s] = f + 1;
    }
}

}  // namespace dn
