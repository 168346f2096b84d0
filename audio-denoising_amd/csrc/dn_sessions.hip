// dn_sessions.hip -- the hop of a SESSION POOL (dn_sessions_*): the same bodies as dn_stream_step, for a list of n slots of a pool of `capacity`
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
// Four translation units, as dn_hop.hip (Makefile: the scheduling strategy of each kernel family):
//   dn_sessions.hip       (this file)            n_fft 1024 one-launch form (max-ILP, as frame_kernel), the open and record kernels, the dispatch;
//   dn_sessions1536.hip   (DN_SESS_TU_1536)      n_fft 1536 one-launch form (default strategy);
//   dn_sessions512.hip    (DN_SESS_TU_512)       n_fft 512 one-launch form (default strategy);
//   dn_sessions_glw.hip   (DN_SESS_TU_GLW)       the two-launch form (iterative-ILP, as the wavefront-per-stream hop kernels).
#include "dn_hop_common.hpp"

namespace dn {

// the slot's input row and output row of the call (int16 or float32)
__device__ __forceinline__ const void* sess_row(const void* p, int s16, size_t i, int hop) {
    return s16 ? static_cast<const void*>(static_cast<const short*>(p) + i * hop) : static_cast<const void*>(static_cast<const float*>(p) + i * hop);
}
__device__ __forceinline__ void* sess_row(void* p, int s16, size_t i, int hop) {
    return s16 ? static_cast<void*>(static_cast<short*>(p) + i * hop) : static_cast<void*>(static_cast<float*>(p) + i * hop);
}
// a priming push emits zeros: the reference's ola[:hop] is still zero (app3.py:133,219)
__device__ __forceinline__ void sess_zero_row(void* out, int s16, int hop, int tid, int threads) {
    for (int n = tid; n < hop; n += threads) {
        if (s16) static_cast<short*>(out)[n] = 0;
        else static_cast<float*>(out)[n] = 0.0f;
    }
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
        sess_zero_row(out, a.out_s16, kHop, tid, kHopPipeThreads);
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

template <int NFFT, bool PHIN>
static void launch_sess_frame_p(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st) {
    constexpr int kUsualC = NFFT == 1024 ? 5 : 4;
    const dim3 grid(a.n), block(kHopPipeThreads);
    if (a.C == kUsualC) {
        if (bf16) hipLaunchKernelGGL((sess_frame_kernel<NFFT, true, kUsualC, PHIN>), grid, block, 0, st, d, c, a);
        else hipLaunchKernelGGL((sess_frame_kernel<NFFT, false, kUsualC, PHIN>), grid, block, 0, st, d, c, a);
    } else {
        if (bf16) hipLaunchKernelGGL((sess_frame_kernel<NFFT, true, 0, PHIN>), grid, block, 0, st, d, c, a);
        else hipLaunchKernelGGL((sess_frame_kernel<NFFT, false, 0, PHIN>), grid, block, 0, st, d, c, a);
    }
}
template <int NFFT>
static void launch_sess_frame_n(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    if (phase_in) launch_sess_frame_p<NFFT, true>(d, c, a, bf16, st);
    else launch_sess_frame_p<NFFT, false>(d, c, a, bf16, st);
}

#if defined(DN_SESS_TU_GLW)
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
        sess_zero_row(sess_row(a.hop_out, a.out_s16, i, kHop), a.out_s16, kHop, tid, kHopPipeThreads);
        if (tid == 0) { meta[0] = 0u; a.pushes[s] = pushed + 1; }
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
        const uint64_t seed = a.seed + f;
        meta[0] = 1u;
        meta[1] = (uint32_t)seed;
        meta[2] = (uint32_t)(seed >> 32);
        a.frames[s] = f + 1;
    }
}

// Second: wavefront j of workgroup g runs the whole Griffin-Lim chain of row 4 g + j (P11-P12) and emits its hop.
__global__ __launch_bounds__(kHopPipeThreads, 2) void sess_chain_kernel(DspDev d, SessArgs a) {
    constexpr int kNR = 1024, kHop = 512, kBins = Geo<1024>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[glw_smem<1024>()];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t i = (size_t)blockIdx.x * kGlwWaves + wv;
    const uint32_t* meta = a.meta + i * kSessMeta;
    const bool runs = i < (size_t)a.n && __builtin_amdgcn_readfirstlane((int)meta[0]) != 0;
    if (!runs) {
        // every wave meets the others at ONE LDS-only barrier: the ones with a chain inside glw_body, after their share of the window tables
        glw_fill_tables<kNR, kHopPipeThreads>(smem, d, tid);
        DN_LDS_BARRIER();
        return;
    }
    const size_t s = (size_t)a.ids[i];
    const uint64_t seed = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)meta[1]) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)meta[2]) << 32);
    const uint64_t sid = a.sids[s];
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + i * 3 * kBins : nullptr;
    glw_body<kNR, kEmitStream>(smem, d, a.lin + i * 3 * kBins, init, seed, sid, a.peak + i, nullptr, a.n_iter, a.mom, 0, lane, wv,
                               a.ola + s * kNR, sess_row(a.hop_out, a.out_s16, i, kHop), a.out_s16, 0, -1, kGlwFresh, nullptr, tid);
}

template <bool PHIN>
static void launch_sess_front(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st) {
    const dim3 block(kHopPipeThreads);
    if (a.C == 5) {
        if (bf16) hipLaunchKernelGGL((sess_front_kernel<true, 5, PHIN>), dim3(a.n), block, 0, st, d, c, a);
        else hipLaunchKernelGGL((sess_front_kernel<false, 5, PHIN>), dim3(a.n), block, 0, st, d, c, a);
    } else {
        if (bf16) hipLaunchKernelGGL((sess_front_kernel<true, 0, PHIN>), dim3(a.n), block, 0, st, d, c, a);
        else hipLaunchKernelGGL((sess_front_kernel<false, 0, PHIN>), dim3(a.n), block, 0, st, d, c, a);
    }
}
void launch_sess_split(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    // (input-phase pool: a.init is the phasor rows; the front halves store them and the chains start from them as from injected phases)
    if (phase_in) launch_sess_front<true>(d, c, a, bf16, st);
    else launch_sess_front<false>(d, c, a, bf16, st);
    hipLaunchKernelGGL(sess_chain_kernel, dim3((a.n + kGlwWaves - 1) / kGlwWaves), dim3(kHopPipeThreads), 0, st, d, a);
}
#elif defined(DN_SESS_TU_1536)
void launch_sess_frame_1536(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    launch_sess_frame_n<1536>(d, c, a, bf16, st, phase_in);
}
#elif defined(DN_SESS_TU_512)
void launch_sess_frame_512(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    launch_sess_frame_n<512>(d, c, a, bf16, st, phase_in);
}
#else
void launch_sess_frame_1536(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in);     // (dn_sessions1536.hip)
void launch_sess_frame_512(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in);      // (dn_sessions512.hip)

void launch_sess_frame(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in) {
    if (d.n_fft == 1536) launch_sess_frame_1536(d, c, a, bf16, st, phase_in);
    else if (d.n_fft == 512) launch_sess_frame_512(d, c, a, bf16, st, phase_in);
    else launch_sess_frame_n<1024>(d, c, a, bf16, st, phase_in);
}

// (re)open: slot ids[i] gets a zero ring, overlap-add line and hx, zero counters and the stream id sids_in[i]
__global__ void sess_open_kernel(SessArgs a, const uint64_t* sids_in, int n_fft) {
    const size_t s = (size_t)a.ids[blockIdx.x];
    for (int k = threadIdx.x; k < n_fft; k += blockDim.x) {
        a.ring[s * n_fft + k] = 0.0f;
        a.ola[s * n_fft + k] = 0.0f;
    }
    for (int k = threadIdx.x; k < kHidden * a.C; k += blockDim.x) a.hx[s * kHidden * a.C + k] = 0.0f;
    if (threadIdx.x == 0) {
        a.frames[s] = 0;
        a.pushes[s] = 0;
        a.sids[s] = sids_in[blockIdx.x];
    }
}
void launch_sess_open(const SessArgs& a, const uint64_t* sids_in, int n_fft, hipStream_t st) {
    hipLaunchKernelGGL(sess_open_kernel, dim3(a.n), dim3(256), 0, st, a, sids_in, n_fft);
}

// ---- session records (dn_sessions_export / dn_sessions_import).  Workgroup i moves the record of row i: slot ids[i] <-> records + i * stride.
// The lines go 16 bytes a lane (n_fft % 4 == 0, the pool's lines and the records 16-byte aligned); hx is [17][C] at a slot stride of 68 C bytes,
// not 16-byte aligned, so it goes a float a lane.  Header and counters are plain stores of thread 0.
constexpr int kSessRecThreads = 256;

// export: the slot's state into its record; the pool is only read
__global__ __launch_bounds__(kSessRecThreads) void sess_export_kernel(SessArgs a, SessRec r, int n_fft, char* records) {
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    char* rec = records + i * r.stride;
    const float4* ring = reinterpret_cast<const float4*>(a.ring + s * n_fft);
    const float4* ola = reinterpret_cast<const float4*>(a.ola + s * n_fft);
    float4* ring_r = reinterpret_cast<float4*>(rec + kSessRecHead);
    float4* ola_r = reinterpret_cast<float4*>(rec + r.ola_off);
    for (int k = tid; k < n_fft / 4; k += kSessRecThreads) {
        ring_r[k] = ring[k];
        ola_r[k] = ola[k];
    }
    const int nh = kHidden * a.C;
    const float* hx = a.hx + s * nh;
    float* hx_r = reinterpret_cast<float*>(rec + r.hx_off);
    for (int k = tid; k < nh; k += kSessRecThreads) hx_r[k] = hx[k];
    // the padding behind hx is zero: a record's bytes are a function of the session's state alone
    uint32_t* tail = reinterpret_cast<uint32_t*>(rec);
    for (size_t k = (r.hx_off + 4 * (size_t)nh) / 4 + tid; k < r.stride / 4; k += kSessRecThreads) tail[k] = 0u;
    if (tid == 0) {
        dn_session_record_header h = r.want;
        h.pushes = a.pushes[s];
        h.reserved0 = 0;
        h.frames = a.frames[s];
        h.stream_id = a.sids[s];
        h.reserved1 = 0;
        *reinterpret_cast<dn_session_record_header*>(rec) = h;
    }
}

// check: thread i compares record i's header with the pool's and leaves 0 or the first fault in status[i] (page-locked: the host reads it
// after one synchronisation)
__global__ __launch_bounds__(kSessRecThreads) void sess_check_kernel(SessRec r, int n, const char* records, uint32_t* status) {
    const size_t i = (size_t)blockIdx.x * kSessRecThreads + threadIdx.x;
    if (i >= (size_t)n) return;
    const uint4* hv = reinterpret_cast<const uint4*>(records + i * r.stride);
    const uint4 w0 = hv[0], w1 = hv[1], w2 = hv[2];              // magic version sr n_fft | hop n_mels hidden C | pushes ...
    uint32_t bad = 0;
    if (w0.x != r.want.magic) bad = kSessRecBadMagic;
    else if (w0.y != r.want.version) bad = kSessRecBadVersion;
    else if (w0.z != r.want.sample_rate || w0.w != r.want.n_fft || w1.x != r.want.hop || w1.y != r.want.n_mels || w1.z != r.want.hidden ||
             w1.w != r.want.C) bad = kSessRecBadGeometry;
    else if (w2.x > r.prime) bad = kSessRecBadPushes;
    status[i] = bad;
}

// import: record i's state into slot ids[i] (sids_in: the caller's stream ids, or null: the recorded ones)
__global__ __launch_bounds__(kSessRecThreads) void sess_import_kernel(SessArgs a, SessRec r, int n_fft, const char* records, const uint64_t* sids_in) {
    const int tid = threadIdx.x;
    const size_t i = blockIdx.x;
    const size_t s = (size_t)a.ids[i];
    const char* rec = records + i * r.stride;
    const float4* ring_r = reinterpret_cast<const float4*>(rec + kSessRecHead);
    const float4* ola_r = reinterpret_cast<const float4*>(rec + r.ola_off);
    float4* ring = reinterpret_cast<float4*>(a.ring + s * n_fft);
    float4* ola = reinterpret_cast<float4*>(a.ola + s * n_fft);
    for (int k = tid; k < n_fft / 4; k += kSessRecThreads) {
        ring[k] = ring_r[k];
        ola[k] = ola_r[k];
    }
    const int nh = kHidden * a.C;
    const float* hx_r = reinterpret_cast<const float*>(rec + r.hx_off);
    float* hx = a.hx + s * nh;
    for (int k = tid; k < nh; k += kSessRecThreads) hx[k] = hx_r[k];
    if (tid == 0) {
        const dn_session_record_header* h = reinterpret_cast<const dn_session_record_header*>(rec);
        a.pushes[s] = h->pushes;
        a.frames[s] = h->frames;
        a.sids[s] = sids_in != nullptr ? sids_in[i] : h->stream_id;
    }
}

void launch_sess_export(const SessArgs& a, const SessRec& r, int n_fft, void* records, hipStream_t st) {
    hipLaunchKernelGGL(sess_export_kernel, dim3(a.n), dim3(kSessRecThreads), 0, st, a, r, n_fft, static_cast<char*>(records));
}
void launch_sess_check(const SessArgs& a, const SessRec& r, const void* records, uint32_t* status, hipStream_t st) {
    hipLaunchKernelGGL(sess_check_kernel, dim3((a.n + kSessRecThreads - 1) / kSessRecThreads), dim3(kSessRecThreads), 0, st, r, a.n,
                       static_cast<const char*>(records), status);
}
void launch_sess_import(const SessArgs& a, const SessRec& r, int n_fft, const void* records, const uint64_t* sids_in, hipStream_t st) {
    hipLaunchKernelGGL(sess_import_kernel, dim3(a.n), dim3(kSessRecThreads), 0, st, a, r, n_fft, static_cast<const char*>(records), sids_in);
}
#endif

}  // namespace dn
