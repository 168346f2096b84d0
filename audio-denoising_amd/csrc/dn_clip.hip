// dn_clip.hip -- clip mode: N consecutive hops of B streams in ONE call (dn_clip_process), for a caller that already holds the audio.
//
// A stream is a serial chain of hops only through hx: hop i + 1 needs hop i's hidden state and nothing else.  With the whole clip in hand the
// analysis of all N frames runs at once, the N model forwards run back to back in one workgroup per stream, and all B x N Griffin-Lim chains
// (~3/4 of a hop's work) spread over the GPU instead of queueing behind each other.  A call is a fixed number of launches, whatever N:
//
//   1. clip_analysis_kernel   grid B N     frame i of stream b = samples [(i+1) hop, (i+1) hop + n_fft) of concat(ring[b], hops_in[b]) -> the
//                                          workspace's frame row (int16 converted on the way), then P1-P6 (stft_body) -> mel, peak
//   2. clip_model_kernel      grid B       the stream's new ring (= its last frame: every frame has been read by now), then cell_body N times,
//                                          hx handed on in place -> residual
//   3. chains, one per (stream, hop), whole (P8-P11), the frame x 1/envelope left unscaled in the workspace's frame row:
//      clip_chain_kernel        grid B N        a wavefront per column (gl_body, the inverse mel as its prologue), every n_fft
//      clip_invmel_kernel +     grid B N        n_fft 1024: the inverse mel into the frame row (invmel_body), then a wavefront per frame, four
//      clip_chain_glw_kernel    grid ceil(B N / 4)   frames a workgroup (glw_body; dn_clip_glw.hip) -- five launches in this form
//   4. clip_fold_kernel       elementwise  the overlap-add across hops: what N applications of gl_body<.., STREAM>'s epilogue compute, in the
//                                          same order and rounding
//
// Every body is called with its pointers offset to the frame's rows and b = 0 (sid0 = the stream's id), as dn_sessions.hip does: hops out, ring, ola
// and hx are the bits N calls of dn_stream_step give.
//
// Workspace, per frame f = b N + i: a frame row of kStride floats (the samples; n_fft 1024 per stream: then the linear magnitudes [3][513]; then
// the finished frame x 1/envelope), mel [3][M], residual [3][M], peak.
//
// Two translation units (Makefile): this file, and dn_clip_glw.hip (DN_CLIP_TU_GLW) for the wavefront-per-frame chains under iterative-ILP
// scheduling, as the other kernels built on glw_body.
#include "dn_hop_common.hpp"

namespace dn {

#if defined(DN_CLIP_TU_GLW)
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
    const size_t b = f / (size_t)a.N, i = f - b * (size_t)a.N;
    float* row = a.fr + f * a.fr_stride;
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + f * 3 * kBins : nullptr;
    glw_body<kNR, kEmitStage>(smem, d, row, init, a.seed + i, a.sid0 + b, nullptr, nullptr, a.n_iter, a.mom, 0, lane, wv, nullptr, nullptr, 0, 0, -1,
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
#else
void launch_clip_chains_glw(const DspDev& d, const ClipArgs& a, hipStream_t st);          // (dn_clip_glw.hip)

// ---- 1. analysis: workgroup f = b N + i stages frame i of stream b and runs P1-P6 on it
// PHIN (DN_PHASE_FROM_INPUT): it also stores the unit phasors of the frame's STFT in the workspace's phasor row f, which launch_clip hands the chains of
// either layout as their init (two kernel boundaries later).
template <int NFFT, bool PHIN>
__global__ __launch_bounds__(kHopPipeThreads) void clip_analysis_kernel(DspDev d, ClipArgs a) {
    constexpr int kNR = NFFT, kHop = NFFT / 2, kLine4 = kNR / 4, kHop4 = kHop / 4;
    static_assert(kLine4 <= 2 * kHopPipeThreads, "two float4 per thread cover the frame");
    __shared__ __attribute__((aligned(16))) char smem[stft_smem<NFFT>()];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const size_t b = f / (size_t)a.N, i = f - b * (size_t)a.N;
    float* row = a.fr + f * a.fr_stride;
    // sample j of the frame is sample (i + 1) hop + j of concat(ring[b], hops_in[b]): the ring's second half in front of frame 0 only
    const float4* r4 = reinterpret_cast<const float4*>(a.ring + b * kNR);
    const size_t in0 = b * (size_t)a.N * kHop;          // the stream's first new sample
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j4 = tid + kHopPipeThreads * r;
        if (j4 >= kLine4) continue;
        float4 v;
        if (i == 0 && j4 < kHop4) v = r4[kHop4 + j4];
        else {
            const size_t at = in0 + (i == 0 ? 0 : (i - 1) * kHop) + 4 * (size_t)(i == 0 ? j4 - kHop4 : j4);
            if (a.in_s16) {      // int16 -> float32 / iinfo(int16).max   (app3.py:172, as ring_shift)
                const short4 q = *reinterpret_cast<const short4*>(static_cast<const short*>(a.hops_in) + at);
                v = make_float4((float)q.x / 32767.0f, (float)q.y / 32767.0f, (float)q.z / 32767.0f, (float)q.w / 32767.0f);
            } else {
                v = *reinterpret_cast<const float4*>(static_cast<const float*>(a.hops_in) + at);
            }
        }
        reinterpret_cast<float4*>(row)[j4] = v;
    }
    __syncthreads();
    stft_body<NFFT, false, true, kHopPipeThreads, PHIN>(smem, d, row, nullptr, a.mel + f * 3 * d.n_mels, a.peak + f, DN_PEAK_NORMALIZE | DN_PRE_WINDOW, 0, tid,
                                                        PHIN ? reinterpret_cast<float2*>(a.phas) + f * 3 * Geo<NFFT>::kBins : nullptr);   // P1-P6
}

// ---- 2. model: workgroup b runs the stream's N forwards back to back (P7), hx in place
template <bool BF16, int CT>
__global__ __launch_bounds__(kHopPipeThreads) void clip_model_kernel(const CellDev* __restrict__ cp, ClipArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kCellSmem];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const size_t f0 = b * (size_t)a.N;
    {   // the new ring is the last n_fft samples of concat(ring, hops_in): the stream's last frame (launch 1 has read every frame's samples)
        const float4* last = reinterpret_cast<const float4*>(a.fr + (f0 + a.N - 1) * a.fr_stride);
        float4* r4 = reinterpret_cast<float4*>(a.ring + b * (size_t)a.n_fft);
        for (int k = tid; k < a.n_fft / 4; k += kHopPipeThreads) r4[k] = last[k];
    }
    float* hx = a.hx + b * kHidden * a.C;
    const size_t M3 = 3 * (size_t)a.n_mels;
#pragma unroll 1
    for (int i = 0; i < a.N; ++i) {
        // The loop encloses one large inlined stage whose table loads are all loop-invariant: the model's view is rebased every hop by a zero the
        // compiler cannot see through, so the stage loads what it needs where it needs it (dn_group.hip: hoisted, they spill).
        int z;
        DN_OPAQUE_ZERO(z);
        const CellDev& cz = cp[z];
        cell_body<kHopPipeThreads / 64, BF16, CT>(smem, cz, a.mel + (f0 + i) * M3, hx + z, a.diff + (f0 + i) * M3, hx + z, 3, a.C, 0, tid + z);
        __syncthreads();          // the next hop reuses the LDS stages and reads the hx this one stored
    }
}

// ---- 3a. chains, a wavefront per column: workgroup f runs P8-P11 of frame f whole (gl_body with the inverse mel as its prologue) and leaves the
// frame x 1/envelope, unscaled, in the frame row
template <int NFFT>
__global__ __launch_bounds__(kHopThreads, NFFT == 1536 ? 2 : 1) void clip_chain_kernel(DspDev d, ClipArgs a) {
    constexpr int kBins = Geo<NFFT>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[gl_smem<NFFT>()];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const size_t b = f / (size_t)a.N, i = f - b * (size_t)a.N;
    const size_t M3 = 3 * (size_t)d.n_mels;
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + f * 3 * kBins : nullptr;
    gl_body<NFFT, true, false, false, true>(smem, d, a.mel + f * M3, a.diff + f * M3, init, a.seed + i, a.sid0 + b, nullptr, a.fr + f * a.fr_stride,
                                            a.n_iter, a.mom, 0, tid);
}

// ---- 3b. n_fft 1024, in front of the wavefront-per-frame chains: P8-P10 of frame f into its frame row (the samples are not needed any more)
__global__ __launch_bounds__(kHopPipeThreads) void clip_invmel_kernel(DspDev d, ClipArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kInvSmem];
    const size_t f = blockIdx.x;
    const size_t M3 = 3 * (size_t)d.n_mels;
    invmel_body<1024, true, kHopPipeThreads>(smem, d, a.mel + f * M3, a.diff + f * M3, a.fr + f * a.fr_stride, 3, 0, threadIdx.x);
}

// ---- 4. fold: the overlap-add across hops.  E_i = frame row of hop i (frame x 1/envelope), s_i its peak, lo = [:hop], hi = [hop:]:
//   out_0 = ola_in.lo     out_1 = fma(E_0.lo, s_0, ola_in.hi)     out_i = fma(E_{i-1}.lo, s_{i-1}, fma(E_{i-2}.hi, s_{i-2}, 0))
//   ola.lo = fma(E_{N-1}.lo, s_{N-1}, h), h = fma(E_{N-2}.hi, s_{N-2}, 0) (N = 1: ola_in.hi)     ola.hi = fma(E_{N-1}.hi, s_{N-1}, 0)
// which is what N applications of the epilogue of gl_body<.., STREAM> leave, operation for operation.  A thread owns one sample pair of one job
// of one stream; job 0 is everything that touches the stream's overlap-add line (out_0, out_1, the new line: the pair's old samples are in
// registers before the thread rewrites them, and no other thread reads them), job j >= 1 is out_{j+1}.
constexpr int kClipFoldThreads = 256;
__device__ __forceinline__ void clip_emit(void* out, int s16, size_t at, v2f v) {
    if (s16) {
        const float c0 = fminf(fmaxf(v[0], -1.0f), 1.0f) * 32767.0f, c1 = fminf(fmaxf(v[1], -1.0f), 1.0f) * 32767.0f;   // np.clip, * iinfo(int16).max
        // astype(int16): truncation; the pair goes out as one 4-byte store
        *reinterpret_cast<unsigned int*>(static_cast<short*>(out) + at) = (unsigned int)(unsigned short)(short)c0 | ((unsigned int)(unsigned short)(short)c1 << 16);
    } else {
        *reinterpret_cast<v2f*>(static_cast<float*>(out) + at) = v;
    }
}
__global__ __launch_bounds__(kClipFoldThreads) void clip_fold_kernel(ClipArgs a) {
    const int hop = a.n_fft / 2, pairs = hop / 2;
    const size_t jobs = a.N > 1 ? (size_t)a.N - 1 : 1;
    const size_t u = (size_t)blockIdx.x * kClipFoldThreads + threadIdx.x;
    if (u >= (size_t)a.B * jobs * pairs) return;
    const int m = (int)(u % pairs);
    const size_t bj = u / pairs, b = bj / jobs, j = bj - b * jobs;
    const size_t f0 = b * (size_t)a.N;
    const int n = 2 * m;
    auto pair = [&](size_t i, int off) { return *reinterpret_cast<const v2f*>(a.fr + (f0 + i) * a.fr_stride + off + n); };
    auto fma2 = [](v2f e, float s, v2f c) { return mk2(fmaf(e[0], s, c[0]), fmaf(e[1], s, c[1])); };
    const v2f zero = mk2(0.0f, 0.0f);
    const size_t out0 = f0 * hop + n;          // the pair in hop 0 of the stream's output row
    if (j == 0) {
        float* orow = a.ola + b * (size_t)a.n_fft;
        const v2f lo = *reinterpret_cast<const v2f*>(orow + n), hi = *reinterpret_cast<const v2f*>(orow + hop + n);
        clip_emit(a.hops_out, a.out_s16, out0, lo);
        const v2f first = fma2(pair(0, 0), a.peak[f0], hi);          // hop 0's frame on the old line
        v2f nlo = first;
        if (a.N > 1) {
            clip_emit(a.hops_out, a.out_s16, out0 + hop, first);
            const size_t l = (size_t)a.N - 1;
            nlo = fma2(pair(l, 0), a.peak[f0 + l], fma2(pair(l - 1, hop), a.peak[f0 + l - 1], zero));
        }
        const size_t l = (size_t)a.N - 1;
        const v2f nhi = fma2(pair(l, hop), a.peak[f0 + l], zero);
        *reinterpret_cast<v2f*>(orow + n) = nlo;
        *reinterpret_cast<v2f*>(orow + hop + n) = nhi;
    } else {
        const size_t i = j + 1;
        clip_emit(a.hops_out, a.out_s16, out0 + i * hop, fma2(pair(i - 1, 0), a.peak[f0 + i - 1], fma2(pair(i - 2, hop), a.peak[f0 + i - 2], zero)));
    }
}

void launch_clip(const DspDev& d, const CellDev* c_dev, const ClipArgs& args, bool bf16, hipStream_t st) {
    ClipArgs a = args;
    if (a.phas != nullptr) a.init = a.phas;          // input-phase mode: the chains start from the phasors the analysis stores
    const dim3 frames((unsigned)a.frames), block(kHopPipeThreads);
    auto sized = [&](auto k512, auto k1024, auto k1536, dim3 blk) {
        if (d.n_fft == 512) hipLaunchKernelGGL(k512, frames, blk, 0, st, d, a);
        else if (d.n_fft == 1536) hipLaunchKernelGGL(k1536, frames, blk, 0, st, d, a);
        else hipLaunchKernelGGL(k1024, frames, blk, 0, st, d, a);
    };
    if (a.phas != nullptr) sized(clip_analysis_kernel<512, true>, clip_analysis_kernel<1024, true>, clip_analysis_kernel<1536, true>, block);
    else sized(clip_analysis_kernel<512, false>, clip_analysis_kernel<1024, false>, clip_analysis_kernel<1536, false>, block);
    const int usual = d.n_fft == 1024 ? 5 : 4;
    auto model = [&](auto k) { hipLaunchKernelGGL(k, dim3(a.B), block, 0, st, c_dev, a); };
    if (a.C == usual && usual == 5) { if (bf16) model(clip_model_kernel<true, 5>); else model(clip_model_kernel<false, 5>); }
    else if (a.C == usual) { if (bf16) model(clip_model_kernel<true, 4>); else model(clip_model_kernel<false, 4>); }
    else { if (bf16) model(clip_model_kernel<true, 0>); else model(clip_model_kernel<false, 0>); }
    if (a.per_stream) {
        hipLaunchKernelGGL(clip_invmel_kernel, frames, block, 0, st, d, a);
        launch_clip_chains_glw(d, a, st);
    } else {
        sized(clip_chain_kernel<512>, clip_chain_kernel<1024>, clip_chain_kernel<1536>, dim3(kHopThreads));
    }
    const size_t jobs = a.N > 1 ? (size_t)a.N - 1 : 1;
    const size_t units = (size_t)a.B * jobs * (a.n_fft / 4);
    hipLaunchKernelGGL(clip_fold_kernel, dim3((unsigned)((units + kClipFoldThreads - 1) / kClipFoldThreads)), dim3(kClipFoldThreads), 0, st, a);
}
#endif

}  // namespace dn
