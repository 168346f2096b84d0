// dn_clip_kernels.hpp -- clip mode: N consecutive hops of B streams in ONE call (dn_clip_process), for a caller that already holds the audio.
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
// A ragged call (dn_clip_process_ragged: stream b runs n_hops[b] hops) is the same launches on F = sum n_hops frames, f = off[b] + i, off the
// running sum of n_hops: the table off [B + 1] | frame0 [B] heads the workspace, a frame finds its stream by bisection in it (clip_frame below),
// its seed is seed + frame0[b] + i, hops_in / hops_out are packed in frame order, and a stream without hops is not touched.  Every kernel picks
// the form by a branch on the table pointer, a kernel argument: behind it the uniform call computes what it did.
//
// Two translation units (Makefile): dn_clip.hip (the kernels below, clip_invmel_kernel, clip_fold_kernel and launch_clip) and dn_clip_glw.hip
// (clip_chain_glw_kernel) for the wavefront-per-frame chains under iterative-ILP scheduling, as the other kernels built on glw_body.  (No clip
// kernel has probe arrays of its own, so the stamped diagnostic build keeps the same two units.)
#pragma once
#include "dn_dispatch.hpp"
#include "dn_hop_common.hpp"

namespace dn {

void launch_clip_chains_glw(const DspDev& d, const ClipArgs& a, hipStream_t st);          // (dn_clip_glw.hip)

// ---- frame -> (stream, hop).  A uniform call (dn_clip_process) has f = b N + i.  A ragged call (dn_clip_process_ragged; a.off non-null) finds the
// stream that owns f in off[0 .. B], off[0] = 0 <= f < off[B] = frames, by bisection: the UPPER bound of f less one, the last b with off[b] <= f.
// Zero-length streams make equal neighbours in off; of a run of them and the live stream behind it that bound is the live one, off[b] <= f < off[b + 1].
// At most ceil(log2 B) steps; every caller passes an f the compiler knows to be the same for the whole wavefront (blockIdx, a readfirstlane'd wave
// index), so the loads of the search stay scalar.  The branch on the table pointer is a kernel argument's: uniform.
// The table is complete before the call's first launch and no kernel writes it, which the compiler cannot see behind a pointer in ClipArgs (a
// uniform read through it becomes a vector load and a readfirstlane): the kernels read it through the constant address space.
#if defined(__HIP_DEVICE_COMPILE__)
template <typename T> using ClipTable = const __attribute__((address_space(4))) T*;
#define DN_CLIP_TABLE(T, p) ((ClipTable<T>)(p))
#else
template <typename T> using ClipTable = const T*;
#define DN_CLIP_TABLE(T, p) (p)
#endif
__device__ __forceinline__ int clip_owner(const int* table, int B, int f) {
    const ClipTable<int> off = DN_CLIP_TABLE(int, table);
    int lo = 0, hi = B;          // off[lo] <= f < off[hi]
    while (hi - lo > 1) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (off[mid] <= f) lo = mid;
        else hi = mid;
    }
    return lo;
}
struct ClipFrame { size_t b, i; uint64_t seed; };          // frame f is hop i of stream b and draws from (seed, sid0 + b)
__device__ __forceinline__ ClipFrame clip_frame(const ClipArgs& a, size_t f) {
    ClipFrame c;
    if (a.off != nullptr) {
        const int b = clip_owner(a.off, a.B, (int)f);
        c.b = (size_t)b;
        c.i = f - (size_t)DN_CLIP_TABLE(int, a.off)[b];
        c.seed = a.seed + DN_CLIP_TABLE(uint64_t, a.frame0)[b] + c.i;
    } else {
        c.b = f / (size_t)a.N;
        c.i = f - c.b * (size_t)a.N;
        c.seed = a.seed + c.i;
    }
    return c;
}

// ---- 1. analysis: workgroup f = b N + i (ragged: off[b] + i) stages frame i of stream b and runs P1-P6 on it
// PHIN (DN_PHASE_FROM_INPUT): it also stores the unit phasors of the frame's STFT in the workspace's phasor row f, which launch_clip hands the chains of
// either layout as their init (two kernel boundaries later).
template <int NFFT, bool PHIN>
__global__ __launch_bounds__(kHopPipeThreads) void clip_analysis_kernel(DspDev d, ClipArgs a) {
    constexpr int kNR = NFFT, kHop = NFFT / 2, kLine4 = kNR / 4, kHop4 = kHop / 4;
    static_assert(kLine4 <= 2 * kHopPipeThreads, "two float4 per thread cover the frame");
    __shared__ __attribute__((aligned(16))) char smem[stft_smem<NFFT>()];
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const ClipFrame c = clip_frame(a, f);
    const size_t b = c.b, i = c.i;
    float* row = a.fr + f * a.fr_stride;
    // sample j of the frame is sample (i + 1) hop + j of concat(ring[b], hops_in[b]): the ring's second half in front of frame 0 only
    const float4* r4 = reinterpret_cast<const float4*>(a.ring + b * kNR);
    const size_t in0 = (f - i) * kHop;          // the stream's first new sample: its frame 0 is b N, or off[b]
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j4 = tid + kHopPipeThreads * r;
        if (j4 >= kLine4) continue;
        float4 v;
        if (i == 0 && j4 < kHop4) v = r4[kHop4 + j4];
        else {
            const size_t at = in0 + (i == 0 ? 0 : (i - 1) * kHop) + 4 * (size_t)(i == 0 ? j4 - kHop4 : j4);
            v = pcm_load4(a.hops_in, a.in_s16, at);
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
    // ragged: the stream's frames are off[b] .. off[b + 1]; one without hops leaves before it touches its ring
    const size_t f0 = a.off != nullptr ? (size_t)DN_CLIP_TABLE(int, a.off)[b] : b * (size_t)a.N;
    const int N = a.off != nullptr ? DN_CLIP_TABLE(int, a.off)[b + 1] - DN_CLIP_TABLE(int, a.off)[b] : a.N;
    if (N == 0) return;
    {   // the new ring is the last n_fft samples of concat(ring, hops_in): the stream's last frame (launch 1 has read every frame's samples)
        const float4* last = reinterpret_cast<const float4*>(a.fr + (f0 + N - 1) * a.fr_stride);
        float4* r4 = reinterpret_cast<float4*>(a.ring + b * (size_t)a.n_fft);
        for (int k = tid; k < a.n_fft / 4; k += kHopPipeThreads) r4[k] = last[k];
    }
    float* hx = a.hx + b * kHidden * a.C;
    const size_t M3 = 3 * (size_t)a.n_mels;
#pragma unroll 1
    for (int i = 0; i < N; ++i) {
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
    const ClipFrame c = clip_frame(a, f);
    const size_t M3 = 3 * (size_t)d.n_mels;
    const v2f* init = a.init != nullptr ? reinterpret_cast<const v2f*>(a.init) + f * 3 * kBins : nullptr;
    gl_body<NFFT, true, false, false, true>(smem, d, a.mel + f * M3, a.diff + f * M3, init, c.seed, a.sid0 + c.b, nullptr, a.fr + f * a.fr_stride,
                                            a.n_iter, a.mom, 0, tid);
}

}  // namespace dn
