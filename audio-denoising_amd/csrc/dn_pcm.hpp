// dn_pcm.hpp -- the PCM conventions at the stream boundary and the overlap-add term of P12, once.  Every front end of the hop path (frame and
// stream steps, pipes, hop groups, session pools, clip mode) and the resampler's int16 I/O call these, so they give the same bits by construction.
//   int16 in:   x / iinfo(int16).max, a true division                                              (app3.py:172)
//   int16 out:  np.clip(x, -1, 1) * iinfo(int16).max, astype(int16) = truncation                   (app3.py:244-245)
//   no frame:   a hop of zeros, the reference's ola[:hop] before any frame has been folded in      (app3.py:133,219)
//   P12:        ola <- fma(frame x 1/envelope, peak, old): the ROUNDED product first, then one fma (app3.py:217-224)
// `s16` says which type a buffer holds; `at`, `row`, `hop` and `i` count samples of that type.  The callers keep their own loop strides and store
// widths.  The shapes of the arguments are what leaves every kernel the code it was (tools/same_code.py): change them with that check at hand.
#pragma once
#include <dn_cpx.hpp>

namespace dn {

constexpr float kPcmMax = 32767.0f;          // iinfo(int16).max

__device__ __forceinline__ float pcm_f32(short q) { return (float)q / kPcmMax; }
__device__ __forceinline__ float4 pcm_f32(const short4& q) { return make_float4(pcm_f32(q.x), pcm_f32(q.y), pcm_f32(q.z), pcm_f32(q.w)); }
__device__ __forceinline__ short pcm_s16(float v) { return (short)(fminf(fmaxf(v, -1.0f), 1.0f) * kPcmMax); }
__device__ __forceinline__ unsigned int pcm_s16_pair(float v0, float v1) {
    return (unsigned int)(unsigned short)pcm_s16(v0) | ((unsigned int)(unsigned short)pcm_s16(v1) << 16);
}

// one sample, and four on an 8-byte (int16) or 16-byte (float32) boundary
__device__ __forceinline__ float pcm_load(const void* in, int s16, size_t at) {
    return s16 ? pcm_f32(static_cast<const short*>(in)[at]) : static_cast<const float*>(in)[at];
}
__device__ __forceinline__ float4 pcm_load4(const void* in, int s16, size_t at) {
    if (s16) return pcm_f32(*reinterpret_cast<const short4*>(static_cast<const short*>(in) + at));
    return *reinterpret_cast<const float4*>(static_cast<const float*>(in) + at);
}

// sample i of row `row` of out [..][hop]; a pair on an even sample as ONE 4-byte (int16) or 8-byte (float32) store (the buffer may be host memory
// behind PCIe).  (The index is formed per sample type, as the kernels always formed it: formed once in front of both, they compile to other code.)
__device__ __forceinline__ void pcm_store(void* out, int s16, size_t row, int hop, int i, float v) {
    if (s16) static_cast<short*>(out)[row * hop + i] = pcm_s16(v);
    else static_cast<float*>(out)[row * hop + i] = v;
}
__device__ __forceinline__ void pcm_store_pair(void* out, int s16, size_t row, int hop, int i, v2f v) {
    if (s16) *reinterpret_cast<unsigned int*>(static_cast<short*>(out) + row * hop + i) = pcm_s16_pair(v[0], v[1]);
    else *reinterpret_cast<v2f*>(static_cast<float*>(out) + row * hop + i) = v;
}
__device__ __forceinline__ void pcm_store_pair(void* out, int s16, size_t at, v2f v) { pcm_store_pair(out, s16, at, 1, 0, v); }          // the pair at sample `at`

// nothing to emit yet: row `row` of out [..][hop] <- 0, by `threads` threads
__device__ __forceinline__ void pcm_zero_hop(void* out, int s16, size_t row, int hop, int tid, int threads) {
    for (int n = tid; n < hop; n += threads) {
        if (s16) static_cast<short*>(out)[row * hop + n] = 0;
        else static_cast<float*>(out)[row * hop + n] = 0.0f;
    }
}

// the overlap-add term: e is the rounded product frame x 1/envelope (formed here, or staged in memory by an earlier launch)
__device__ __forceinline__ float ola_term(float e, float peak, float old) { return fmaf(e, peak, old); }
__device__ __forceinline__ v2f ola_term(v2f e, float peak, v2f old) { return mk2(fmaf(e[0], peak, old[0]), fmaf(e[1], peak, old[1])); }
__device__ __forceinline__ float ola_term(float frame, float inv_env, float peak, float old) { return ola_term(frame * inv_env, peak, old); }
__device__ __forceinline__ v2f ola_term(v2f frame, v2f inv_env, float peak, v2f old) {
    return ola_term(mk2(frame[0] * inv_env[0], frame[1] * inv_env[1]), peak, old);
}

}  // namespace dn
