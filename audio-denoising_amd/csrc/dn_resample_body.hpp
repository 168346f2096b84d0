// dn_resample_body.hpp -- what the resampler's kernel families share (dn_resample.hip, dn_ratebank.hip): the virtual input of a row, the staging
// of a tile into LDS, the paired store, and the chain of one block of the small form.  One output is ONE chain acc = fmaf(k[p][j], v[q o + j], acc),
// j ascending from acc = 0: rs_small_block is that chain, and every kernel of the small form calls it, so they give the same bits by construction.
#pragma once
#include "dn_internal.hpp"
#include "dn_pcm.hpp"

namespace dn {

constexpr int kRsTileMax = (kRsTileQ - 1) * kRsSmallMaxO + kRsSmallMaxTable;            // samples of the small form's input tile at most

// where sample i of a tile lies in LDS: skewed by one word every 32 for even o (dn_resample.hip), plain for odd o
template <bool SKEW>
__device__ __forceinline__ int rs_pos(int i) { return SKEW ? i + (i >> 5) : i; }

// sample i of the row's virtual input (i >= 0): history or zeros, then x, then zeros
template <bool S16>
__device__ __forceinline__ float rs_sample(const ResampleArgs& a, const void* xrow, const float* hrow, int i) {
    if (i < a.lead) return hrow ? hrow[i] : 0.0f;
    const int k = i - a.lead;
    if (k >= a.Lx) return 0.0f;
    return pcm_load(xrow, S16, k);
}

// xs[pos(i)] = v[v0 + i], i in [0, len): groups of four samples on 4-element boundaries of x, one 16-byte load (8 bytes for int16) where a group
// lies inside both the tile and the row and the rows are aligned (a.x_vec); sample by sample at the edges, in the history and beyond the row
template <bool S16, typename POS>
__device__ __forceinline__ void rs_stage(float* xs, POS pos, const ResampleArgs& a, const void* xrow, const float* hrow, int v0, int len, int tid,
                                         int threads) {
    const int k0 = v0 - a.lead, k1 = k0 + len;          // the tile in samples of x (k0 may be negative: history, or the zeros in front)
    const int ka = k0 & ~3;                             // (two's complement: rounds down for negative k0 too)
    for (int kg = ka + 4 * tid; kg < k1; kg += 4 * threads) {
        if (a.x_vec && kg >= k0 && kg >= 0 && kg + 4 <= k1 && kg + 4 <= a.Lx) {
            const float4 v = pcm_load4(xrow, S16, kg);
            const int i = kg - k0;
            xs[pos(i)] = v.x; xs[pos(i + 1)] = v.y; xs[pos(i + 2)] = v.z; xs[pos(i + 3)] = v.w;
        } else {
            for (int e = 0; e < 4; ++e) {
                const int k = kg + e;
                if (k >= k0 && k < k1) xs[pos(k - k0)] = rs_sample<S16>(a, xrow, hrow, v0 + (k - k0));
            }
        }
    }
}

// outputs m, m + 1 of a row (the second only if `two`): one 8-byte (float32) or 4-byte (int16) store where the pair starts on an even element of an
// aligned row, else element by element
__device__ __forceinline__ void rs_store2(const ResampleArgs& a, void* yrow, int m, float v0, float v1, bool two) {
    if (two && a.y_pair && (m & 1) == 0) {
        if (a.out_s16) *reinterpret_cast<unsigned int*>(static_cast<short*>(yrow) + m) = pcm_s16_pair(v0, v1);
        else *reinterpret_cast<float2*>(static_cast<float*>(yrow) + m) = make_float2(v0, v1);
        return;
    }
    if (a.out_s16) {
        static_cast<short*>(yrow)[m] = pcm_s16(v0);
        if (two) static_cast<short*>(yrow)[m + 1] = pcm_s16(v1);
    } else {
        static_cast<float*>(yrow)[m] = v0;
        if (two) static_cast<float*>(yrow)[m + 1] = v1;
    }
}

// the N outputs of the block whose taps start at sample `at` of the tile xs (table ks [N][KW], both in LDS)
template <int N, bool SKEW>
__device__ __forceinline__ void rs_small_block(const float* xs, const float* ks, int at, int KW, float (&acc)[N]) {
    for (int p = 0; p < N; ++p) acc[p] = 0.0f;
    for (int j = 0; j < KW; ++j) {
        const float xv = xs[rs_pos<SKEW>(at + j)];
        for (int p = 0; p < N; ++p) acc[p] = fmaf(ks[p * KW + j], xv, acc[p]);
    }
}

}  // namespace dn
