// dn_internal.hpp -- launcher prototypes shared between dn_api.hip and the kernel files.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dn_denoise.h"
#include "dn_plan.hpp"

// Wave-uniform read-only tables (conv weights) are read through the constant address space so that
// hipcc emits scalar loads (s_load_dwordx*, scalar cache) and the FMAs take the weight as an SGPR
// operand, instead of 64 lanes fetching the same dword through the vector memory path.
#ifndef DN_CONST_AS
#define DN_CONST_AS __attribute__((address_space(4)))
#endif

namespace dn {

typedef const DN_CONST_AS float* cfloat_ptr;

// accumulator fragment of v_mfma_f32_16x16x4_f32: lane l holds D[row = (l >> 4) * 4 + r][col = l & 15], r = 0..3
#ifndef DN_F32X4
#define DN_F32X4
typedef float f32x4 __attribute__((ext_vector_type(4)));
#endif

// Workgroup barrier that orders LDS traffic only: global loads issued before it stay in flight across it (a plain
// __syncthreads() drains vmcnt first).  For phases that hand over LDS data while prefetches for later phases are pending.
#ifndef DN_LDS_BARRIER
#define DN_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")
#endif

// Every vector-memory operation of the calling wave has completed (loads returned, stores acknowledged).
#ifndef DN_WAIT_VMEM
#define DN_WAIT_VMEM() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#endif

// Wave-wide max / sum, the result in every lane.  On the device: six DPP steps on the VALU (row_shr 1, 2, 4, 8, then the row
// broadcasts 15 and 31 leave the total in lane 63) -- __shfl_xor compiles to ds_bpermute, an LDS round trip of ~230 cycles a step.
// (DN_WAVE_REDUCE_SHFL selects the __shfl_xor form, for a build whose target has no DPP.)
#ifdef DN_WAVE_REDUCE_SHFL
__device__ __forceinline__ float wave_max(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float quad_sum(float v) {       // the sum of each aligned group of four lanes, in all four
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    return v;
}
#else
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take(float v) {       // lanes without a source keep their own value
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, v), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_take<0x111, 0xf>(v));     // row_shr:1
    v = fmaxf(v, dpp_take<0x112, 0xf>(v));     // row_shr:2
    v = fmaxf(v, dpp_take<0x114, 0xf>(v));     // row_shr:4
    v = fmaxf(v, dpp_take<0x118, 0xf>(v));     // row_shr:8   -> lane 15 of every row of 16 holds the row's max
    v = fmaxf(v, dpp_take<0x142, 0xa>(v));     // row_bcast:15 into rows 1 and 3
    v = fmaxf(v, dpp_take<0x143, 0xc>(v));     // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's max
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
// (the shifted-in operand must be 0 where a lane has no source: `old` = 0 with the lane's own value added outside)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_take0(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_take0<0x111, 0xf>(v);
    v += dpp_take0<0x112, 0xf>(v);
    v += dpp_take0<0x114, 0xf>(v);
    v += dpp_take0<0x118, 0xf>(v);
    v += dpp_take0<0x142, 0xa>(v);
    v += dpp_take0<0x143, 0xc>(v);
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float quad_sum(float v) {       // the sum of each aligned group of four lanes, in all four
    v += dpp_take0<0xB1, 0xf>(v);     // quad_perm [1,0,3,2]
    v += dpp_take0<0x4E, 0xf>(v);     // quad_perm [2,3,0,1]
    return v;
}
#endif

// Elementwise transcendentals of the front half on the hardware units (v_exp_f32 / v_log_f32 / v_sqrt_f32 / v_rcp_f32, 1 ulp each)
// instead of libm's correctly rounded sequences (30-130 instructions a call).  The front workgroup shares its SIMDs with a Griffin-Lim
// chain that wins issue arbitration, so it pays ~11 cycles per instruction it issues: these calls were ~600 of its instructions.
// Absolute errors ~1e-7 relative to values of order 1-10 (log-mel features, linear magnitudes), against a parity tolerance of 1e-4.
__device__ __forceinline__ float fast_log1p(float x) { return __builtin_amdgcn_logf(1.0f + x) * 0.693147180559945309f; }   // x >= 0 here
__device__ __forceinline__ float fast_expm1(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f) - 1.0f; }
__device__ __forceinline__ float fast_abs2(float re, float im) { return __builtin_amdgcn_sqrtf(fmaf(re, re, im * im)); }

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

constexpr int kHidden = 17;      // H
constexpr int kGates = 51;       // 3H
constexpr int kGauss = 6;        // G
constexpr int kCellChunk = 3;    // time steps whose encoder/decoder run batched (= columns per hop)
constexpr int kMaxC = 5;         // compressed bins supported by the cell kernel (51*C gate lanes <= 256; F <= 80)
// most steps of the packed mel schedule (DspDev::mel_q) a wavefront unrolls: 19 are needed for 80 mels at 16 kHz / n_fft 1024, 39 for 64 mels at
// 48 kHz / n_fft 1536 (measured: a 48-step unroll costs the n_fft-1024 hop 1 %, and gives the 1536 one 0.8 %)
constexpr int mel_q_steps(int n_fft) { return n_fft == 1536 ? 48 : 32; }
constexpr int kInvBand = 16;      // diagonals of (fb^T fb)^-1 kept on either side of the main one (DspDev::ginv_band)
constexpr int kSlotMeta = 16;     // u32 of per-stream hand-over data in a pipe's scratch slot (FrameMeta below fills ten of them)
constexpr int kGlwAutoStreams = 768;
constexpr long kSplitAutoChains = 4096;         // DN_SPLIT_AUTO: chain wavefronts per launch from which a hop goes out as two launches (measured: 2,048 -2.4 %, 4,096 +2.1 %, 8,192 +5.1 %)   // DN_GL_AUTO: from this many streams per pipe on (three per CU of an MI355X; measured crossover between 512 and 768) the back half runs a wavefront per stream
// Floats of the VALU-row weight table of a GRUUNet2 conv level (CellDev; dn_cell_body.hpp: rows_down / rows_up): `slots4` float4 of weights for each
// of the `rows` rows of the partial last row tile, in whole 256-byte lines.  It sits between the whole row tiles' fragments and the partial one's.
constexpr int cell_rowtab_floats(int rows, int slots4) { return (rows * slots4 * 4 + 63) / 64 * 64; }
constexpr int kArenaSlack = 8192; // zero bytes behind every device arena: kernels that move whole rounds of an array read past its end (dn_cell_body.hpp)

// ---- what one launch hands the next through device memory: each format once, for its writer, its readers and the host code that sizes it.
// A pipe's scratch slot, offsets in floats: mel [B][3][M] | residual [B][3][M] | peak [B] | meta [B][kSlotMeta] u32 | lin [B][3][K]
struct SlotLayout {
    size_t diff, peak, meta, lin, floats;
    __host__ __device__ constexpr SlotLayout(int B, int M, int K)
        : diff((size_t)B * 3 * M), peak(2 * diff), meta(peak + B), lin(meta + kSlotMeta * (size_t)B), floats(lin + (size_t)B * 3 * K) {}
};
static_assert(SlotLayout(256, 80, 513).floats == 256 * 2036 && SlotLayout(256, 80, 513).lin == 256 * 497, "a change of the slot layout is a deliberate edit");

// The slot's meta record of a stream, written by the frame's front workgroup and read by its Griffin-Lim workgroup in a later launch -- everything
// the pending hop is finished with is the FRAME's own, not the next call's.  Words: [0] has_init  [1,2] seed  [3,4] sid0  [5] it0  [6] n_iter
// [7] mom (bits)  [8,9] out.
struct FrameMeta {
    bool has_init;          // the frame's phases are in the slot's init area (injected, drawn by the front workgroup, or its STFT's phasors)
    uint64_t seed, sid0;    // Griffin-Lim seed; stream id of stream 0
    int it0;                // head-start iterations the front workgroup already ran
    int n_iter;
    float mom;              // momentum / (1 + momentum)
    float* out;             // where the frame goes (frame mode: the `out` of its dn_pipe_submit)
    __device__ __forceinline__ void store(uint32_t* m) const {
        m[0] = has_init ? 1u : 0u;
        m[1] = (uint32_t)seed;
        m[2] = (uint32_t)(seed >> 32);
        m[3] = (uint32_t)sid0;
        m[4] = (uint32_t)(sid0 >> 32);
        m[5] = (uint32_t)it0;
        m[6] = (uint32_t)n_iter;
        m[7] = __builtin_bit_cast(uint32_t, mom);
        const uint64_t dst = reinterpret_cast<uint64_t>(out);
        m[8] = (uint32_t)dst;
        m[9] = (uint32_t)(dst >> 32);
    }
    // Loading is field by field: a reader takes the fields it uses where it uses them (group_kernel never reads it0), between its own address
    // arithmetic -- one load of the whole record moves the loads against that and the kernels compile to other code.  The words come back through
    // the vector memory path: readfirstlane tells the compiler that it0, n_iter and mom are wave-uniform, so the iteration loop keeps a scalar
    // trip count and a scalar branch; the other fields do not take one.
    static __device__ __forceinline__ bool load_has_init(const uint32_t* m) { return m[0] != 0; }
    static __device__ __forceinline__ uint64_t load_seed(const uint32_t* m) { return (uint64_t)m[1] | ((uint64_t)m[2] << 32); }
    static __device__ __forceinline__ uint64_t load_sid0(const uint32_t* m) { return (uint64_t)m[3] | ((uint64_t)m[4] << 32); }
    static __device__ __forceinline__ int load_it0(const uint32_t* m) { return __builtin_amdgcn_readfirstlane((int)m[5]); }
    static __device__ __forceinline__ int load_n_iter(const uint32_t* m) { return __builtin_amdgcn_readfirstlane((int)m[6]); }
    static __device__ __forceinline__ float load_mom(const uint32_t* m) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane((int)m[7])); }
    static __device__ __forceinline__ float* load_out(const uint32_t* m) { return reinterpret_cast<float*>((uint64_t)m[8] | ((uint64_t)m[9] << 32)); }
};

// The chain a head start parks (gl_body writes it; gl_body or glw_body's kGlwFromX resumes it): [stream][column][parked_rows][64] complex, one
// coalesced row of 64 lanes per register of the lane's state, n_fft / 128 complex values a lane.  glw_body's own segment format fits inside it.
constexpr int parked_rows(int n_fft) { return 2 * (n_fft / 128) + 2; }                     // rows a column
constexpr size_t parked_elems(int n_fft) { return (size_t)3 * parked_rows(n_fft) * 64; }   // complex values a stream
static_assert(parked_elems(512) == 1920 && parked_elems(1024) == 3456 && parked_elems(1536) == 4992, "a change of the parked chain is a deliberate edit");
template <int NFFT> struct Parked {
    static constexpr int kNV = NFFT / 128, kNP = kNV / 2;
    // the lane's element of row 0 of column c of stream b; the rows below are offsets from it, t = 0 .. kNP - 1
    template <typename T> static __device__ __forceinline__ T* column(T* state, size_t b, int c, int lane) { return state + ((b * 3 + c) * parked_rows(NFFT)) * 64 + lane; }
    static constexpr int xlo(int t) { return 64 * t; }                       // X = angles * magnitude of bin pair t: the low bins
    static constexpr int xhi(int t) { return 64 * (kNP + t); }               //                                      the high bins
    static constexpr int xmid() { return 64 * kNV; }                         // X of bin NC / 2
    static constexpr int plo(int t) { return 64 * (kNV + 1 + t); }           // the previous rebuilt spectrum, likewise
    static constexpr int phi(int t) { return 64 * (kNV + 1 + kNP + t); }
    static constexpr int pmid() { return 64 * (2 * kNV + 1); }
    static_assert(pmid() == 64 * (parked_rows(NFFT) - 1), "the rows fill the column");
};

void launch_stft(const DspDev& d, const float* frames, float* spec, float* mel, float* peak, int B, uint32_t flags,
                 hipStream_t st);
void launch_stft_phasors(const DspDev& d, const float* frames, float* phas, int B, uint32_t flags, hipStream_t st);
void launch_mel(const DspDev& d, const float* mag, float* mel, int rows, hipStream_t st);
void launch_invmel(const DspDev& d, const float* x, const float* diff, float* lin, int rows, hipStream_t st);
void launch_griffinlim(const DspDev& d, const float* mag, const float* init, uint64_t seed, uint64_t sid0,
                       const float* scale, float* wave, int B, int n_iter, float momentum, hipStream_t st);
void launch_draw_phases(const DspDev& d, float* out, uint64_t seed, uint64_t sid0, int B, hipStream_t st);
void launch_synthesis(const DspDev& d, const float* x, const float* diff, const float* init, uint64_t seed, uint64_t sid0,
                      const float* scale, float* wave, int B, int n_iter, float momentum, hipStream_t st);
void launch_cell(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                 int C, hipStream_t st);
void launch_cell_parent_tiles(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                              int C, hipStream_t st);
// Device-resident control block of a dn_pipe.  Every launch of hop_kernel derives its scratch slot, the Griffin-Lim seed
// and whether a hop is pending from it, and its last workgroup advances it -- so a launch captured in a hipGraph can
// be replayed indefinitely (nothing that changes from hop to hop is baked into the kernel arguments).
struct PipeCtl {
    unsigned long long pushes;   // launches that carried a front half (streaming: the first n_fft/hop - 1 only fill the ring)
    unsigned long long frames;   // frames whose front half (P1-P10) has run
    unsigned long long launches; // launches of the pipe so far (submits, pushes and flushes)
    unsigned int pending;        // frames whose Griffin-Lim has not finished: the most recent `pending` ones (0/1; up to the pipe's depth)
    unsigned int done;           // workgroup ticket of the launch in flight (0 between launches)
    unsigned int slot_next;      // scratch slot the next front half writes (slots are used round robin)
    unsigned int pad_;
    unsigned long long front_launch[8];   // launch index in which frame f's front half ran, at [f & 7] (its chain segment s runs in launch + 1 + s)
};

// Arguments of the software-pipelined hop launch (dn_hop.hip).
struct HopArgs {
    PipeCtl* ctl;
    // scratch slots (n_slots of them, used round robin; depth + 1), each: mel [B][3][M] | residual [B][3][M] | peak [B] | meta [B][kSlotMeta] (u32, see
    // SlotLayout) | lin [B][3][K]; per slot also the frame's initial phases [B][3][K] complex (parity mode; or null) and its parked
    // Griffin-Lim chain (head start, chain segments; or null)
    float* slots; size_t slot_stride;
    float2* slot_init; size_t init_stride;
    float2* gl_state; size_t state_stride;
    int n_slots;
    // front half: this hop's analysis + model + inverse mel, written to slot ctl->slot_next
    const float* frames; float* hx;
    const float* init_in;    // this hop's initial phases [B][3][K] complex (copied into the slot), or null = device RNG
    uint64_t seed, sid0;     // the frame's Griffin-Lim draws from (seed + frame index, sid0 + stream)
    // these three describe THIS hop's frame too: the back half finishes a pending hop with the n_iter, momentum and destination its own front
    // workgroup left in the slot
    float* gl_out;
    int n_iter; float mom;
    // head start: the front workgroup, done with P1-P10 long before the launch ends, runs the first `gl_split` Griffin-Lim iterations of
    // ITS frame and parks the chain in the slot's gl_state; the back workgroup of the next launch resumes there (0 = no head start)
    int gl_split;
    int front_B, back_B, B, C;
    // back half: back_blocks workgroups.  A wavefront per column: back_B of them, one pending hop.  A wavefront per stream (dn_glw_body.hpp): each
    // holds spb streams x depth chain segments (spb x depth <= 4), back_blocks = ceil(back_B / spb)
    int back_blocks, spb, depth, glw;
    // split: the hop goes out as two launches (launch_hop does that: chains, then front halves); front_only marks the second of them
    int split, front_only;
    // streaming mode (pipe-owned per-stream state): the front half first shifts `hop_in` into `ring` and uses the ring
    // as its frame (app3.py:178,226); the back half folds its frame into `ola` and emits `hop_out` (app3.py:219-224)
    const void* hop_in; float* ring; int in_s16; int prime;
    float* ola; void* hop_out; int out_s16;
    // zero-copy host transport: hop_in / hop_out are page-locked HOST memory; the last workgroup of the launch, after every workgroup's stores have
    // been fenced to system scope, publishes host_done_value in *host_done (page-locked too) -- the host polls that word instead of a HIP event
    unsigned long long* host_done; unsigned long long host_done_value;
    // deferred host output (DN_HOST_DEFER): the hop the PREVIOUS push emitted sits in a device staging buffer; the front workgroup of stream b
    // moves that stream's row (host_copy_n16 / B 16-byte units) to that push's page-locked buffer before it starts on its own hop, so the PCIe
    // writes overlap the hop instead of ending it as one burst (null = nothing to move; only launches with front workgroups carry one)
    const uint4* host_copy_src; uint4* host_copy_dst; unsigned int host_copy_n16;
    // hop groups (group_kernel; dn_pipe_set_group): ONE launch carries `group_hops` consecutive new hops of every stream (their front halves run one
    // after the other in the stream's front workgroup, hx carried) and the WHOLE Griffin-Lim chains of the hops the previous launch fronted, one
    // wavefront each -- no chain is ever parked.  Hop h of the group reads frames + h * frames_stride (hop_in + h * hop_in_stride when streaming),
    // takes its injected phases from init_in + h * init_in_stride and is written to gl_out + h * out_stride; a streaming launch emits `group_out`
    // hops at hop_out + i * hop_out_stride (strides in elements of the respective type); filler_first: hops without a frame behind them (start of a
    // stream) are the leading ones of a push and the trailing ones of a flush
    int group_hops, group_out, filler_first, n_mels;
    const DspDev* d_dev; const CellDev* c_dev;          // device copies of the plan's and the model's views (group_kernel reads them where it needs them)
    long long frames_stride, out_stride, init_in_stride, hop_in_stride, hop_out_stride;
    // input-phase pipe (DN_PHASE_FROM_INPUT): the front half stores the unit phasors of its STFT in the slot's init area, nothing is drawn.  (The last
    // member: the kernel-argument offsets of everything above are what they were, so the default instantiations compile to the code they were.)
    int phase_in;
};
void launch_host_copy(const uint4* src, uint4* dst, unsigned int n16, unsigned long long* done, unsigned long long value, hipStream_t st);
void launch_hop(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);
void launch_group(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);
void launch_ctl_set(PipeCtl* ctl, unsigned long long pushes, unsigned long long frames, unsigned int pending, hipStream_t st);

// The whole hop for one batch in ONE launch, nothing overlapped (dn_process_frame / dn_stream_step).
struct FrameArgs {
    const float* frames; float* hx; float* out;
    float* mel; float* diff; float* peak;        // workspace (diff may be the caller's mel_residual_out)
    const float* init; uint64_t seed, sid0;
    int n_iter; float mom; int C;
    const float* hop_in; float* ring; float* ola; float* hop_out;    // dn_stream_step (ring != null)
    float* phas;             // DN_PHASE_FROM_INPUT: workspace rows [B][3][K] complex for the unit phasors of the analysis STFT (the chain's initial phases), else null
};
void launch_frame(const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st);
// One hop for n listed slots of a session pool (dn_sessions.hip).  Slot-indexed: ring, ola, hx and the counters; row-indexed (list order): hop_in,
// hop_out, init and the workspace.
constexpr int kSessMeta = 4;      // u32 a row the front launch of the two-launch form leaves its chain (SessMeta fills three of them)
// The record of a row: [0] the row runs a chain (0: a priming push)  [1,2] the frame's Griffin-Lim seed.  The chain launch asks runs() first -- only
// for rows of the list, and only a row that runs is loaded -- and takes both through readfirstlane (wave-uniform: a wavefront serves one row).
struct SessMeta {
    uint64_t seed;
    static __device__ __forceinline__ void store_idle(uint32_t* m) { m[0] = 0u; }          // (the seed words stay what they were)
    __device__ __forceinline__ void store(uint32_t* m) const {
        m[0] = 1u;
        m[1] = (uint32_t)seed;
        m[2] = (uint32_t)(seed >> 32);
    }
    static __device__ __forceinline__ bool runs(const uint32_t* m) { return __builtin_amdgcn_readfirstlane((int)m[0]) != 0; }
    static __device__ __forceinline__ SessMeta load(const uint32_t* m) {
        return SessMeta{(uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)m[1]) | ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)m[2]) << 32)};
    }
};
struct SessArgs {
    const int32_t* ids; int n;                                  // [n] slot of row i (device copy, validated on the host)
    float* ring; float* ola; float* hx;                         // [cap][n_fft], [cap][n_fft], [cap][17][C]
    unsigned long long* frames; unsigned long long* sids;       // [cap] frames since the slot's open, its Griffin-Lim stream id
    unsigned int* pushes;                                       // [cap] pushes since the open, counted up to `prime`
    int prime;                                                  // n_fft / hop - 1: pushes that only fill the ring
    const void* hop_in; int in_s16; void* hop_out; int out_s16; // [n][hop] float32 or int16
    const float* init;                                          // [n][3][K] complex initial phases, or null = device RNG; an input-phase pool (phase_in of the
                                                                // launchers): its phasor rows [cap][3][K] complex in list order, which the analysis WRITES
    float* mel; float* diff; float* lin; float* peak; uint32_t* meta;   // workspace rows [cap][3][M], [cap][3][M], [cap][3][K], [cap], [cap][kSessMeta]
    uint64_t seed; int n_iter; float mom; int C;
};
// (phase_in is an argument of the launchers and not a member: SessArgs, and with it the kernels' argument layout, stays what it was)
void launch_sess_frame(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in = false);
void launch_sess_split(const DspDev& d, const CellDev& c, const SessArgs& a, bool bf16, hipStream_t st, bool phase_in = false);     // n_fft 1024
void launch_sess_open(const SessArgs& a, const uint64_t* sids_in, int n_fft, hipStream_t st);
// Session records (dn_sessions_export / dn_sessions_import; layout: include/dn_denoise.h).  Record i of a call is records + i * stride and
// belongs to slot ids[i].
constexpr int kSessRecHead = 64;                                // sizeof(dn_session_record_header): the ring starts here
struct SessRec {
    size_t stride, ola_off, hx_off;                             // bytes: one record, the overlap-add line, hx
    dn_session_record_header want;                              // this pool's header (magic .. C); the counters are the slot's
    unsigned int prime;                                         // n_fft / hop - 1: the largest valid priming count
};
void launch_sess_export(const SessArgs& a, const SessRec& r, int n_fft, void* records, hipStream_t st);
// status [n] (page-locked, mapped): 0 for a valid header, else kSessRecBad*
constexpr uint32_t kSessRecBadMagic = 1, kSessRecBadVersion = 2, kSessRecBadGeometry = 3, kSessRecBadPushes = 4;
void launch_sess_check(const SessArgs& a, const SessRec& r, const void* records, uint32_t* status, hipStream_t st);
void launch_sess_import(const SessArgs& a, const SessRec& r, int n_fft, const void* records, const uint64_t* sids_in, hipStream_t st);
// N consecutive hops of B streams in one call (dn_clip.hip; dn_clip_process).  Frame f = b N + i is hop i of stream b.  Ragged
// (dn_clip_process_ragged): stream b runs off[b + 1] - off[b] hops, frame f = off[b] + i.
constexpr long kClipGlwAutoFrames = 1024;       // n_fft 1024: from this many frames (B x N) on a call runs its chains a wavefront per frame (measured, profiles/clip_time.txt: per column / per frame 0.87 at 256 frames, 1.03 at 1,024, 1.15 at 4,096, 1.28 at 24,000)
constexpr int kClipRow1024 = 1540;               // floats of a frame row at n_fft 1024: the linear magnitudes [3][513], in whole 16-byte units (else n_fft: the samples)
struct ClipArgs {
    const void* hops_in; int in_s16;                            // [B][N hop] float32 or int16
    float* ring; float* ola; float* hx;                         // [B][n_fft], [B][n_fft], [B][17][C]: advanced in place by N hops
    void* hops_out; int out_s16;                                // [B][N hop] float32 or int16
    const float* init;                                          // [B][N][3][K] complex initial phases, or null = device RNG
    uint64_t seed, sid0; int n_iter; float mom;                 // hop i of stream b draws from (seed + i, sid0 + b)
    int C, B, N, n_fft, n_mels;
    size_t frames;                                              // B x N
    float* fr; size_t fr_stride;                                // workspace: frame rows [B N][fr_stride]
    float* mel; float* diff; float* peak;                       //            [B N][3][M], [B N][3][M], [B N]
    int per_stream;                                             // chains a wavefront per frame (n_fft 1024) instead of a wavefront per column
    float* phas;                                                // DN_PHASE_FROM_INPUT: workspace rows [B N][3][K] complex, written by the analysis, the chains' init; else null
    // ragged call (dn_clip_process_ragged), else both null: stream b owns frames off[b] .. off[b + 1] (off[0] = 0, off[B] = frames; N unused), its
    // rows of hops_in / hops_out start at off[b] hop, and its hop i draws from (seed + frame0[b] + i, sid0 + b)
    const int* off; const uint64_t* frame0;                     // [B + 1], [B], at the head of the workspace
};
void launch_clip(const DspDev& d, const CellDev* c_dev, const ClipArgs& a, bool bf16, hipStream_t st);
void launch_cell_bf16(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                      int C, hipStream_t st);
void launch_cell_ex(const CellDev& c, const float* x, const float* hx_in, float* out, float* hx_out, int B, int T,
                    int C, float hx_scale, hipStream_t st);
void launch_stft_general(const DspDev& d, const float* x, float* spec, float* logmel, int B, int L, hipStream_t st);
void launch_server_rows(const DspDev& d, const float* logmel, const float* model_out, const float* spec_in, float* spec_out, int rows,
                        hipStream_t st);
void launch_istft_general(const DspDev& d, const float* spec, float* wave, int B, int T, hipStream_t st);
void launch_server_mag(const DspDev& d, const float* logmel, const float* model_out, float* mag_out, int rows, hipStream_t st);
// Griffin-Lim on [B][T][K] magnitudes, any T >= 3 (dn_glg.hip).  WHOLE: one launch, T <= kGlgWholeMax wavefronts a workgroup, x / prev / sig unused.
// STEPS: x, prev [B][T][K] complex and sig [B][hop (T - 1)] are the caller's workspace.  Both give the same bits.
constexpr int kGlgWholeMax = 8;
struct GlgArgs {
    const float* mag; const float* init; int normalize;           // init: [B][T][K] complex or null = device RNG; normalize: its unit phasors
    uint64_t seed, sid0;
    float* wave;                                                   // [B][hop (T - 1)]
    float* x; float* prev; float* sig;
    int B, T, n_iter; float mom;                                   // mom = momentum / (1 + momentum)
};
void launch_glg_whole(const DspDev& d, const GlgArgs& a, hipStream_t st);
void launch_glg_steps(const DspDev& d, const GlgArgs& a, hipStream_t st);
void launch_draw_phases_general(const DspDev& d, float* out, uint64_t seed, uint64_t sid0, int B, int T, hipStream_t st);
// Polyphase sinc resampling (dn_resample.hip; dn_resample, dn_resample_push).  A row's virtual input v is `lead` samples -- hist [B][lead], or
// zeros when hist is null -- followed by the Lx samples of x and zeros beyond; output q n + p of the row (below Ly) is ONE chain
// acc = fmaf(k[p][j], v[q o + j], acc), j ascending from acc = 0, in both kernel forms.  The whole-signal call has lead = width and no hist, a
// push lead = H and hist = the stream's state: the same body, the same bits.
constexpr int kRsSmallMaxN = 4, kRsSmallMaxO = 8, kRsSmallMaxTable = 512;       // the block-per-lane form: n <= 4, o <= 8, n KW <= 512 floats (table in LDS)
constexpr int kRsThreads = 256, kRsTileQ = 512;                                                    // small form: blocks a workgroup, two a lane
constexpr int kRsGenThreads = 128, kRsGenPhases = 2 * kRsGenThreads, kRsGenBlocks = 4;      // general form: phases and blocks a workgroup
constexpr int kRsMaxLen = 1 << 30;                                               // samples of a row, in and out: every 32-bit index stays in range
struct ResampleArgs {
    const void* x; int in_s16; long long x_stride; int Lx;      // [B][x_stride] float32 or int16 (x / 32767)
    const float* hist; int lead;                                 // [B][lead] or null
    void* y; int out_s16; long long y_stride; int Ly;            // [B][y_stride] float32 or int16 (clip, * 32767, truncate)
    const float* table;                                          // small form: [n][KW]; general form: tap-major [KW][np], np = n rounded up to even
    int o, n, KW, np;
    int B, nblk;                                                 // rows; blocks of n outputs a row: ceil(Ly / n)
    int small;                                                   // which form the handle was built for
    int x_vec, y_pair;                                           // x rows start on 4-element boundaries; y rows start on 2-element boundaries
};
void launch_resample(const ResampleArgs& a, hipStream_t st);
// state [B][H] <- the last H samples of [state | chunk], chunk [B][x_stride] with Lc >= 1 samples a row: one workgroup per stream, after the
// launch that read the old state (stream order)
void launch_resample_state(float* state, int H, const void* x, int in_s16, long long x_stride, int Lc, int B, hipStream_t st);

// Rate banks (dn_ratebank.hip; dn_ratebank_ingest, dn_ratebank_emit): one side of a bank converts a LIST of rows, row i at the rate of its own
// session, and updates that session's converter state in the same launch -- one workgroup a row, the small form's chain (dn_resample_body.hpp).
// A row of rate index r reads [state[slot][:H] | x_i[:chunk_in]] (blocks o samples), writes blocks n outputs, then state[slot][:H] <- the last H
// samples it read; a row of rate index -1 (the plan's own rate) is a conversion copy of `copy` samples and has no state.
constexpr int kRbMaxRates = 8;
constexpr int kRbMaxChunk = 1536;                // samples a row brings at most (48 kHz on a 16 kHz plan of hop 512; 96 kHz on 48 kHz / hop 768)
constexpr int kRbMaxHist = 80;                   // H at most: the small form's o = 6 : 1 has 79
constexpr int kRbTile = kRbMaxChunk + kRbMaxHist;
static_assert(kRbTile >= 1536 + 79, "the tile holds [state | chunk] of the largest accepted rate");
struct RateBankRate {
    int o, n, KW, H;                             // the side's reduced pair, taps and history
    int blocks;                                  // blocks a hop: chunk_in = blocks o samples in, chunk_out = blocks n samples out
    int table;                                   // offset of its [n][KW] table in `tables`, floats
};
struct RateBankArgs {
    const void* x; int in_s16; long long x_stride;        // [n][x_stride] float32 or int16 (x / 32767)
    void* y; int out_s16; long long y_stride;             // [n][y_stride] float32 or int16 (clip, * 32767, truncate)
    float* state; int state_stride;                       // [capacity][state_stride]
    const int* rows;                                      // [n] x (slot, rate index)
    const float* tables;
    int copy;                                             // samples of a plan-rate row
    RateBankRate r[kRbMaxRates];
};
void launch_ratebank(const RateBankArgs& a, int n, hipStream_t st);

}  // namespace dn

// Comparison entry (dn_api_model.hip): the stand-alone fp32 forward on the conv tiles of before the live-row / lane-geometry change.  Not in the
// public header; nothing in the product calls it.
struct dn_model;
extern "C" int dn_cell_forward_parent_tiles(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out, int32_t B, int32_t T,
                                            int32_t F, int32_t C, void* stream);
