// dn_hop_kernels.hpp -- the whole hop as ONE launch (app3.py:178-226 for B streams), in two schedules:
//
// frame_kernel   nothing overlapped: one workgroup per stream runs P1-P12 back to back (dn_process_frame, dn_stream_step).
//
// hop_kernel     software-pipelined: ONE launch per hop that overlaps hop n's Griffin-Lim with hop n+1's analysis + model +
//                inverse mel (consecutive loop iterations of app3.py:178 overlapped; dn_pipe_*).
//   Consecutive hops depend on each other only through hx (the model); hop n's Griffin-Lim (~3/4 of a hop, a
//   strictly serial chain per stream that occupies three wavefronts of a CU) does not depend on hop n+1's
//   front half.  A launch therefore carries two kinds of workgroups:
//     blocks [0, back_B)           Griffin-Lim of the PENDING hop, reading scratch slot (frames-1) & 1
//     blocks [back_B, back_B + B)  P1-P10 of THIS hop (stft -> GRUUNet2 -> inverse mel, one stream per workgroup,
//                                  stages separated by workgroup barriers), writing scratch slot frames & 1
//   Both kinds are resident together (192 threads, <= 35 KB LDS: a Griffin-Lim and a front workgroup share a CU),
//   so the front half fills issue slots and the fourth SIMD the latency-bound Griffin-Lim leaves idle.  Everything is on
//   the caller's stream: launch k+1 is ordered behind launch k, which is all the synchronisation the slot hand-over
//   needs -- no events, no second stream (a two-stream/event version lost ~13 us per hop to cross-queue signalling).
//   What changes from hop to hop -- the slot parity, the Griffin-Lim seed, whether a hop is pending, the ring priming
//   of a new stream -- lives in a device-resident control block (PipeCtl) that the last workgroup of every launch
//   advances, so one captured launch replays indefinitely under hipGraph (BASELINE config 5).
#pragma once
#include "dn_dispatch.hpp"
#include "dn_hop_common.hpp"

// The kernels below are instantiated in FOUR translation units, because LLVM's GCN scheduling strategies suit them differently (Makefile; measured,
// profiles/r04_group_sweep.txt):
//   dn_hop.hip      n_fft 1024, a wavefront per STFT column (the one-hop pipe, the unpipelined hop): max-ILP, +2..3 %;
//   dn_hop_glw.hip  n_fft 1024, a wavefront per stream (deep pipes, the saturated regime, the front-only launch of a split hop):
//                   iterative-ILP, +3..7 % (1,024 streams 6.73 -> 7.00 M frames/s, the captured streaming step 6.34 -> 6.79 M);
//   dn_hop1536.hip  n_fft 1536: the default strategy (max-ILP costs it 12 %: it sits at the 256-register cap and spills more);
//   dn_hop512.hip   n_fft 512, a wavefront per STFT column: the default strategy (no strategy has been measured against it yet).
// Each unit defines the launchers declared here for its size or schedule, by instantiating launch_hop_of / launch_frame_of below.
// The stamped diagnostic build keeps everything in dn_hop.hip (its probe arrays are per translation unit): there the side units are empty.

namespace dn {

void launch_hop_unit(Size<1024>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);          // (dn_hop.hip: a.glw -> launch_hop_glw)
void launch_hop_unit(Size<1536>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);          // (dn_hop1536.hip)
void launch_hop_unit(Size<512>, const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);           // (dn_hop512.hip)
void launch_hop_glw(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st);                       // (dn_hop_glw.hip)
void launch_frame_unit(Size<1024>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st);
void launch_frame_unit(Size<1536>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st);
void launch_frame_unit(Size<512>, const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st);

// n_fft 1536: the Griffin-Lim body would take 330 registers and shut the front workgroup out of the CU; capping the
// kernel at two waves per SIMD (256 registers, ~80 values spilled to scratch) keeps both halves resident (+30 % at 1024
// streams).  n_fft 1024 fits in 229 registers without a cap (capping it costs 8 %).
// The pipelined launch uses workgroups of FOUR wavefronts.  A Griffin-Lim workgroup needs three (one per column): its fourth exits at
// once.  A front workgroup uses all four: its waves share SIMDs with the Griffin-Lim waves of the same CU (six or seven waves on four
// SIMDs) and its phases end at workgroup barriers, so the front half -- not the Griffin-Lim chain -- was what ended a batch-256 launch
// (measured: two iterations moved INTO the front workgroup cost 4.8 us); a fourth wave shortens every conv phase by a quarter.
#ifdef DN_PROBE
// diagnostic build only: when the two kinds of workgroups of one launch start and finish (workgroups 0 and back_B of the last launch)
static __device__ unsigned long long g_hop_wg_probe[8];
static __device__ unsigned long long g_hop_blk_t[2048][2];   // start / end of every workgroup of the last launch (s_memtime)
static __device__ unsigned int g_hop_blk_hw[2048];          // where every workgroup of the last launch ran: HW_ID | XCC_ID << 28 (tools/glw_probe.py census)
#define DN_HSTAMP(id) do { if (tid == 0 && (blockIdx.x == 0 || (int)blockIdx.x == a.back_blocks)) { unsigned long long t_; \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); g_hop_wg_probe[id] = t_; } } while (0)
#else
#define DN_HSTAMP(id) do { } while (0)
#endif

// CT: the number of compressed mel bins when the plan has the usual one (80 mels at n_fft 1024, 64 at 512 and 1536), 0 = any (run-time lengths in the model)
// GLW: the pending hops' Griffin-Lim runs one wavefront per stream and chain segment (dn_glw_body.hpp) instead of one wavefront per column (one
//      stream a workgroup, one pending hop).  A workgroup then holds a.spb streams x a.depth chain segments (spb x depth <= 4):
//        depth 1  four streams a workgroup: the saturated regime (several streams per CU);
//        depth D  a stream's chain is cut into D segments that run in D consecutive launches, so D hops of the SAME stream are in flight
//                 (wave j of the workgroup advances frame frames-1-j by its next segment and parks it in HBM, the last segment emits): with
//                 about one stream per CU this is what fills the CU -- throughput of the saturated regime at batch 256 for D - 1 more
//                 hops of latency.
//      Capped at two waves per SIMD.
// FRONT: a launch of front workgroups only, the second of the TWO launches of a split hop (a.front_only; the first is this kernel's
//      ordinary form with front_B = 0: the chains).  Where a launch carries many more workgroups than the chip holds at once, its Griffin-Lim
//      workgroups (the low block ids) run first and its front workgroups after them anyway -- two phases, not a mix -- and a front workgroup
//      compiled beside the chain inherits the chain's 243 registers: two workgroups a CU.  On its own the front half is capped at
//      kFrontPerCu workgroups a CU (its phases end at workgroup barriers and wait on memory: more of them in flight is what it wants).
// PHIN: an input-phase pipe (a.phase_in; DN_PHASE_FROM_INPUT): the front half stores the unit phasors of its STFT in the slot's init area and marks the
//      frame as carrying its phases; nothing is drawn, by the spare wave or by the chain.  A template parameter: the default instantiation is unchanged.
//      The head start reads the slot back in the same workgroup: wave w / lane l loads the bins wave w / lane l stored (stft_body; every n_fft), so
//      program order covers it, with workgroup barriers between besides.  Every other reader (the chains of a later launch) is behind a kernel boundary.
template <int NFFT, bool STREAM, bool BF16, int CT, bool GLW, bool FRONT = false, bool PHIN = false>
__global__ __launch_bounds__(kHopPipeThreads, FRONT ? kFrontPerCu : (NFFT == 1536 || GLW) ? 2 : 1) void hop_kernel(DspDev d, CellDev cd, HopArgs a) {
    constexpr int kNR = NFFT, kBins = Geo<NFFT>::kBins;
    __shared__ __attribute__((aligned(16))) char smem[FRONT ? front_smem<NFFT>() : hop_smem<NFFT>()];
    const int tid = threadIdx.x;
    // control block as the previous launch left it (uniform: scalar loads)
    const unsigned long long pushes = a.ctl->pushes, frames = a.ctl->frames, launches = a.ctl->launches;
    const unsigned int pending = a.ctl->pending, slot_next = a.ctl->slot_next;
    const SlotLayout sl(a.B, d.n_mels, kBins);
    const bool priming = STREAM && pushes < (unsigned long long)a.prime;
#ifdef DN_PROBE
    if (tid == 0 && blockIdx.x < 2048) {
        unsigned int hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_hop_blk_hw[blockIdx.x] = (hw & 0x0fffffffu) | (xcc << 28);
        unsigned long long t_;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
        g_hop_blk_t[blockIdx.x][0] = t_;
    }
#endif
    // the oldest frame in flight completes in this launch when this is its last segment (wavefront per column: depth 1, always)
    const int depth = GLW ? a.depth : 1;
    const bool completes = !FRONT && pending > 0 && launches - a.ctl->front_launch[(frames - pending) & 7] == (unsigned long long)depth;
    if (!FRONT && GLW && (int)blockIdx.x < a.back_blocks) {
        if constexpr (GLW && !FRONT) {
            const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int sidx = wv / depth, j = wv - sidx * depth;          // stream of the workgroup, frames behind the newest (uniform)
            const size_t b = (size_t)blockIdx.x * a.spb + sidx;
            DN_WSTAMP(0);
            // the workgroup's window tables: every wave fills its share and meets the others at ONE LDS-only barrier -- a wave that runs a chain
            // does both inside glw_body, behind the loads of its own prologue; the others here
            const bool runs = pending && sidx < a.spb && b < (size_t)a.back_B && j < (int)pending;
            if (pending && !runs) {
                glw_fill_tables<NFFT, kHopPipeThreads>(smem, d, tid);
                DN_LDS_BARRIER();
            }
            DN_WSTAMP(1);
            if (sidx < a.spb && b < (size_t)a.back_B) {          // (a wave without work skips to the ticket: wave 0 always has a stream)
                if (j < (int)pending) {
                    const unsigned long long g = frames - 1 - j;                                          // the frame
                    const int seg = (int)(launches - a.ctl->front_launch[g & 7]) - 1;                     // its next segment: 0 .. depth-1
                    const int s = slot_behind(slot_next, 1 + j, a.n_slots);
                    const float* slot = a.slots + (size_t)s * a.slot_stride;
                    const uint32_t* meta = reinterpret_cast<const uint32_t*>(slot + sl.meta) + kSlotMeta * b;
                    const v2f* init = FrameMeta::load_has_init(meta) ? reinterpret_cast<const v2f*>(a.slot_init + (size_t)s * a.init_stride) : nullptr;
                    const uint64_t seed = FrameMeta::load_seed(meta), sid0 = FrameMeta::load_sid0(meta);
                    const int it0 = FrameMeta::load_it0(meta), n_iter = FrameMeta::load_n_iter(meta);
                    const float mom = FrameMeta::load_mom(meta);
                    float* gl_out = FrameMeta::load_out(meta);
                    // iterations [lo, hi) of the frame's chain; the last segment runs to the end and emits.  (A frame of a deep pipe comes with its
                    // initial phases in the slot -- injected, or drawn by its front workgroup's spare wave -- so every segment starts alike.)
                    const int span = n_iter > it0 ? n_iter - it0 : 0;
                    auto cut = [&](int k) { return k <= 0 ? 0 : k >= depth ? span : (span * k + depth / 2) / depth; };
                    const int lo = it0 + cut(seg), hi = it0 + cut(seg + 1);
                    const bool last = seg == depth - 1;
#ifdef DN_GLW_PRIO
                    __builtin_amdgcn_s_setprio(DN_GLW_PRIO);
#endif
                    glw_body<NFFT, STREAM>(smem, d, slot + sl.lin, init, seed, sid0, slot + sl.peak, STREAM ? nullptr : gl_out, n_iter, mom, b, lane, wv,
                                           a.ola, a.hop_out, a.out_s16, lo, last ? -1 : hi, seg > 0 ? kGlwFromSeg : it0 > 0 ? kGlwFromX : kGlwFresh,
                                           reinterpret_cast<v2f*>(a.gl_state + (size_t)s * a.state_stride), tid);
                    DN_WSTAMP(7);
                }
                if (STREAM && j == 0 && !completes) pcm_zero_hop(a.hop_out, a.out_s16, b, kNR / 2, lane, 64);   // nothing to emit in this launch
            }
        }
    } else if (!FRONT && (int)blockIdx.x < a.back_blocks) {
      if constexpr (!FRONT) {
        const size_t b = blockIdx.x;
        if (tid >= kHopThreads) return;         // (before any barrier: a terminated wave no longer counts at s_barrier)
        DN_HSTAMP(0);
        if (pending) {
            // the Griffin-Lim chain is the critical path of the launch: let its waves win issue arbitration against the
            // front-half waves they share SIMDs with
            __builtin_amdgcn_s_setprio(DN_GL_PRIO);
            const int s = slot_behind(slot_next, 1, a.n_slots);
            const float* slot = a.slots + (size_t)s * a.slot_stride;
            // the frame's own n_iter / momentum (those of its submit, not of this call: it0 <= n_iter by construction) and destination
            const uint32_t* meta = reinterpret_cast<const uint32_t*>(slot + sl.meta) + kSlotMeta * b;
            const v2f* init = FrameMeta::load_has_init(meta) ? reinterpret_cast<const v2f*>(a.slot_init + (size_t)s * a.init_stride) : nullptr;
            const uint64_t seed = FrameMeta::load_seed(meta), sid0 = FrameMeta::load_sid0(meta);
            const int it0 = FrameMeta::load_it0(meta), n_iter = FrameMeta::load_n_iter(meta);
            const float mom = FrameMeta::load_mom(meta);
            v2f* st = reinterpret_cast<v2f*>(a.gl_state + (size_t)s * a.state_stride);
            if (!STREAM) {
                float* gl_out = FrameMeta::load_out(meta);
                gl_body<NFFT, false, false>(smem, d, slot + sl.lin, nullptr, init, seed, sid0, slot + sl.peak, gl_out, n_iter, mom, b, tid,
                                            nullptr, nullptr, 0, it0, -1, st);
            } else
                gl_body<NFFT, false, true>(smem, d, slot + sl.lin, nullptr, init, seed, sid0, slot + sl.peak, nullptr, n_iter, mom, b, tid,
                                           a.ola, a.hop_out, a.out_s16, it0, -1, st);
            __builtin_amdgcn_s_setprio(0);
            DN_HSTAMP(1);
        } else if (STREAM) {
            // nothing to emit yet: pcm_zero_hop(a.hop_out, a.out_s16, b, kNR / 2, tid, kHopThreads), spelled out (three waves are left) -- through the
            // helper ten of this branch's kernels get their blocks laid out in another order
            for (int n = tid; n < kNR / 2; n += kHopThreads) {
                if (a.out_s16) static_cast<short*>(a.hop_out)[b * (kNR / 2) + n] = 0;
                else static_cast<float*>(a.hop_out)[b * (kNR / 2) + n] = 0.0f;
            }
        }
      }
    } else {
        const size_t b = blockIdx.x - (FRONT ? 0 : a.back_blocks);
        DN_HSTAMP(2);
        const float* frames_in = a.frames;
        if (STREAM) {
            if (__builtin_expect(a.host_copy_src != nullptr, 0)) {
                // deferred host output: the hop the PREVIOUS push emitted for this stream, device staging buffer -> its page-locked host buffer.
                // The front workgroups of a launch start all through it, so the posted stores drain while the hop computes instead of ending the
                // previous launch as one PCIe burst; the last workgroup's system-scope fence below covers them.  (Here and not at the head of the
                // kernel: there the same lines cost the chain waves of EVERY streaming launch 2 % -- 155.8 -> 159.2 us at 1,024 streams.)
                const unsigned int per = a.host_copy_n16 / (unsigned int)a.B;          // 16-byte units of one stream's hop
                for (unsigned int i = tid; i < per; i += kHopPipeThreads) a.host_copy_dst[b * per + i] = a.host_copy_src[b * per + i];
            }
            ring_shift<NFFT, kHopPipeThreads>(a.ring, a.hop_in, a.in_s16, b, tid);
            frames_in = a.ring;
        }
        if (!priming) {
            const int s = (int)slot_next;
            float* slot = a.slots + (size_t)s * a.slot_stride;
            float2* slot_init = a.slot_init + (size_t)s * a.init_stride;
            stft_body<NFFT, false, true, kHopPipeThreads, PHIN>(smem, d, frames_in, nullptr, slot, slot + sl.peak, DN_PEAK_NORMALIZE | DN_PRE_WINDOW, b, tid,
                                                                slot_init);   // P1-P6
            const int split = FRONT ? 0 : min(a.gl_split, a.n_iter);        // (a split hop has no head start)
            // (measured: n_fft 1536, 13 bins a lane: 106 -> 100 us per batch-256 hop; n_fft 1024, 9 bins a lane: 54.7 -> 55.2 us -- the draw's 12 KB
            // a stream through HBM cost more than the multiplies it moved off the chain, so only the long transform uses it)
            // A deep pipe (a.depth > 1: the chain runs as segments, one wavefront per stream) draws here too, at either transform length: there the
            // draw is 27 Philox blocks a lane (~12 k cycles) on the first segment's wave, which then has to get an iteration less than the others.
            const bool draw = !PHIN && a.init_in == nullptr && (NFFT == 1536 ? split > 0 : a.depth > 1);
            if (draw && tid >= kHopThreads) {
                // The fourth wave has no column to transform and would wait here: it draws the random initial phases the head start
                // below begins with (the same Philox blocks, so the same bits) into the slot.  A block is ten rounds of quarter-rate integer
                // multiplies and serves one bin pair -- drawn by the head start itself they were ~7 k cycles on the launch's critical path.
                float2* dst = slot_init + b * 3 * kBins;
                constexpr int kPairs = (kBins - 1) / 2 + 1;                 // one block per bin pair (m, NC - m), m = 0..NC/2
                for (int i = tid - kHopThreads; i < 3 * kPairs; i += 64) {
                    const int col = i / kPairs, m = i - col * kPairs;
                    v2f lo, hi;
                    rand_angle_pair(a.seed + frames, a.sid0 + b, col, m, lo, hi);
                    dst[col * kBins + m] = make_float2(lo[0], lo[1]);
                    if (2 * m != kBins - 1) dst[col * kBins + kBins - 1 - m] = make_float2(hi[0], hi[1]);
                }
            }
            __syncthreads();
            DN_HSTAMP(5);
            cell_body<kHopPipeThreads / 64, BF16, CT, FRONT ? false : kCellStageDefault>(smem, cd, slot, a.hx, slot + sl.diff, a.hx, 3, a.C, b, tid);   // P7
            __syncthreads();
            DN_HSTAMP(6);
            invmel_body<NFFT, true, kHopPipeThreads>(smem, d, slot, slot + sl.diff, slot + sl.lin, 3 * a.B, b * 3, tid);                  // P8-P10
            // what this frame's Griffin-Lim (next launch) needs besides the magnitudes: its seed, its stream ids and, in parity mode, its phases
            DN_HSTAMP(3);                          // front half (P1-P10) done
            if (tid == 0) {
                uint32_t* meta = reinterpret_cast<uint32_t*>(slot + sl.meta) + kSlotMeta * b;
                const uint64_t seed = a.seed + frames;
                const bool in_slot = PHIN || a.init_in != nullptr || (draw && a.depth > 1);       // the frame's phases are in the slot
                FrameMeta{in_slot, seed, a.sid0, split, a.n_iter, a.mom, a.gl_out}.store(meta);
            }
            if (!PHIN && a.init_in != nullptr) {
                const float2* src = reinterpret_cast<const float2*>(a.init_in) + b * 3 * kBins;
                float2* dst = slot_init + b * 3 * kBins;
                for (int i = tid; i < 3 * kBins; i += kHopPipeThreads) dst[i] = src[i];
            }
            if constexpr (!FRONT) if (split > 0) {
                // head start: this workgroup would idle for the rest of the launch (the pending hop's chain is ~1.5x longer than P1-P10)
                __syncthreads();                       // the magnitudes are in the slot
                if (tid >= kHopThreads) return;        // the chain is three waves wide
                __builtin_amdgcn_s_setprio(DN_HS_PRIO); // below the pending hop's chain (3): that one ends the launch
                gl_body<NFFT, false, false, NFFT == 1536>(smem, d, slot + sl.lin, nullptr,
                                            (PHIN || draw) ? reinterpret_cast<const v2f*>(slot_init) : reinterpret_cast<const v2f*>(a.init_in), a.seed + frames, a.sid0,
                                            nullptr, nullptr, a.n_iter, a.mom, b, tid, nullptr, nullptr, 0, 0, split,
                                            reinterpret_cast<v2f*>(a.gl_state + (size_t)s * a.state_stride));
                __builtin_amdgcn_s_setprio(0);
                DN_HSTAMP(4);                      // head start done
            }
        }
    }
    // ---- ticket: the last workgroup of the launch advances the control block (every workgroup has read it by then)
    // Zero-copy host transport: the completion word the last workgroup publishes must not overtake ANY workgroup's samples.  A workgroup barrier
    // orders LDS and (in this wave-sharing mode) does not have to wait for outstanding stores: every wave therefore waits until its own stores are
    // ACKNOWLEDGED (s_waitcnt vmcnt(0)) before the barrier that precedes its workgroup's ticket.  The samples go to page-locked host memory, which
    // the L2s do not cache: an acknowledged store has left the chip's caches for the fabric, and the completion word -- written by the last
    // workgroup after it has seen every ticket, behind a system-scope fence -- follows them through the same PCIe port, where posted writes of one
    // device stay in order.  The strict form of the memory model -- the ticket as a release / acquire pair at SYSTEM scope -- is kept behind
    // DN_HOST_STRICT_RELEASE: it writes an XCD's whole L2 back once per workgroup (the slots of the pipe are in there) and measured 10-14 % of the
    // host-fed rate (256 streams 59.5 -> 68.0 us per hop, 1,024 streams 163.6 -> 186.5: profiles/r04_v4_side_measurements.jsonl) for stores that
    // are not in the L2 in the first place.
    if (a.host_done != nullptr) DN_WAIT_VMEM();
    __syncthreads();
#ifdef DN_PROBE
    if (tid == 0 && blockIdx.x < 2048) {
        unsigned long long t_;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");
        g_hop_blk_t[blockIdx.x][1] = t_;
    }
#endif
    if (tid == 0) {
#ifdef DN_HOST_STRICT_RELEASE
        const unsigned int t = a.host_done != nullptr ? __hip_atomic_fetch_add(&a.ctl->done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM)
                                                      : atomicAdd(&a.ctl->done, 1u);
#else
        const unsigned int t = atomicAdd(&a.ctl->done, 1u);
#endif
        if (t == gridDim.x - 1) {
            a.ctl->done = 0;
            if (!FRONT) a.ctl->launches = launches + 1;     // (the chains' launch of a split hop has counted it: this one is launch `launches - 1` still)
            const bool fronted = a.front_B > 0 && !priming;
            if (a.front_B > 0) a.ctl->pushes = pushes + 1;
            if (fronted) {
                a.ctl->front_launch[frames & 7] = FRONT ? launches - 1 : launches;
                a.ctl->frames = frames + 1;
                a.ctl->slot_next = (int)slot_next + 1 == a.n_slots ? 0u : slot_next + 1;
            }
            a.ctl->pending = pending - (completes ? 1u : 0u) + (fronted ? 1u : 0u);
            if (a.host_done != nullptr) {
                __threadfence_system();
                __hip_atomic_store(a.host_done, a.host_done_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// One pipelined launch at size NFFT in the schedule GLW.  a.front_only (GLW units): the second launch of a split hop, front workgroups alone under
// their own register budget.  PHIN only with front workgroups: a launch without them -- a flush, the chains' launch of a split hop -- runs no
// analysis and takes the default instantiation.
template <int NFFT, bool GLW>
static void launch_hop_of(const DspDev& d, const CellDev& c, const HopArgs& a, bool bf16, hipStream_t st) {
    with_bool(a.ola != nullptr, a.phase_in && a.front_B > 0, [&](auto stream, auto phin) {
        with_bool_if<GLW>(a.front_only, [&](auto front) {
            with_model<NFFT>(bf16, a.C, [&](auto bf, auto ct) {
                constexpr bool kFront = decltype(front)::value;
                hipLaunchKernelGGL((hop_kernel<NFFT, decltype(stream)::value, decltype(bf)::value, decltype(ct)::value, GLW, kFront, decltype(phin)::value>),
                                   dim3(kFront ? a.front_B : a.back_blocks + a.front_B), dim3(kHopPipeThreads), 0, st, d, c, a);
            });
        });
    });
}

// ---- the unpipelined hop: P1-P12 of one stream in one workgroup, one launch per hop (zero added latency).  Four wavefronts for the
// front half (the conv phases split four ways), three for the Griffin-Lim chain behind it (the fourth exits).
// PHIN (DN_PHASE_FROM_INPUT; a.phas != null): the analysis also stores the unit phasors of its STFT in the workspace and the chain starts from them.
// A template parameter, so the default instantiation is the kernel it was.  Wave w / lane l of the chain loads the bins wave w / lane l of the
// analysis stored (stft_body; n_fft 512, 1024 and 1536 alike), so program order covers the hand-over -- and two workgroup barriers lie between.
template <int NFFT, bool STREAM, bool BF16, int CT, bool PHIN = false>
__global__ __launch_bounds__(kHopPipeThreads, NFFT == 1536 ? 2 : 1) void frame_kernel(DspDev d, CellDev cd, FrameArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[hop_smem<NFFT>()];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float* frames_in = a.frames;
    if (STREAM) {
        ring_shift<NFFT, kHopPipeThreads>(a.ring, a.hop_in, 0, b, tid);
        frames_in = a.ring;
    }
    stft_body<NFFT, false, true, kHopPipeThreads, PHIN>(smem, d, frames_in, nullptr, a.mel, a.peak, DN_PEAK_NORMALIZE | DN_PRE_WINDOW, b, tid,
                                                        reinterpret_cast<float2*>(a.phas));   // P1-P6
    __syncthreads();
    cell_body<kHopPipeThreads / 64, BF16, CT, kCellStageDefault, DN_FRAME_TILES>(smem, cd, a.mel, a.hx, a.diff, a.hx, 3, a.C, b, tid);     // P7
    __syncthreads();
    if (tid >= kHopThreads) return;
    const v2f* init = reinterpret_cast<const v2f*>(PHIN ? a.phas : a.init);
    // P8-P12: the inverse-mel contraction is the Griffin-Lim prologue (the linear magnitudes stay in LDS)
    if (!STREAM)
        gl_body<NFFT, true, false>(smem, d, a.mel, a.diff, init, a.seed, a.sid0, a.peak, a.out, a.n_iter, a.mom, b, tid);
    else
        gl_body<NFFT, true, true>(smem, d, a.mel, a.diff, init, a.seed, a.sid0, a.peak, nullptr, a.n_iter, a.mom, b, tid,
                                  a.ola, a.hop_out, 0);
}

template <int NFFT>
static void launch_frame_of(const DspDev& d, const CellDev& c, const FrameArgs& a, int B, bool bf16, hipStream_t st) {
    with_bool(a.ring != nullptr, a.phas != nullptr, [&](auto stream, auto phin) {
        with_model<NFFT>(bf16, a.C, [&](auto bf, auto ct) {
            hipLaunchKernelGGL((frame_kernel<NFFT, decltype(stream)::value, decltype(bf)::value, decltype(ct)::value, decltype(phin)::value>),
                               dim3(B), dim3(kHopPipeThreads), 0, st, d, c, a);
        });
    });
}

}  // namespace dn
