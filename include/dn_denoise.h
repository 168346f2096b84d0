/*
 * dn_denoise.h -- C ABI of the MI355X-native per-hop speech-denoising path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.
 * Every buffer argument marked [dev] is a DEVICE pointer owned by the caller
 * (e.g. torch.Tensor.data_ptr() of a contiguous fp32 tensor on the GPU); the
 * library never frees or retains it beyond the call.  Arguments marked
 * [host] are host pointers read during the call only.  All kernels are
 * enqueued on the HIP stream passed in (`stream`, a hipStream_t cast to
 * void*; NULL = the null stream); no call synchronises the device.
 * Handles are immutable after creation and may be shared by threads.
 *
 * Reference interfaces replaced (file:line in belacks/audio-denoising):
 *   dn_model_create / dn_cell_forward   gruunet2.py:246-306  GRUUNet2.__init__/forward
 *                                       (called at app3.py:112-116, 200-201; server.py:151,212)
 *   dn_momo_create / dn_momo_forward    momo3.py:247-324     MOMO3.__init__/forward (sibling model)
 *   dn_dsp_create                       app3.py:135-155  construction of the torchaudio
 *                                       Spectrogram/MelScale/InverseMelScale/GriffinLim + Hann window
 *   dn_stft                             app3.py:191      Spectrogram(power=None)(x)
 *   dn_stft_phasors                     server.py:208    spec.angle() of the noisy input, as unit phasors (DN_PHASE_FROM_INPUT)
 *   dn_stft_mel_log1p                   app3.py:179-195  peak-normalise, Hann, STFT, |.|, MelScale, log1p, transpose
 *   dn_mel_scale                        app3.py:193      MelScale(mag)
 *   dn_invmel / dn_residual_invmel      app3.py:203-211  leaky_relu(in-out), expm1, clamp, InverseMelScale, clamp
 *   dn_griffinlim                       app3.py:213-217  GriffinLim(power=1)(lin) (* peak)
 *   dn_synthesis                        app3.py:203-217  residual .. InverseMelScale .. GriffinLim (* peak), one launch
 *   dn_istft                            server.py:174,216 InverseSpectrogram
 *   dn_stft_general / dn_server_rows / dn_istft_general / dn_cell_forward_ex   server.py:199-217  the socket server's variant
 *   dn_process_frame                    app3.py:178-217  the whole per-hop loop body for B streams
 *   dn_stream_step                      app3.py:178-226  the same plus ring buffer / overlap-add state (P12)
 *   dn_clip_process                     app3.py:178-226  N consecutive dn_stream_step calls in one: audio that is already there
 *   dn_clip_process_ragged              app3.py:178-226  the same for clips of different lengths: n_hops[b] hops of stream b
 *   dn_sessions_*                       app3.py:123-250  one DenoisingAudioProcessor per session: slots that join, leave
 *                                       and push hops on their own, batched per tick; sessions exported to and
 *                                       imported from self-contained records (move, resume, resize a pool)
 *   dn_resample_*                       utils.py:48-49, app.py:181  torchaudio Resample / librosa.resample: audio at another
 *                                       rate than the plan's, whole signals and streams
 *   dn_pipe_*                           app3.py:167-250  the same hop, consecutive hops software-pipelined in one launch per hop
 *                                       (dn_pipe_stream_*: the steady-state recv loop with its per-stream buffers)
 *
 * Memory layouts (row-major, fp32; "complex" = interleaved re,im float pairs):
 *   frames      [B][n_fft]
 *   spec        [B][T][K] complex      K = n_fft/2+1, T = 3 columns per frame.  The reference's
 *                                      (B,K,T) tensors are the transpose(-1,-2) VIEW of this buffer.
 *   mel / x     [B][T][M]              exactly the (B,T,F) tensor GRUUNet2.forward takes
 *   hx          [B][17][C]             C = M/16
 *   mag         [B][T][K]
 *   wave        [B][n_fft]
 *
 * Return value: 0 on success, negative dn_status on failure; the message of
 * the last failure on the calling thread is returned by dn_last_error().
 */
#ifndef DN_DENOISE_H
#define DN_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DN_ABI_VERSION 9

typedef enum dn_status {
    DN_OK = 0,
    DN_ERR_INVALID = -1,      /* bad argument / shape mismatch */
    DN_ERR_UNSUPPORTED = -2,  /* configuration outside what the kernels are built for */
    DN_ERR_HIP = -3,          /* HIP runtime failure (message has hipGetErrorString) */
    DN_ERR_NOMEM = -4
} dn_status;

typedef struct dn_model dn_model; /* GRUUNet2 weights, packed and resident on one device */
typedef struct dn_dsp dn_dsp;     /* STFT/mel/inverse-mel/Griffin-Lim plan, resident on one device */

/* Constructor arguments of gruunet2.GRUUNet2 (gruunet2.py:248-255).  The kernels are built for
 * the architecture of every GRUUNet2 checkpoint in the reference: 4 levels, hidden 17, k3 s2 p1,
 * 6 gaussians; anything else returns DN_ERR_UNSUPPORTED. */
typedef struct dn_model_cfg {
    int32_t num_compressed_bins; /* C; default hx is zeros(B,17,C) */
    int32_t in_size;             /* must be 1 (gruunet2.py:257) */
    int32_t n_levels;            /* 4 */
    int32_t hidden_size;         /* 17 (all levels equal) */
    int32_t kernel_size;         /* 3 */
    int32_t stride;              /* 2 */
    int32_t padding;             /* 1 */
    int32_t num_gaussians;       /* 6 */
} dn_model_cfg;

#define DN_MODEL_N_FLOATS 15337  /* state_dict order, SURVEY.md Appendix A.4 */

/* weights [host]: the reference state_dict flattened in its own key order (15,337 fp32).
 * The handle lives on the current HIP device. */
int dn_model_create(const float* weights, size_t n_floats, const dn_model_cfg* cfg, dn_model** out);
void dn_model_destroy(dn_model* m);

/* GRUUNet2.forward for B independent streams, T sequential steps.
 *   x [dev][B][T][F], hx_in [dev][B][17][C] (NULL = zeros), out [dev][B][T][F], hx_out [dev][B][17][C].
 * F must equal 16*C (else DN_ERR_INVALID, mirroring the reference's shape error).  hx_in is not
 * modified (gruunet2.py:240 builds a new tensor); hx_out may alias hx_in. */
int dn_cell_forward(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out,
                    int32_t B, int32_t T, int32_t F, int32_t C, void* stream);

/* dn_cell_forward with the returned state scaled: hx_out = hx' * hx_out_scale (the `hx = hx * 0.9` of server.py:214). */
int dn_cell_forward_ex(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out,
                       int32_t B, int32_t T, int32_t F, int32_t C, float hx_out_scale, void* stream);

/* BASELINE config 3: the same forward with bf16 MFMA conv tiles (v_mfma_f32_16x16x32_bf16): encoder / decoder conv
 * inputs and weights are rounded to bf16 (round to nearest even), accumulation, biases, the recurrent gate conv, the
 * GRU math and the last decoder level stay fp32.  Not bit-compatible with the fp32 reference: tolerance is restated
 * (tests/test_gpu_parity.py: <= 1e-2 relative RMS, <= 5e-1 max-abs on the mel residual; measured 4e-3 / 0.07-0.31). */
int dn_cell_forward_bf16(const dn_model* m, const float* x, const float* hx_in, float* out, float* hx_out,
                         int32_t B, int32_t T, int32_t F, int32_t C, void* stream);

/* ---- Sibling model MOMO3 (momo3.py:247-324; checkpoint saves/MOMO3-4d4ea0) on the same fp32 MFMA conv tiles -------------
 * Differences from GRUUNet2: a second input channel, the frame delta x_t - prev (momo3.py:285-289); the position code
 * enters only at the encoder input and at the hidden-gate conv (momo3.py:138-145); 3 levels, hidden 16, per-level
 * paddings (1, 0, 1) -- 22 input bins compress to 3.  The kernels are built for that architecture (paddings 0 or 1, up to
 * 64 input bins); anything else returns DN_ERR_UNSUPPORTED. */
typedef struct dn_momo dn_momo;
typedef struct dn_momo_cfg {
    int32_t num_compressed_bins; /* default hx is zeros(B,16,num_compressed_bins) */
    int32_t in_size;             /* 1 (the delta channel is added internally, momo3.py:260) */
    int32_t n_levels;            /* 3 */
    int32_t hidden_size;         /* 16 */
    int32_t kernel_size;         /* 3 */
    int32_t stride;              /* 2 */
    int32_t paddings[3];         /* (1, 0, 1) in the checkpoint */
    int32_t num_gaussians;       /* 6 */
} dn_momo_cfg;
#define DN_MOMO3_N_FLOATS 9197   /* state_dict order of momo3.MOMO3 */
int dn_momo_create(const float* weights, size_t n_floats, const dn_momo_cfg* cfg, dn_momo** out);
void dn_momo_destroy(dn_momo* m);
/* MOMO3.forward for B streams, T sequential steps: x [dev][B][T][F], hx_in [dev][B][16][C] (NULL = zeros), prev_in [dev][B][F]
 * (the frame before x[:,0]; NULL = the first delta is zero, momo3.py:277-278), out [dev][B][T][F], hx_out [dev][B][16][C],
 * prev_out [dev][B][F] or NULL (the last frame: what the caller passes as prev_in to continue the sequence).  C must be what F
 * compresses to under the model's paddings (else DN_ERR_INVALID, mirroring the reference's broadcast error). */
int dn_momo_forward(const dn_momo* m, const float* x, const float* hx_in, const float* prev_in, float* out, float* hx_out,
                    float* prev_out, int32_t B, int32_t T, int32_t F, int32_t C, void* stream);

typedef struct dn_dsp_cfg {
    int32_t sample_rate;
    int32_t n_fft;   /* 512, 1024 or 1536 (hop = n_fft/2, win_length = n_fft); any other size: DN_ERR_UNSUPPORTED.  512 runs the one-hop
                      * schedules only (unpipelined hop, pipe of depth 1, one-launch sessions, the general kernels): see the setters below */
    int32_t hop;
    int32_t n_mels;  /* 0 = no mel stages */
} dn_dsp_cfg;

/* fb [host][K][n_mels]: mel filterbank as MelScale.fb (NULL = HTK triangles computed natively, f_min 0,
 * f_max sr//2, norm None).  pinv [host][K][n_mels]: pseudo-inverse of fb^T used by the inverse-mel GEMM
 * (NULL = computed natively in double precision from fb; the plan then also keeps the operator in factors, fb and the
 * significant diagonals of (fb^T fb)^-1, and the kernels apply those when fb has at most two filters per bin -- the same
 * min-norm least-squares solution to fp32 rounding; an explicit pinv is always applied as the dense matrix).
 * window [host][n_fft] (NULL = periodic Hann). */
int dn_dsp_create(const dn_dsp_cfg* cfg, const float* fb, const float* pinv, const float* window, dn_dsp** out);
void dn_dsp_destroy(dn_dsp* d);
/* Copies of the plan's host-side tables, for inspection/tests: fb and pinv are [K][n_mels]. */
int dn_dsp_get_tables(const dn_dsp* d, float* fb, float* pinv, float* window);

/* flags for the analysis entry points */
#define DN_PEAK_NORMALIZE 1u /* P1: x /= max|x| when that is > 1e-6 (app3.py:181-186) */
#define DN_PRE_WINDOW 2u     /* P2: multiply by the window before the STFT windows again (app3.py:188) */

/* Spectrogram(power=None): frames [dev][B][n_fft] -> spec [dev][B][3][K] complex. */
int dn_stft(const dn_dsp* d, const float* frames, float* spec, int32_t B, uint32_t flags, void* stream);

/* P1,P2,P4,P5,P6 fused: frames -> mel [dev][B][3][M] = log1p(MelScale(|STFT|)), peak [dev][B]
 * (peak may be NULL; it is 1 where normalisation was skipped). */
int dn_stft_mel_log1p(const dn_dsp* d, const float* frames, float* mel, float* peak, int32_t B,
                      uint32_t flags, void* stream);

/* MelScale alone: mag [dev][B][T][K] -> mel [dev][B][T][M] (no log). */
int dn_mel_scale(const dn_dsp* d, const float* mag, float* mel, int32_t B, int32_t T, void* stream);

/* InverseMelScale: mel_mag [dev][B][T][M] -> lin [dev][B][T][K] = relu(pinv(fb^T) @ mel). */
int dn_invmel(const dn_dsp* d, const float* mel_mag, float* lin, int32_t B, int32_t T, void* stream);

/* P8,P9,P10 fused: lin = relu(pinv @ clamp(expm1(leaky_relu(x - diff, 0.2)), 0)).
 * x, diff [dev][B][T][M]; lin [dev][B][T][K]. */
int dn_residual_invmel(const dn_dsp* d, const float* x, const float* diff, float* lin, int32_t B, int32_t T,
                       void* stream);

/* GriffinLim(power=1, n_iter, momentum, length=None) on 3-column magnitudes.
 *   mag [dev][B][3][K]; init_angles [dev][B][3][K] complex or NULL; when NULL the initial phases are drawn
 *   on the device (real, imag ~ U[0,1) independently, as the reference's torch.rand(complex64)) from a
 *   counter-based generator keyed by (seed, stream_id0 + b, element), so results do not depend on how
 *   streams are sharded.  scale [dev][B] or NULL multiplies the output (the `* peak` of app3.py:217).
 *   wave [dev][B][n_fft]. */
int dn_griffinlim(const dn_dsp* d, const float* mag, const float* init_angles, uint64_t seed,
                  uint64_t stream_id0, const float* scale, float* wave, int32_t B, int32_t n_iter,
                  float momentum, void* stream);

/* The initial phases dn_griffinlim / dn_synthesis / the fused hops draw when init_angles is NULL, for streams stream_id0 .. stream_id0 + B - 1:
 * angles_out [dev][B][3][K] complex, real and imaginary part ~ U[0,1) independently (torchaudio's GriffinLim(rand_init=True) =
 * torch.rand(complex64), app3.py:149-153).  Generator: Philox4x32-10 (Salmon et al., SC'11), one block per bin PAIR (m, K-1-m), m = 0..(K-1)/2:
 * counter = (m, column, stream id lo, hi), key = (seed lo, hi); words 0, 1 of the block are bin m, words 2, 3 bin K-1-m (the self-paired
 * middle bin takes words 0, 1), top 24 bits each -- so the draw does not depend on how streams are batched or sharded.
 * Feeding the result back as init_angles reproduces the NULL launch bit for bit (and lets a CPU reference run with the same phases). */
int dn_griffinlim_draw_phases(const dn_dsp* d, uint64_t seed, uint64_t stream_id0, float* angles_out, int32_t B, void* stream);

/* P8..P12 in ONE launch (app3.py:203-217): x, diff [dev][B][3][M] (model input and model output) ->
 * leaky_relu(x - diff, 0.2), expm1, clamp, inverse mel, relu, Griffin-Lim, * scale.  The linear magnitudes
 * stay in LDS.  init_angles / seed / stream_id0 / scale as for dn_griffinlim. */
int dn_synthesis(const dn_dsp* d, const float* x, const float* diff, const float* init_angles, uint64_t seed,
                 uint64_t stream_id0, const float* scale, float* wave, int32_t B, int32_t n_iter, float momentum,
                 void* stream);

/* torch.istft(center=True, length=None) of 3 columns: spec [dev][B][3][K] complex -> wave [dev][B][n_fft]. */
int dn_istft(const dn_dsp* d, const float* spec, float* wave, int32_t B, void* stream);

/* ---- Arbitrary-length chunks: the request loop of the reference's socket server (server.py:199-217) ----
 * dn_stft_general: Spectrogram(power=None) of x [dev][B][L] (any L > n_fft/2) -> spec [dev][B][T][K] complex (may be NULL),
 *   and/or logmel [dev][B][T][M] = log1p(MelScale(|spec|)) (may be NULL); T = 1 + L / hop.          server.py:207-210
 * dn_server_rows: per (b,t) row: relu(model_out) * 3, exp(logmel - .) - 1, InverseMelScale, torch.polar(., angle(spec_in))
 *   -> spec_out [dev][rows][K] complex (may alias spec_in).                                         server.py:213-216
 * dn_istft_general: InverseSpectrogram (length=None), spec [dev][B][T][K], T >= 2 -> wave [dev][B][hop*(T-1)].  server.py:216 */
int dn_stft_general(const dn_dsp* d, const float* x, float* spec, float* logmel, int32_t B, int32_t L, void* stream);
int dn_server_rows(const dn_dsp* d, const float* logmel, const float* model_out, const float* spec_in, float* spec_out,
                   int32_t rows, void* stream);
int dn_istft_general(const dn_dsp* d, const float* spec, float* wave, int32_t B, int32_t T, void* stream);

/* ---- Griffin-Lim on any number of columns: phase reconstruction for the any-length path -----------------------
 * dn_griffinlim_general: mag [dev][B][T][K], T >= 3 -> wave [dev][B][hop*(T-1)], torchaudio's fast Griffin-Lim (n_iter iterations, momentum as
 * torchaudio's, then one istft; n_iter = 0 is istft(init * mag)).  init_angles [dev][B][T][K] complex, or NULL: column t of stream b draws the
 * Philox phases of (seed, stream_id0 + b, t) -- the numbering of dn_griffinlim, so with T = 3 both draw the same.  DN_GL_INIT_NORMALIZE: init_angles
 * holds an arbitrary spectrum (the noisy STFT, say) whose unit phasors are the initial phases, with the arithmetic of DN_PHASE_FROM_INPUT.
 * Two forms that give the same bits: WHOLE, one launch with every iteration on chip, for T <= dn_griffinlim_general_whole_max(d); STEPS, two
 * launches an iteration, for any T.  With neither force flag WHOLE runs when T fits.  `workspace`: dn_griffinlim_general_workspace_bytes(d, B, T)
 * bytes of the caller's (nonzero for every valid (B, T), 0 for a null plan or T < 3; WHOLE leaves it unused); the library allocates nothing and
 * nothing synchronises.  Every argument is checked before the first launch: null d / mag / wave / workspace, B < 0, n_iter < 0, T < 3 (reflect
 * padding needs hop*(T-1) > n_fft/2), momentum outside [0, 1), unknown flag bits, both force flags, DN_GL_INIT_NORMALIZE with NULL init_angles
 * (all DN_ERR_INVALID), DN_GLG_WHOLE with T above the maximum (DN_ERR_UNSUPPORTED); the outputs are then untouched.  B == 0 returns DN_OK. */
#define DN_GLG_WHOLE 2u            /* force; T > dn_griffinlim_general_whole_max(d): DN_ERR_UNSUPPORTED */
#define DN_GLG_STEPS 4u            /* force; both: DN_ERR_INVALID; neither: WHOLE when T fits */
#define DN_GL_INIT_NORMALIZE 16u
int32_t dn_griffinlim_general_whole_max(const dn_dsp* d);
size_t dn_griffinlim_general_workspace_bytes(const dn_dsp* d, int32_t B, int32_t T);
int dn_griffinlim_general(const dn_dsp* d, const float* mag, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                          float* wave, void* workspace, int32_t B, int32_t T, int32_t n_iter, float momentum, uint32_t flags,
                          void* stream);
/* The phases dn_griffinlim_general draws with init_angles == NULL: angles_out [dev][B][T][K] complex. */
int dn_griffinlim_draw_phases_general(const dn_dsp* d, uint64_t seed, uint64_t stream_id0, float* angles_out, int32_t B, int32_t T,
                                      void* stream);
/* The magnitude half of dn_server_rows: relu(pinv . (exp(logmel - 3 relu(model_out)) - 1)) -> mag_out [dev][rows][K] float. */
int dn_server_mag(const dn_dsp* d, const float* logmel, const float* model_out, float* mag_out, int32_t rows, void* stream);

/* flags of the fused entry points */
#define DN_CONV_BF16 1u /* BASELINE config 3: encoder/decoder convs on bf16 MFMA tiles (as dn_cell_forward_bf16); 0 = exact fp32 */

/* ---- Input-phase mode: the Griffin-Lim chain starts from the phases of the noisy input ----------------------
 * DN_PHASE_FROM_INPUT, a flag of every fused entry point (dn_process_frame, dn_stream_step, dn_clip_process per call; dn_pipe_create,
 * dn_pipe_stream_create and dn_sessions_create for the life of the pipe or pool).  Let X[c][k] be the 3-column analysis STFT the hop computes
 * anyway: the STFT of the peak-normalised, pre-windowed frame, whose magnitudes feed the mel.  With the flag the chain's initial phases are the unit
 * phasors u = X / |X| instead of the reference's random draw (app3.py:149-153,213), and everything else is as before:
 * out = GriffinLim(lin, init = u, n_iter, momentum) * peak, then the overlap-add; frame counters advance as before; `seed` and `stream_id0` are
 * ignored for the phases.  n_iter = 0 is istft(polar(lin, angle(X))) -- the reconstruction of the reference's socket server (server.py:208,216:
 * phase = spec.angle(); I0(torch.polar(O, phase))) inside the real-time hop; n_iter = k is Griffin-Lim warm-started from the input.
 * Arithmetic: u = (re * r, im * r) with ONE reciprocal square root r = rsq(fmaf(re, re, im * im)), the same instructions in every kernel, so every
 * entry point gives the same bits; a bin whose |X|^2 is below the smallest normal float (1.17549435e-38: |X| < ~1.1e-19, zero included) gets
 * u = (1, 0), which is torch.polar(m, angle(0)) = m.
 * The flag excludes init_angles: the per-call entry points return DN_ERR_INVALID for flag + non-NULL init_angles before anything is launched; a
 * pipe or pool created with the flag returns it for every later submit / push that passes init_angles.  Either way nothing is changed.
 * Off by default; without the flag every entry point computes what it did before. */
#define DN_PHASE_FROM_INPUT 8u

/* The phasors themselves: frames [dev][B][n_fft] -> phasors [dev][B][3][K] complex, the layout of init_angles.  flags as for dn_stft
 * (DN_PEAK_NORMALIZE | DN_PRE_WINDOW is what the fused hops apply).  The same device code the fused kernels run, so the same bits: a call without
 * DN_PHASE_FROM_INPUT that is handed these phasors as init_angles reproduces the call with the flag bit for bit. */
int dn_stft_phasors(const dn_dsp* d, const float* frames, float* phasors, int32_t B, uint32_t flags, void* stream);

/* Scratch the fused entry points need, in bytes, for a batch of B streams. */
size_t dn_workspace_bytes(const dn_dsp* d, int32_t B);
/* The same for a call with `flags`: dn_workspace_bytes(d, B) when DN_PHASE_FROM_INPUT is not set; with it, plus the phasor rows --
 * 3 K complex values a stream, rounded up to 256 bytes.  (0 for unknown flag bits.) */
size_t dn_workspace_bytes_ex(const dn_dsp* d, int32_t B, uint32_t flags);

/* The whole per-hop body for B streams (app3.py:178-217): frames [dev][B][n_fft] raw samples,
 * hx [dev][B][17][C] in/out, out [dev][B][n_fft] = GriffinLim(...) * peak.
 * mel_residual_out [dev][B][3][M] or NULL receives the model output (predicted_diff_mel).
 * workspace [dev] of dn_workspace_bytes(d, B) bytes.  ONE launch (one workgroup per stream runs P1-P12 back to back);
 * no hop of added latency.  flags: DN_CONV_BF16, DN_PHASE_FROM_INPUT (then workspace of dn_workspace_bytes_ex(d, B, flags) bytes and
 * init_angles NULL) or 0. */
int dn_process_frame(const dn_model* m, const dn_dsp* d, const float* frames, float* hx, float* out,
                     float* mel_residual_out, const float* init_angles, uint64_t seed, uint64_t stream_id0,
                     int32_t n_iter, float momentum, void* workspace, int32_t B, uint32_t flags, void* stream);

/* Streaming step (app3.py:178-226): ring [dev][B][n_fft] holds the last n_fft input samples per stream;
 * hop_in [dev][B][hop] new samples are shifted in first.  ola [dev][B][n_fft] is the output
 * overlap-add buffer; hop_out [dev][B][hop] receives ola[:hop] before the shift (app3.py:219-224).
 * ONE launch; every argument is validated before it, so a failed call leaves ring, ola and hx untouched.  flags as dn_process_frame. */
int dn_stream_step(const dn_model* m, const dn_dsp* d, const float* hop_in, float* ring, float* ola, float* hx,
                   float* hop_out, const float* init_angles, uint64_t seed, uint64_t stream_id0, int32_t n_iter,
                   float momentum, void* workspace, int32_t B, uint32_t flags, void* stream);

/* ---- Clip mode: N hops per call --------------------------------------------------------------------
 * For a caller that already holds the audio (a recorded file, a buffered upload, a backlog): exactly N consecutive
 * dn_stream_step calls for B streams, hop i with seed + i -- the same hops out, ring, ola and hx, bit for bit -- as a fixed
 * number of launches, whatever N: the analysis of all B x N frames at once, the N model forwards of a stream back to back
 * in one workgroup (hx is the only chain from hop to hop), all B x N Griffin-Lim chains side by side over the whole GPU,
 * then the overlap-add across hops.  No call synchronises.
 *   hops_in  [dev][B][N*hop]  float32, or int16 PCM (x / 32767) when in_s16
 *   ring, ola [dev][B][n_fft], hx [dev][B][17][C]: the stream state of dn_stream_step, advanced in place by N hops
 *   hops_out [dev][B][N*hop]  float32, or int16 (clip, * 32767, truncate) when out_s16; must not overlap hops_in
 *   init_angles [dev][B][N][3][K] complex or NULL (NULL: hop i of stream b draws from (seed + i, stream_id0 + b))
 *   workspace [dev] of dn_clip_workspace_bytes(d, B, N) bytes, 16-byte aligned: (n_fft + 6 M + 1) floats a frame
 *   (1540 + 6 M + 1 at n_fft 1024: ~8 KB at 80 mels), rounded up to 256 bytes, plus 256.
 * All three transform sizes.  flags: DN_CONV_BF16, and at most one of the two below (both: DN_ERR_INVALID); with neither the
 * library picks: n_fft 1024 runs a wavefront per frame from 1,024 frames (B x N) a call on, everything else a wavefront per
 * column.  Either way the same bits.  Every argument is validated before the first launch (N >= 1, B >= 1, B x N <= 2^22), so a
 * failed call leaves ring, ola and hx untouched. */
#define DN_CLIP_GL_PER_COLUMN 2u   /* chains: one workgroup per frame, a wavefront per column (gl_body)            */
#define DN_CLIP_GL_PER_STREAM 4u   /* chains: a wavefront per frame, four frames a workgroup (glw_body; n_fft 1024, else DN_ERR_UNSUPPORTED) */
size_t dn_clip_workspace_bytes(const dn_dsp* d, int32_t B, int32_t N);
/* With DN_PHASE_FROM_INPUT in `flags` (the only bit that changes the size; the others a call may carry are accepted): plus the phasor rows of the
 * B x N frames, 3 K complex each, rounded up to 256 bytes -- what dn_clip_process wants when called with that flag.  Else dn_clip_workspace_bytes. */
size_t dn_clip_workspace_bytes_ex(const dn_dsp* d, int32_t B, int32_t N, uint32_t flags);
int dn_clip_process(const dn_model* m, const dn_dsp* d, const void* hops_in, int32_t in_s16, float* ring, float* ola,
                    float* hx, void* hops_out, int32_t out_s16, const float* init_angles, uint64_t seed,
                    uint64_t stream_id0, int32_t n_iter, float momentum, void* workspace, int32_t B, int32_t N,
                    uint32_t flags, void* stream);

/* ---- Clip mode, ragged: every stream its own number of hops ---------------------------------------------
 * Clips of different lengths (a folder of files, a batch of uploads, a backlog) in ONE call.  For every stream b with
 * n_hops[b] >= 1 the call does exactly what dn_clip_process does with B = 1, N = n_hops[b], seed + frame0[b] and
 * stream_id0 + b on that stream's rows -- n_hops[b] consecutive dn_stream_step calls, the same hops out, ring, ola and hx,
 * bit for bit: hop i of stream b draws from (seed + frame0[b] + i, stream_id0 + b).  With F = sum n_hops and
 * off[b] = n_hops[0] + ... + n_hops[b-1]:
 *   n_hops  [host][B]  >= 0;   frame0 [host][B] or NULL (zeros).  Both are the caller's again when the call returns.
 *   hops_in, hops_out [dev][F*hop]  packed, float32 or int16 as in the uniform call: stream b's hops start at off[b]*hop
 *   init_angles [dev][F][3][K] complex or NULL, frame off[b] + i = hop i of stream b
 *   ring, ola [dev][B][n_fft], hx [dev][B][17][C] as in the uniform call.  A stream with n_hops[b] == 0 has no rows in the
 *   packed arrays and is left exactly as it was: no byte of its ring, ola or hx is written.
 *   workspace [dev] of dn_clip_ragged_workspace_bytes(d, B, F, flags) bytes, 16-byte aligned: the table -- off [B+1] int32,
 *   padded to an 8-byte boundary, then frame0 [B] uint64 -- rounded up to 256 bytes, then the uniform call's layout for F
 *   frames (frame rows | mel | residual | peak, rounded up to 256 bytes, plus 256; the phasor rows with
 *   DN_PHASE_FROM_INPUT).  The size depends on B only through the table; it is 0 for a null plan, B < 1, total_hops < 1,
 *   total_hops > 2^22 or unknown flag bits.
 * flags and their refusals are the uniform call's (with neither chain flag n_fft 1024 runs a wavefront per frame from 1,024
 * frames F on).  Everything is validated on the host before anything is enqueued -- B >= 1, n_hops non-NULL and every entry
 * >= 0, F <= 2^22, non-NULL pointers when F > 0 -- so a failed call leaves ring, ola, hx, hops_out and the workspace
 * untouched; F == 0 returns DN_OK with nothing enqueued.  A frame finds its stream by bisection in off on the device.
 * The library builds the table in host memory of its own and copies it to the head of the workspace with a stream-ordered
 * copy on `stream`.  That source is pageable, so the copy completes before the call returns: this is the one clip call
 * that may wait for earlier work on `stream`, and it cannot be captured into a hipGraph. */
size_t dn_clip_ragged_workspace_bytes(const dn_dsp* d, int32_t B, int64_t total_hops, uint32_t flags);
int dn_clip_process_ragged(const dn_model* m, const dn_dsp* d, const void* hops_in, int32_t in_s16, float* ring, float* ola,
                           float* hx, void* hops_out, int32_t out_s16, const float* init_angles, uint64_t seed,
                           uint64_t stream_id0, const int32_t* n_hops, const uint64_t* frame0, int32_t n_iter,
                           float momentum, void* workspace, int32_t B, uint32_t flags, void* stream);

/* ---- Software-pipelined hops ------------------------------------------------------------------------
 * Consecutive hops depend on each other only through hx (the model); hop n's Griffin-Lim (~3/4 of a hop) is
 * independent of hop n+1's analysis + model + inverse mel.  A dn_pipe overlaps them inside ONE launch per hop:
 * dn_pipe_submit(hop n+1) launches a grid whose first B workgroups run hop n's Griffin-Lim and whose next B run
 * hop n+1's P1-P10 (double-buffered scratch); dn_pipe_flush launches the last pending Griffin-Lim.  Everything is
 * enqueued on `stream`; the output of a submitted hop is complete (in stream order) after the NEXT submit or the
 * flush.  `frames`, `hx` and `out` of a submit must stay valid and untouched until then (hx is advanced in place, hop by
 * hop); `init_angles` is copied during the submit and is free again once that launch ran.
 *
 * Replayable launches: everything that changes from hop to hop (scratch-slot parity, whether a hop is pending, the ring
 * priming of new streams, the frame index that keys the Griffin-Lim seed) lives in a device-resident control block that the
 * last workgroup of every launch advances.  A dn_pipe_submit / dn_pipe_stream_push captured into a hipGraph can therefore be
 * replayed indefinitely (BASELINE config 5: the captured streaming step); the caller rewrites the contents of the buffers
 * whose pointers were captured.  The Griffin-Lim of frame f draws its phases from (seed + f, stream_id0 + stream), f counted
 * per pipe from 0 (dn_pipe_stream_set_state can restore it), so a replayed launch does not repeat phases and a resumed
 * stream continues the sequence of the uninterrupted one.
 *
 * Reconfiguring a live pipe: a pipe may change mode while it carries a stream.  dn_pipe_set_head_start, dn_pipe_set_gl_schedule and
 * dn_pipe_set_split may be called between any two launches, with a hop in flight: a frame carries what it needs in its scratch slot (a chain
 * parked under one schedule is resumed under the other).  dn_pipe_set_depth, dn_pipe_set_group and dn_pipe_stream_set_state want a drained pipe
 * (after create, dn_pipe_flush, depth x dn_pipe_stream_flush or dn_pipe_stream_flush_group; the first two refuse a pipe with hops in flight, the
 * third drops them).  Across every such switch frames, hx, emitted samples and the seed sequence (frame f draws from seed + f) continue bit for
 * bit as on a pipe that was never reconfigured; a setter that returns an error has changed nothing.  The priming count behind *hops_valid of
 * dn_pipe_stream_flush_group covers every hop this pipe has taken: single-hop pushes before dn_pipe_set_group count (the setter reads the
 * control block), as do restored states, so a stream that was primed by single pushes gets H valid hops from its first group.
 *
 * A pipe holds a reference on its model and plan: dn_model_destroy / dn_dsp_destroy while a pipe still uses them only drop
 * the creator's reference.  dn_pipe_set_model rebinds a pipe to other weights between two launches (launches already
 * enqueued keep reading the old model: keep it alive until they have run).  flags: DN_CONV_BF16, DN_PHASE_FROM_INPUT or 0.
 * An input-phase pipe (DN_PHASE_FROM_INPUT) allocates the slots' init area at create, as dn_pipe_reserve_parity does, so a captured push allocates
 * nothing: every front half leaves its frame's phasors there, in every mode (head start, either schedule, depth, split, groups). */
typedef struct dn_pipe dn_pipe;
int dn_pipe_create(const dn_model* m, const dn_dsp* d, int32_t B, uint32_t flags, dn_pipe** out);
void dn_pipe_destroy(dn_pipe* p);
int dn_pipe_set_model(dn_pipe* p, const dn_model* m);
/* Head start: a front workgroup is done with P1-P10 well before the pending hop's Griffin-Lim chain (same launch) is; with
 * `iterations` > 0 it goes on with the first iterations of ITS frame's chain and parks it in HBM, and the next launch resumes there.
 * Same results bit for bit, no added latency; pays when there is about one stream per CU.  dn_pipe_create turns it on by itself up to
 * 256 streams (8 iterations at n_fft 1024, 12 at 1536: the measured optima; 512 takes 1024's).  Call between launches (0 = off). */
int dn_pipe_set_head_start(dn_pipe* p, int32_t iterations);
/* Depth of the pipe = hops of ONE stream in flight (n_fft 1024; DN_ERR_UNSUPPORTED at 1536, where the per-lane state of a stream does not fit one wavefront, and at 512, where the schedule is not built).  1 (default): hop n's Griffin-Lim runs beside hop n+1's front half, as
 * described above.  D > 1: a frame's Griffin-Lim chain is cut into D segments that run in the D launches after its submit -- one wavefront
 * per stream and segment (DN_GL_WAVE_PER_STREAM), the chain parked in HBM between launches at the top of an iteration, so the result is
 * bit-identical to depth 1 -- and a launch carries the segments of D different hops of every stream.  With about one stream per CU (the
 * batch-256 metric) that is what fills the CU: the throughput of the saturated regime for D - 1 more hops of latency.  The output of a submit
 * is then complete after the D-th launch that follows it (dn_pipe_flush runs as many as are needed); a stream push emits the samples of the
 * frame delivered D pushes earlier, and dn_pipe_stream_flush must be called D times to drain (each call emits one hop).
 * Call while nothing is in flight (after create or flush); synchronises the device. */
#define DN_PIPE_MAX_DEPTH 4
int dn_pipe_set_depth(dn_pipe* p, int32_t depth);
/* Hop groups (n_fft 1024; DN_ERR_UNSUPPORTED at 1536, where the form measured slower than the one-hop pipe, and at 512, where it is not built): the loop body of app3.py:178-226 for `hops` CONSECUTIVE hops of every stream in ONE launch.
 * A deep pipe (above) pays for every launch boundary inside a Griffin-Lim chain: the chain parks in HBM and comes back at the head of the next
 * launch.  With dn_pipe_set_group(p, H), 1 <= H <= DN_PIPE_MAX_GROUP, a launch is as long as a chain instead: dn_pipe_submit_group carries up to H
 * new hops of every stream -- hop h of the group reads frames + h * frames_stride, its front half (P1-P10) runs behind hop h-1's with hx handed on,
 * its result goes to out + h * out_stride, its injected phases (parity mode) come from init_angles + h * init_stride (strides in floats) -- beside
 * the WHOLE chains of the hops the previous launch fronted, one wavefront each.  Nothing is parked between launches; frames, hx and samples are
 * those of the one-hop pipe bit for bit (same seeds: the f-th frame of the pipe draws from seed + f).  The output of a group is complete after
 * the next dn_pipe_submit_group or one dn_pipe_flush.  Throughput of the deep pipe without its hand-off, for input that arrives H hops at a time.
 * Streaming form: dn_pipe_stream_push_group takes exactly H hops (hop_in + h * in_stride, elements of the input type) and emits H hops
 * (hop_out + i * out_stride); the emitted stream is the one-hop pipe's delayed by H - 1 more hops (zeros until then), and
 * dn_pipe_stream_flush_group emits the frames still pending first and zero hops behind them (always H hops; *hops_valid, may be NULL, says how
 * many carry samples as far as this host thread's own pushes tell -- after graph replays ask dn_pipe_get_counters for `pending` before the flush).
 * With H < 4 a workgroup's four wavefronts serve 4 / H streams (H = 2: two streams a workgroup -- what 512 to 768 streams per GPU want).
 * dn_pipe_set_group: call while nothing is in flight; H = 0 returns the pipe to single hops; synchronises the device; excludes depth > 1, a head
 * start and the host-buffer transport.  dn_pipe_submit on a group pipe is a group of one hop. */
#define DN_PIPE_MAX_GROUP 4
int dn_pipe_set_group(dn_pipe* p, int32_t hops);
int dn_pipe_submit_group(dn_pipe* p, const float* frames, int64_t frames_stride, float* hx, float* out, int64_t out_stride,
                         const float* init_angles, int64_t init_stride, uint64_t seed, uint64_t stream_id0, int32_t hops,
                         int32_t n_iter, float momentum, void* stream);
int dn_pipe_stream_push_group(dn_pipe* p, const void* hop_in, int64_t in_stride, int32_t in_is_s16, void* hop_out, int64_t out_stride,
                              int32_t out_is_s16, const float* init_angles, int64_t init_stride, uint64_t seed, uint64_t stream_id0,
                              int32_t n_iter, float momentum, void* stream);
int dn_pipe_stream_flush_group(dn_pipe* p, void* hop_out, int64_t out_stride, int32_t out_is_s16, int32_t* hops_valid, void* stream);
/* How the pending hop's Griffin-Lim is laid out on the GPU (n_fft 1024; results are bit-identical either way; at 512 and 1536 only the
 * per-column form exists: DN_GL_AUTO resolves to it and DN_GL_WAVE_PER_STREAM is DN_ERR_UNSUPPORTED):
 *   DN_GL_WAVE_PER_COLUMN  three wavefronts per stream, one per STFT column: the shortest chain for one stream -- right when there is
 *                          about one stream per CU (the batch-256 metric);
 *   DN_GL_WAVE_PER_STREAM  one wavefront per stream, the three columns interleaved inside it, four streams per workgroup: no workgroup
 *                          barrier, the overlap-add in registers, four times the streams in flight -- right for several streams per CU;
 *   DN_GL_AUTO (default)   per stream from 768 streams per pipe on (three per CU of an MI355X: the measured crossover), per column below.
 * Call between launches.  A deep pipe and a group pipe run a wavefront per stream whatever is set here: DN_GL_WAVE_PER_COLUMN on either is
 * DN_ERR_INVALID, and a schedule set before dn_pipe_set_depth / dn_pipe_set_group takes effect again at depth 1 / after dn_pipe_set_group(p, 0). */
#define DN_GL_AUTO 0
#define DN_GL_WAVE_PER_COLUMN 1
#define DN_GL_WAVE_PER_STREAM 2
int dn_pipe_set_gl_schedule(dn_pipe* p, int32_t schedule);
/* A hop as TWO launches instead of one: first the Griffin-Lim chains of the hops in flight (what a flush launch is), then the new hop's front
 * halves (P1-P10) as a launch of their own.  Where a launch carries several times the workgroups the GPU holds at once its chains and its front
 * halves run as two phases anyway, and a front workgroup compiled into the same kernel as a chain inherits the chain's register budget (two
 * workgroups per CU); on their own four fit.  Only with the wavefront-per-stream schedule (n_fft 1024; DN_SPLIT_ON is DN_ERR_UNSUPPORTED at 512 and 1536) and no head start; same control block,
 * same samples, still capturable (two kernel nodes).  DN_SPLIT_AUTO (default) decides from the number of chain wavefronts per launch. */
#define DN_SPLIT_AUTO (-1)
#define DN_SPLIT_OFF 0
#define DN_SPLIT_ON 1
int dn_pipe_set_split(dn_pipe* p, int32_t mode);
/* Allocates the per-slot buffers for injected initial phases now (otherwise the first submit/push with init_angles does it):
 * call before capturing a parity-mode launch into a hipGraph, where allocation is not allowed. */
int dn_pipe_reserve_parity(dn_pipe* p);
int dn_pipe_submit(dn_pipe* p, const float* frames, float* hx, float* out, const float* init_angles, uint64_t seed,
                   uint64_t stream_id0, int32_t n_iter, float momentum, void* stream);
/* Runs the pending hop's Griffin-Lim; a no-op launch when nothing is pending.  A pending hop is always finished with the n_iter,
 * momentum and `out` of ITS OWN submit (they travel with the frame in its scratch slot): the n_iter / momentum arguments of a flush
 * are validated and otherwise unused, a later submit with other values does not change a hop already submitted, and a captured
 * submit may be replayed between eager submits to other `out` buffers. */
int dn_pipe_flush(dn_pipe* p, int32_t n_iter, float momentum, void* stream);
/* Host copy of the control block (pushes, frames, pending; any may be NULL).  Synchronises `stream`. */
int dn_pipe_get_counters(dn_pipe* p, uint64_t* pushes, uint64_t* frames, int32_t* pending, void* stream);

/* Streaming form (BASELINE config 5; app3.py:168-250 without the av container): the pipe owns the per-stream state
 * (input ring, output overlap-add line, hx -- app3.py:130-133) in HBM and every push is ONE launch.
 *   hop_in  [dev][B][hop]  float32 samples, or int16 PCM when in_is_s16 (converted as app3.py:172: x / 32767)
 *   hop_out [dev][B][hop]  float32, or int16 when out_is_s16 (clip to [-1,1], * 32767, truncate: app3.py:244-245)
 * The first n_fft/hop - 1 pushes only fill the ring.  Because hops are software-pipelined, the samples the reference
 * would emit while processing frame f (ola[:hop] before frame f is added, app3.py:219-220) come out of the push
 * that follows the one that delivered frame f's last hop -- one hop of extra latency; zeros until then.
 * dn_pipe_stream_flush emits the last pending hop (zeros when none is pending); as in frame mode a pending hop is finished with
 * the n_iter / momentum of the push that delivered it. */
int dn_pipe_stream_create(const dn_model* m, const dn_dsp* d, int32_t B, uint32_t flags, dn_pipe** out);
int dn_pipe_stream_push(dn_pipe* p, const void* hop_in, int32_t in_is_s16, void* hop_out, int32_t out_is_s16,
                        const float* init_angles, uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum,
                        void* stream);
int dn_pipe_stream_flush(dn_pipe* p, void* hop_out, int32_t out_is_s16, int32_t n_iter, float momentum, void* stream);
/* Host-buffer transport of the streaming form: the reference hands every hop across the host/device boundary (frames arrive as int16 arrays on
 * the host, app3.py:168-172; x.to(device) / y.cpu() around the hop, app3.py:189,215; int16 out, app3.py:244-250).  hop_in_host / hop_out_host
 * [host][B][hop] (int16 or float32).  The call enqueues on `stream` and returns without waiting.
 *   Page-locked buffers (hipHostMalloc, hipHostRegister, torch pin_memory): ZERO COPY -- the launch reads each stream's hop (1 KB) straight from
 *   host memory and stores the emitted hop straight into it; no copy engine and no second queue are involved.
 *   Pageable buffers, or flags = DN_HOST_STAGED: an upload on a copy queue of the pipe, the hop on `stream` behind it, a download on a second copy
 *   queue; device staging is double-buffered, so the upload of hop i+1 and the download of hop i-1 run while hop i computes.
 * `*ticket` (may be NULL) names the push: dn_pipe_stream_host_wait(p, ticket) blocks the calling thread until that push's samples are in ITS
 * hop_out_host.  hop_in_host must stay unchanged, and hop_out_host untouched, until then (wait for push i before reusing the buffers of push i;
 * with four sets in rotation the host can stay two pushes ahead of the result it waits for, which keeps the GPU busy back to back).  Initial phases
 * come from the device generator; mix freely with dn_pipe_stream_push / _flush on the same `stream`.
 *   flags = DN_HOST_DEFER (zero copy only; ignored otherwise): the launch leaves its emitted hop in a device staging buffer and the NEXT push's
 *   launch moves it to hop_out_host, each front workgroup its stream's row before it starts on its own hop -- the PCIe writes then overlap a hop's
 *   arithmetic instead of ending the launch as one burst (1,024 streams: 2 MB in 14 us of a 170 us launch).  The samples of push i are in host
 *   memory once push i + 1 has run; dn_pipe_stream_host_wait on the NEWEST push enqueues the move itself (on the stream of that push), so no
 *   result is ever stranded.  Same samples, one push later: for a host that stays ahead of the results it waits for, not for the lowest latency.
 */
#define DN_HOST_STAGED 1u
#define DN_HOST_DEFER 2u
int dn_pipe_stream_push_host(dn_pipe* p, const void* hop_in_host, int32_t in_is_s16, void* hop_out_host, int32_t out_is_s16,
                             uint64_t seed, uint64_t stream_id0, int32_t n_iter, float momentum, uint32_t flags, void* stream,
                             uint64_t* ticket);
int dn_pipe_stream_host_wait(dn_pipe* p, uint64_t ticket);
/* Checkpoint / resume of live streams: copy the pipe-owned state out to / in from caller buffers [dev]
 * (ring [B][n_fft], ola [B][n_fft], hx [B][17][C]; any may be NULL), ordered on `stream`.  Take snapshots after
 * dn_pipe_stream_flush: set_state drops a pending hop.  A restored ring counts as primed; frames_done (the `frames`
 * counter of dn_pipe_get_counters at snapshot time) makes the resumed stream continue the seed sequence. */
int dn_pipe_stream_get_state(dn_pipe* p, float* ring, float* ola, float* hx, void* stream);
int dn_pipe_stream_set_state(dn_pipe* p, const float* ring, const float* ola, const float* hx, uint64_t frames_done,
                             void* stream);

/* ---- Session pools: streams that join, leave and push hops on their own ------------------------------
 * Every interface above advances ALL B streams of a batch by the same hop.  A session pool holds `capacity` stream slots
 * instead, each with its own state in HBM, owned by the library: ring [cap][n_fft], overlap-add line [cap][n_fft],
 * hx [cap][17][C], a frame counter, a priming count and a Griffin-Lim stream id.  One push runs one hop for a LIST of
 * slots -- any subset, in any order -- and leaves every other slot exactly as it was: one WebRTC session per slot
 * (app3.py:123-133), each of whose recv() calls runs 0, 1 or 2 hops (app3.py:167-178), batched onto the GPU tick by tick.
 *
 *   dn_sessions_open   (re)opens n slots: ring, ola and hx zeroed, frame and priming counts 0, Griffin-Lim stream id
 *                      stream_ids[i] (stream_ids NULL: the slot index).  Enqueued on `stream`.
 *   dn_sessions_close  closes n slots (host bookkeeping only: a closed slot may not be pushed until it is opened again).
 *   dn_sessions_push   one hop for each of the n listed slots.  ids [host][n]; the rows of hop_in [dev][n][hop],
 *                      hop_out [dev][n][hop] and init_angles [dev][n][3][K] complex (NULL: device RNG) are in LIST order.
 *                      in_is_s16 / out_is_s16 as dn_pipe_stream_push (x / 32767 in; clip, * 32767, truncate out).
 *                      A slot's first n_fft/hop - 1 pushes only shift its ring and emit a zero row; after that every push
 *                      runs one frame with no added latency and emits ola[:hop] before the frame is added (app3.py:219-224),
 *                      exactly as dn_stream_step.  The slot's f-th frame (f counted from its open) draws its phases from
 *                      (seed + f, its stream id): a session's samples do not depend on which other slots share a push.
 *
 * The id lists are validated on the HOST before anything is enqueued: every id in [0, capacity), none twice, and (push,
 * close) every slot open.  A bad list returns DN_ERR_INVALID and leaves all state as it was.  The library moves the ids to
 * the device itself (a page-locked staging ring guarded by events): the caller may reuse its array once the call returns.
 * Consecutive calls on one pool are ordered by `stream`: use one stream per pool.
 * NOT thread-safe (one host thread at a time per pool) and NOT capturable into a hipGraph (the list changes every tick).
 *
 * Schedules (dn_sessions_set_schedule):
 *   DN_SESS_ONE_LAUNCH    one workgroup per listed slot runs P1-P12 back to back (n_fft 512, 1024 and 1536);
 *   DN_SESS_TWO_LAUNCHES  the front halves (P1-P10) of all listed slots, then their Griffin-Lim chains a wavefront per
 *                         session (n_fft 1024; DN_ERR_UNSUPPORTED at 512 and 1536); the same samples, bit for bit;
 *   DN_SESS_AUTO          (default) two launches from 1,024 listed slots on at n_fft 1024 (the measured crossover: DESIGN.md 4.11).
 * flags of dn_sessions_create: DN_CONV_BF16, DN_PHASE_FROM_INPUT (the pool then holds phasor rows for its capacity; both schedules; records are the
 * same, so a record exported from a pool in either mode imports into a pool in the other) or 0.  The pool holds a reference on its model and plan (as a dn_pipe). */
typedef struct dn_sessions dn_sessions;
#define DN_SESS_AUTO 0
#define DN_SESS_ONE_LAUNCH 1
#define DN_SESS_TWO_LAUNCHES 2
int dn_sessions_create(const dn_model* m, const dn_dsp* d, int32_t capacity, uint32_t flags, dn_sessions** out);
void dn_sessions_destroy(dn_sessions* s);
int dn_sessions_open(dn_sessions* s, const int32_t* ids, int32_t n, const uint64_t* stream_ids, void* stream);
int dn_sessions_close(dn_sessions* s, const int32_t* ids, int32_t n);
int dn_sessions_push(dn_sessions* s, const int32_t* ids, int32_t n, const void* hop_in, int32_t in_is_s16, void* hop_out,
                     int32_t out_is_s16, const float* init_angles, uint64_t seed, int32_t n_iter, float momentum, void* stream);
int dn_sessions_set_schedule(dn_sessions* s, int32_t schedule);
/* the slot's counters as of the last call on `stream` (synchronises it): frames run since its open, pushes counted up to
 * n_fft/hop - 1 (primed when equal) */
int dn_sessions_get_counters(dn_sessions* s, int32_t id, uint64_t* frames, int32_t* pushes, void* stream);

/* ---- Session records: export and import the state of sessions ---------------------------------------
 * A session's whole state leaves its pool as one self-contained RECORD and enters any pool of the same geometry: a full
 * pool grows (a larger pool imports every session at its slot number), a GPU is drained onto another, sessions are
 * suspended to host memory or a file and resumed in a new process.  Continuation is bit-exact: after an import a
 * session emits the samples it would have emitted in its old pool.
 *
 * Record layout, version 1 (DN_SESS_RECORD_VERSION; little-endian, offsets in bytes from the start of the record):
 *     0  header, 64 B: dn_session_record_header below
 *    64  ring [n_fft]   float32                      the input ring buffer (app3.py:176)
 *   R_o  ola  [n_fft]   float32  R_o = 64 + A(4 n_fft)      the overlap-add line (app3.py:133)
 *   H_o  hx   [17][C]   float32  H_o = R_o + A(4 n_fft)     the GRU hidden state
 *   stride = dn_sessions_record_bytes = round_up(H_o + 4 * 17 * C, 256);  A(x) = round_up(x, 16); the rest is zero.
 * n_fft 1024 / 80 mels: 8,704 B a record; n_fft 512 / 64 mels: 4,608 B.  A list of n records is [n][stride], record i at i * stride, in device memory
 * aligned to 16 bytes (else DN_ERR_INVALID).
 * The header's counters are the slot's: `pushes` counts its pushes up to n_fft/hop - 1 (primed when equal), `frames`
 * the frames run since its open (frame f draws its phases from (seed + f, stream_id)).
 *
 * Neither the weights nor conv_precision are recorded or checked: importing onto updated weights of the same geometry
 * is a rolling upgrade, as dn_pipe_set_model allows for a pipe.  The seed is the caller's (an argument of every push):
 * push with the seed of the pool that exported, or the continuation is not bit-exact.
 *
 *   dn_sessions_record_bytes  the stride of one record for this pool's geometry (0 for a null pool).
 *   dn_sessions_export  writes the records of the n listed slots to records [dev][n][stride] in list order.  Every id in
 *                       range, none twice, every slot open (checked on the host: DN_ERR_INVALID, nothing enqueued).
 *                       Enqueued on `stream`: it sees every earlier push on that stream.  It changes nothing in the
 *                       pool -- an exported session that keeps running gives the same bits as one never exported.
 *   dn_sessions_import  (re)opens the n listed slots with the state of records [dev][n][stride] (record i -> slot
 *                       ids[i]), as dn_sessions_open does; every other slot is left alone.  stream_ids [host][n]
 *                       overrides the recorded Griffin-Lim stream ids (NULL: keep them), so the sessions of two pools do
 *                       not collide on phase keys.  Every record is validated before any slot changes: magic, version,
 *                       a geometry equal to this pool's (sample_rate, n_fft, hop, n_mels, hidden, C) and a priming count
 *                       <= n_fft/hop - 1, plus the id checks of dn_sessions_open (in range, none twice).  On any failure
 *                       it returns DN_ERR_INVALID with a message and the pool is exactly as before.
 *                       Validation reads the headers on the host: import SYNCHRONISES `stream` (one check launch
 *                       into page-locked memory, one synchronisation), then enqueues the copy into the slots. */
#define DN_SESS_RECORD_MAGIC 0x52534E44u    /* "DNSR" */
#define DN_SESS_RECORD_VERSION 1
typedef struct dn_session_record_header {
    uint32_t magic;          /* DN_SESS_RECORD_MAGIC */
    uint32_t version;        /* DN_SESS_RECORD_VERSION */
    uint32_t sample_rate, n_fft, hop, n_mels;
    uint32_t hidden;         /* 17 */
    uint32_t C;              /* n_mels / 16 */
    uint32_t pushes;         /* priming count, up to n_fft/hop - 1 */
    uint32_t reserved0;      /* 0 */
    uint64_t frames;         /* frames since the session's open */
    uint64_t stream_id;      /* Griffin-Lim stream id */
    uint64_t reserved1;      /* 0 */
} dn_session_record_header;
size_t dn_sessions_record_bytes(const dn_sessions* s);
int dn_sessions_export(dn_sessions* s, const int32_t* ids, int32_t n, void* records, void* stream);
int dn_sessions_import(dn_sessions* s, const int32_t* ids, int32_t n, const void* records, const uint64_t* stream_ids,
                       void* stream);

/* ---- Sample-rate conversion ---------------------------------------------------------------------------------
 * torchaudio.transforms.Resample (2.6.0) on the device: the transform the reference builds as Resample(44100, SR) and
 * Resample(SR, 44100) at utils.py:48-49 and replaces with librosa.resample at app.py:181.  Audio that arrives at another rate
 * than the plan's (8 kHz files, 44.1 kHz uploads, 48 kHz WebRTC) is converted where it already is, float32 or int16 PCM.
 *
 * Arithmetic (restated from torchaudio's _get_sinc_resample_kernel / _apply_sinc_resample_kernel; parity with torchaudio itself
 * is unpinned).  With g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g:
 *   base = min(o, n) * rolloff      width = ceil(lowpass_filter_width * o / base)      taps KW = 2 width + o
 *   k[p][j], p in [0, n), j in [0, KW), in double, rounded once to float32:
 *     t = (-p / n + (j - width) / o) * base, clamped to +-lowpass_filter_width
 *     k = sinc(pi t) * cos^2(t pi / lowpass_filter_width / 2) * base / o          (sinc(0) = 1; the Hann window)
 *   y[q n + p] = sum_j k[p][j] * xz[q o + j - width],  xz = x with zeros outside [0, L);  ceil(n L / o) samples out
 * On the device one output is ONE chain acc = fmaf(k[p][j], x, acc) over j ascending from acc = 0, in every kernel form and in
 * both entry points; the bit-for-bit statements below rest on that order.
 *
 * cfg: equal rates, a rate < 1, lowpass_filter_width < 1 or rolloff outside (0, 1]: DN_ERR_INVALID.  o or n > 1024, or
 * n * KW > 2^19 floats: DN_ERR_UNSUPPORTED (the message names the limits).
 * kernel [host][n][KW] or NULL: a caller-built table (torchaudio's Kaiser window, anything else) in place of the Hann table
 * above, as dn_dsp_create takes fb / pinv / window; its geometry is still cfg's (read it back from a handle created with NULL).
 * The handle lives on the current HIP device, is immutable and may be shared by threads. */
typedef struct dn_resampler dn_resampler;
typedef struct dn_resample_cfg {
    int32_t orig_freq;
    int32_t new_freq;
    int32_t lowpass_filter_width; /* torchaudio's default: 6 */
    double rolloff;               /* torchaudio's default: 0.99 */
} dn_resample_cfg;
int dn_resample_create(const dn_resample_cfg* cfg, const float* kernel, dn_resampler** out);
void dn_resample_destroy(dn_resampler* r);
/* o, n, width, taps (KW) and delay_blocks (D = ceil(width / o)); any of the pointers may be NULL */
int dn_resample_geometry(const dn_resampler* r, int32_t* o, int32_t* n, int32_t* width, int32_t* taps, int32_t* delay_blocks);
/* kernel [host][n][KW]: the float32 table as held */
int dn_resample_get_kernel(const dn_resampler* r, float* kernel);
/* ceil(n L / o); 0 for a null handle or L < 1 */
int64_t dn_resample_out_len(const dn_resampler* r, int64_t L);

/* The whole-signal form: B rows of L samples -> B rows of dn_resample_out_len(r, L) samples, one launch; no workspace, no
 * allocation, no synchronisation.
 *   x [dev][B][x_stride]  float32, or int16 PCM (x / 32767) when in_s16; x_stride >= L elements
 *   y [dev][B][y_stride]  float32, or int16 (clip to +-1, * 32767, truncate) when out_s16; y_stride >= the output length
 * (the int16 conventions of dn_stream_step, P12).  Rows need no alignment; rows that start on 16-byte (x) and 8-byte (y; 4 for
 * int16) boundaries are moved in wider accesses.  y must not overlap x.  L >= 1 and at most 2^30 samples in and out;
 * B == 0 returns DN_OK.  A row followed by zeros gives the row's own outputs followed by more: the extra terms are k * 0. */
int dn_resample(const dn_resampler* r, const void* x, int32_t in_s16, void* y, int32_t out_s16, int32_t B, int64_t L,
                int64_t x_stride, int64_t y_stride, void* stream);

/* The streaming form: every push brings `blocks` >= 1 blocks of o samples per stream and emits blocks * n.
 *   state [dev][B][H] float32, H = D o + width, dn_resample_state_bytes(r, B) bytes (0 for a null handle or B < 1): the last H
 *   input samples of each stream, owned by the caller as ring / ola are for dn_stream_step.  All zeros is a fresh stream.
 *   x [dev][B][x_stride], x_stride >= blocks * o;   y [dev][B][y_stride], y_stride >= blocks * n;   formats as above.
 * The concatenated output of a stream is the whole-signal output of (zeros, then the stream) delayed by D blocks:
 *   concat(pushes of L = whole blocks of samples, then a push of D blocks of zeros)[D n : D n + ceil(n L / o)]
 * equals dn_resample of the same L samples bit for bit, however the samples were cut into pushes.  The first D n samples a fresh
 * stream emits are the filter's pre-ringing against the silence before it, not zeros: a caller that wants output sample 0 lined
 * up with input sample 0 drops them.
 * Two launches, in stream order: the outputs from [state | x] (every workgroup reads the old state), then the new state.
 * Every argument of both forms is checked before the first launch: a refused call leaves y and state untouched. */
size_t dn_resample_state_bytes(const dn_resampler* r, int32_t B);
int dn_resample_push(const dn_resampler* r, float* state, const void* x, int32_t in_s16, void* y, int32_t out_s16, int32_t B,
                     int64_t blocks, int64_t x_stride, int64_t y_stride, void* stream);

/* ---- Rate banks: the rate adapters of a session pool -------------------------------------------------------------
 * A pool's tick is a LIST of slots, and its sessions arrive at rates of their own (48 kHz WebRTC, 8 kHz telephony) next to the
 * plan's.  A bank holds, for every session rate r of a small set, the table r -> plan ("down", o_d : n_d) and the table
 * plan -> r ("up", o_u : n_u), both dn_resample_create's Hann tables, and converts every listed row at the rate of its own
 * session in ONE launch a side, updating that session's converter state in the same launch:
 *   dn_ratebank_ingest   x [n][x_stride] at each row's rate  ->  hop_in [n][hop] float32 at the plan's rate
 *   dn_ratebank_emit     hop_out [n][hop] float32            ->  y [n][y_stride] at each row's rate
 * Per hop a session of rate r brings chunk_in = (hop / n_d) o_d samples and receives chunk_out = (hop / o_u) n_u.  A row's samples
 * equal dn_resample_push with that pair's own dn_resampler fed the session's stream alone, bit for bit (the same chain), and
 * so does its state row.  Round-trip lag of a session: D_d n_d plan samples (delay_in) plus D_u n_u samples at its rate
 * (delay_out); the bank does not compensate it.
 *
 * Accepted rates -- both directions of r must
 *   lie inside the small kernel form (n <= 4, o <= 8, n x taps <= 512 floats),
 *   tile the hop (n_d | hop and o_u | hop),
 *   bring at least a history per hop (chunk_in >= H_d; the hop itself >= H_u) and fit the staged tile (chunk_in <= 1536).
 * At a 16 kHz plan (hop 512 or 256) that is 8, 12, 24, 32 and 48 kHz; at 48 kHz / hop 768 it is 12, 16, 24, 32 and 96 kHz.
 * Anything else (44.1 kHz: 441 : 160 tiles no hop) is DN_ERR_UNSUPPORTED at create, the message names the condition.  A rate
 * listed twice, equal to the plan's or < 1, n_rates outside [1, 8], hop < 1: DN_ERR_INVALID.
 *
 * State: state_in / state_out [dev][capacity][dn_ratebank_state_stride(b, side)] float32, the CALLER's, as dn_resample_push's.
 * A slot's row holds the H(rate) leading floats of its session; the rest of the row is never read or written.  All zeros is a
 * fresh session.  Export, import and zeroing on open are plain copies of those rows.
 * slots / rate_idx [host][n]: the listed slots (each in [0, capacity), none twice) and each one's index into cfg.rates, or -1 for
 * a session at the plan's own rate, whose row is the conversion copy of hop samples (x / 32767 in, clip * 32767 truncate out) and
 * has no state.  x_stride / y_stride >= the longest listed chunk; the buffers need hold only (n - 1) stride + the last row's chunk,
 * and what lies in a row beyond its chunk is neither read nor written.
 * Every argument is checked on the host before anything is enqueued: a refused call leaves the outputs and the state
 * untouched.  n == 0 returns DN_OK.  The handle lives on the current HIP device.  It is immutable but for a page-locked staging
 * ring of the (slot, rate) pairs, so it is NOT thread-safe (one host thread a bank) and NOT capturable into a hipGraph. */
typedef struct dn_ratebank dn_ratebank;
typedef struct dn_ratebank_cfg {
    int32_t plan_rate;
    int32_t hop;
    int32_t rates[8];
    int32_t n_rates;
    int32_t lowpass_filter_width; /* 6 */
    double rolloff;               /* 0.99 */
} dn_ratebank_cfg;
#define DN_RATEBANK_IN 0
#define DN_RATEBANK_OUT 1
int dn_ratebank_create(const dn_ratebank_cfg* cfg, dn_ratebank** out);
void dn_ratebank_destroy(dn_ratebank* b);
/* samples per hop in and out, the history of each side (H_d, H_u) and the lags (D_d n_d at the plan's rate, D_u n_u at the
 * session's); any pointer may be NULL */
int dn_ratebank_geometry(const dn_ratebank* b, int32_t rate_index, int32_t* chunk_in, int32_t* chunk_out, int32_t* hist_in,
                         int32_t* hist_out, int32_t* delay_in, int32_t* delay_out);
/* floats per slot of a side's state: the largest H of that side, rounded up to 4; 0 for a null handle or an unknown side */
int32_t dn_ratebank_state_stride(const dn_ratebank* b, int32_t side);
int dn_ratebank_ingest(dn_ratebank* b, const int32_t* slots, const int32_t* rate_idx, int32_t n, int32_t capacity, float* state_in,
                       const void* x, int32_t in_s16, int64_t x_stride, float* hop_in, void* stream);
int dn_ratebank_emit(dn_ratebank* b, const int32_t* slots, const int32_t* rate_idx, int32_t n, int32_t capacity, float* state_out,
                     const float* hop_out, void* y, int32_t out_s16, int64_t y_stride, void* stream);

const char* dn_last_error(void);
int dn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DN_DENOISE_H */
