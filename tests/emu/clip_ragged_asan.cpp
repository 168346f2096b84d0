// TEST INFRASTRUCTURE ONLY -- the ragged clip call (dn_clip_process_ragged) under AddressSanitizer / UBSan on exactly sized heap buffers: the table
// lookup that turns a frame into (stream, hop) is where an out-of-range access of the clip kernels would come from.
// tests/test_emu_clip_ragged_asan.py compiles this file, the host units (dn_api*.hip) and the two clip units (dn_clip.hip, dn_clip_glw.hip: every
// clip kernel with the bodies it inlines) as host C++ against the emulation header (tests/emu/hip/hip_runtime.h) with -fsanitize=address,undefined
// and links what else the host layer refers to from the ordinary libdn_emu.so.  Nothing is preloaded.
//
// Two calls, one Griffin-Lim iteration each, every buffer a heap block of exactly the size the header states:
//   A  n_fft 512, n_hops (2, 0, 1), int16 in and out, a wavefront per column: a zero-length stream between live ones, N = 2 and N = 1 in the fold
//   B  n_fft 1024, n_hops (1, 3, 0), DN_CLIP_GL_PER_STREAM with DN_PHASE_FROM_INPUT: one chain workgroup of four waves, a stream boundary inside it,
//      N >= 3 in the fold, a zero-length stream last
// The streams without hops must keep their state, the others must change theirs, and every sample out must be finite.
//   usage: clip_ragged_asan WEIGHTS.bin      prints "clip_ragged_asan: ok", exit status 0; anything else is a failure
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../include/dn_denoise.h"

namespace {

[[noreturn]] void die(const char* what, int rc) {
    fprintf(stderr, "clip_ragged_asan: %s (%d: %s)\n", what, rc, dn_last_error());
    exit(1);
}

template <typename T>
std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }          // a heap block of exactly n elements, zeroed

template <typename SAMPLE>
void run(const dn_model* m, const dn_dsp_cfg& cfg, const std::vector<int32_t>& n_hops, const std::vector<uint64_t>& frame0, uint32_t flags) {
    dn_dsp* d = nullptr;
    int rc = dn_dsp_create(&cfg, nullptr, nullptr, nullptr, &d);
    if (rc != DN_OK) die("dn_dsp_create", rc);
    const int B = (int)n_hops.size(), n_fft = cfg.n_fft, hop = cfg.hop, hxn = 17 * (cfg.n_mels / 16);
    size_t F = 0;
    for (int32_t n : n_hops) F += (size_t)n;
    constexpr bool s16 = sizeof(SAMPLE) == 2;
    auto in = exact<SAMPLE>(F * hop), out = exact<SAMPLE>(F * hop);
    auto ring = exact<float>((size_t)B * n_fft), ola = exact<float>((size_t)B * n_fft), hx = exact<float>((size_t)B * hxn);
    for (size_t k = 0; k < F * hop; ++k) {
        const float v = 0.3f * sinf(0.05f * (float)k) + 0.01f * (float)(k % 7);
        in[k] = s16 ? (SAMPLE)(v * 32767.0f) : (SAMPLE)v;
    }
    for (size_t k = 0; k < (size_t)B * n_fft; ++k) { ring[k] = 0.1f * cosf(0.03f * (float)k); ola[k] = 0.05f * sinf(0.02f * (float)k); }
    for (size_t k = 0; k < (size_t)B * hxn; ++k) hx[k] = 0.01f * (float)(k % 11);
    const std::vector<float> ring0(ring.get(), ring.get() + (size_t)B * n_fft), ola0(ola.get(), ola.get() + (size_t)B * n_fft),
        hx0(hx.get(), hx.get() + (size_t)B * hxn);
    const size_t need = dn_clip_ragged_workspace_bytes(d, B, (int64_t)F, flags);
    if (need == 0) die("dn_clip_ragged_workspace_bytes returned 0", 0);
    auto ws = exact<uint64_t>(need / sizeof(uint64_t));          // (need is a multiple of 256; operator new aligns to 16 bytes)
    memset(ws.get(), 0xff, need);                                // NaNs
    rc = dn_clip_process_ragged(m, d, in.get(), s16, ring.get(), ola.get(), hx.get(), out.get(), s16, nullptr, 7, 1ull << 40, n_hops.data(),
                                frame0.empty() ? nullptr : frame0.data(), 1, 0.99f, ws.get(), B, flags, nullptr);
    if (rc != DN_OK) die("dn_clip_process_ragged", rc);
    for (int b = 0; b < B; ++b) {
        const bool same = memcmp(ring.get() + (size_t)b * n_fft, ring0.data() + (size_t)b * n_fft, n_fft * sizeof(float)) == 0 &&
                          memcmp(ola.get() + (size_t)b * n_fft, ola0.data() + (size_t)b * n_fft, n_fft * sizeof(float)) == 0 &&
                          memcmp(hx.get() + (size_t)b * hxn, hx0.data() + (size_t)b * hxn, hxn * sizeof(float)) == 0;
        if (same != (n_hops[b] == 0)) die(n_hops[b] == 0 ? "a stream without hops was written" : "a stream with hops kept its state", b);
    }
    for (size_t k = 0; k < F * hop; ++k)
        if (!s16 && !isfinite((float)out[k])) die("a sample out is not finite", (int)k);
    for (size_t k = 0; k < (size_t)B * n_fft; ++k)
        if (!isfinite(ola[k]) || !isfinite(ring[k])) die("the state is not finite", (int)k);
    dn_dsp_destroy(d);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: clip_ragged_asan WEIGHTS.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> w;
    float buf[4096];
    for (size_t n; (n = fread(buf, sizeof(float), 4096, f)) > 0;) w.insert(w.end(), buf, buf + n);
    fclose(f);
    const dn_model_cfg mc{5, 1, 4, 17, 3, 2, 1, 6};
    dn_model* m = nullptr;
    const int rc = dn_model_create(w.data(), w.size(), &mc, &m);
    if (rc != DN_OK) die("dn_model_create", rc);
    run<int16_t>(m, dn_dsp_cfg{16000, 512, 256, 64}, {2, 0, 1}, {5, 9, 2}, 0);
    run<float>(m, dn_dsp_cfg{16000, 1024, 512, 80}, {1, 3, 0}, {}, DN_CLIP_GL_PER_STREAM | DN_PHASE_FROM_INPUT);
    dn_model_destroy(m);
    printf("clip_ragged_asan: ok\n");
    return 0;
}
