// TEST INFRASTRUCTURE ONLY -- the resampler's two entry points (dn_resample, dn_resample_push) under AddressSanitizer / UBSan on exactly sized heap
// buffers: the aprons of a staged tile, the last partial block of a row and the state shift are where an out-of-range access would come from.
// tests/test_emu_resample_asan.py compiles this file, the host units (dn_api*.hip) and the resampler unit (dn_resample.hip) as host C++ against the
// emulation header (tests/emu/hip/hip_runtime.h) with -fsanitize=address,undefined and links what else the host layer refers to from the ordinary
// libdn_emu.so.  Nothing is preloaded.
//
// For a small-ratio pair (48000 -> 16000) and a general one (44100 -> 48000), float32 and int16, every buffer a heap block of exactly the size the
// header states:
//   whole signal   L = 1, L = o (one block), L = H + o (one block more than the history), L = 2 KW + o + 1, and the next multiple of 4 (rows on
//                  16-byte boundaries: the wide loads and the paired stores)
//   pushes         one block, then H / o + 1 blocks (one more than the history), then one block again, on a state of exactly B x H floats
// Every float out must be finite, and the pushes followed by D blocks of zeros must give the whole-signal samples.
//   usage: resample_asan      prints "resample_asan: ok", exit status 0; anything else is a failure
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
    fprintf(stderr, "resample_asan: %s (%d: %s)\n", what, rc, dn_last_error());
    exit(1);
}

template <typename T>
std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]()); }          // a heap block of exactly n elements, zeroed

template <typename SAMPLE>
SAMPLE sample(size_t k) {
    const float v = 0.4f * sinf(0.37f * (float)k) + 0.01f * (float)(k % 5);
    return sizeof(SAMPLE) == 2 ? (SAMPLE)(v * 32767.0f) : (SAMPLE)v;
}

template <typename SAMPLE>
void run(int orig, int rate) {
    constexpr int s16 = sizeof(SAMPLE) == 2, B = 2;
    const dn_resample_cfg cfg{orig, rate, 6, 0.99};
    dn_resampler* r = nullptr;
    int rc = dn_resample_create(&cfg, nullptr, &r);
    if (rc != DN_OK) die("dn_resample_create", rc);
    int32_t o, n, width, KW, D;
    rc = dn_resample_geometry(r, &o, &n, &width, &KW, &D);
    if (rc != DN_OK) die("dn_resample_geometry", rc);
    const int H = D * o + width;
    if (dn_resample_state_bytes(r, B) != (size_t)B * H * sizeof(float)) die("dn_resample_state_bytes", 0);
    auto table = exact<float>((size_t)n * KW);
    if ((rc = dn_resample_get_kernel(r, table.get())) != DN_OK) die("dn_resample_get_kernel", rc);

    for (const long L : {1L, (long)o, (long)(H + o), (long)(2 * KW + o + 1), (long)((2 * KW + o + 4) / 4 * 4)}) {
        const long Ly = (long)dn_resample_out_len(r, L);
        auto x = exact<SAMPLE>((size_t)B * L), y = exact<SAMPLE>((size_t)B * Ly);
        for (size_t k = 0; k < (size_t)B * L; ++k) x[k] = sample<SAMPLE>(k);
        rc = dn_resample(r, x.get(), s16, y.get(), s16, B, L, L, Ly, nullptr);
        if (rc != DN_OK) die("dn_resample", rc);
        for (size_t k = 0; k < (size_t)B * Ly; ++k)
            if (!s16 && !isfinite((float)y[k])) die("a sample out is not finite", (int)k);
    }

    // pushes against the whole-signal call on the same samples
    const long hist_blocks = (H + o - 1) / o, pushes[] = {1, hist_blocks + 1, 1, D};          // (the last one: D blocks of zeros)
    long blocks = 0;
    for (int i = 0; i < 3; ++i) blocks += pushes[i];
    const long L = blocks * o, Ly = (long)dn_resample_out_len(r, L);
    auto x = exact<SAMPLE>((size_t)B * L), whole = exact<SAMPLE>((size_t)B * Ly);
    for (size_t k = 0; k < (size_t)B * L; ++k) x[k] = sample<SAMPLE>(k + 11);
    if ((rc = dn_resample(r, x.get(), s16, whole.get(), s16, B, L, L, Ly, nullptr)) != DN_OK) die("dn_resample", rc);
    auto state = exact<float>((size_t)B * H);
    std::vector<SAMPLE> got[B];
    long at = 0;
    for (int i = 0; i < 4; ++i) {
        const long lc = pushes[i] * o, ly = pushes[i] * n;
        auto chunk = exact<SAMPLE>((size_t)B * lc), out = exact<SAMPLE>((size_t)B * ly);
        if (i < 3)
            for (int b = 0; b < B; ++b) memcpy(chunk.get() + (size_t)b * lc, x.get() + (size_t)b * L + at, lc * sizeof(SAMPLE));
        rc = dn_resample_push(r, state.get(), chunk.get(), s16, out.get(), s16, B, pushes[i], lc, ly, nullptr);
        if (rc != DN_OK) die("dn_resample_push", rc);
        for (int b = 0; b < B; ++b) got[b].insert(got[b].end(), out.get() + (size_t)b * ly, out.get() + (size_t)(b + 1) * ly);
        at += lc;
    }
    for (int b = 0; b < B; ++b)
        if (memcmp(got[b].data() + (size_t)D * n, whole.get() + (size_t)b * Ly, Ly * sizeof(SAMPLE)) != 0) die("the pushes differ from the whole signal", b);
    dn_resample_destroy(r);
}

}  // namespace

int main() {
    run<float>(48000, 16000);
    run<int16_t>(48000, 16000);
    run<float>(44100, 48000);
    run<int16_t>(44100, 48000);
    printf("resample_asan: ok\n");
    return 0;
}
