// TEST INFRASTRUCTURE ONLY -- the rate bank's two calls (dn_ratebank_ingest, dn_ratebank_emit) under AddressSanitizer / UBSan on exactly sized heap
// buffers: a row's vector loads near the end of its chunk, the paired stores at the end of its outputs and the state row are where an
// out-of-range access would come from.  tests/test_emu_ratebank_asan.py compiles this file, the host units (dn_api*.hip) and the two resampler
// units (dn_resample.hip, dn_ratebank.hip) as host C++ against the emulation header with -fsanitize=address,undefined and links what else the
// host layer refers to from the ordinary libdn_emu.so.  Nothing is preloaded.
//
// Bank: a 16 kHz plan of hop 256 with 8, 12 and 48 kHz sessions.  float32 and int16, every buffer a heap block of exactly the size the header
// states -- (n - 1) stride + the LAST row's chunk, the last row being the shortest chunk (8 kHz), stride the longest listed one; states of exactly
// capacity x stride floats -- for a mixed list (48 kHz, the plan's rate, 12 kHz, 8 kHz) pushed twice, and for a one-row list.
// Every float out must be finite.
//   usage: ratebank_asan      prints "ratebank_asan: ok", exit status 0; anything else is a failure
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "../../include/dn_denoise.h"

namespace {

constexpr int kHop = 256, kCap = 5;

[[noreturn]] void die(const char* what, int rc) {
    fprintf(stderr, "ratebank_asan: %s (%d: %s)\n", what, rc, dn_last_error());
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
void run(dn_ratebank* b, const std::vector<int32_t>& slots, const std::vector<int32_t>& ridx) {
    constexpr int s16 = sizeof(SAMPLE) == 2;
    const int n = (int)slots.size();
    std::vector<int> cin(n, kHop), cout(n, kHop);
    int xs = 0, ys = 0;
    for (int i = 0; i < n; ++i) {
        if (ridx[i] >= 0) {
            int32_t ci, co;
            const int rc = dn_ratebank_geometry(b, ridx[i], &ci, &co, nullptr, nullptr, nullptr, nullptr);
            if (rc != DN_OK) die("dn_ratebank_geometry", rc);
            cin[i] = ci; cout[i] = co;
        }
        xs = cin[i] > xs ? cin[i] : xs;
        ys = cout[i] > ys ? cout[i] : ys;
    }
    auto state_in = exact<float>((size_t)kCap * dn_ratebank_state_stride(b, DN_RATEBANK_IN));
    auto state_out = exact<float>((size_t)kCap * dn_ratebank_state_stride(b, DN_RATEBANK_OUT));
    const size_t nx = (size_t)(n - 1) * xs + cin[n - 1], ny = (size_t)(n - 1) * ys + cout[n - 1], nh = (size_t)n * kHop;
    for (int push = 0; push < 2; ++push) {
        auto x = exact<SAMPLE>(nx), y = exact<SAMPLE>(ny);
        auto hop = exact<float>(nh);
        for (size_t k = 0; k < nx; ++k) x[k] = sample<SAMPLE>(k + 7 * push);
        int rc = dn_ratebank_ingest(b, slots.data(), ridx.data(), n, kCap, state_in.get(), x.get(), s16, xs, hop.get(), nullptr);
        if (rc != DN_OK) die("dn_ratebank_ingest", rc);
        for (size_t k = 0; k < nh; ++k)
            if (!isfinite(hop[k])) die("a sample of hop_in is not finite", (int)k);
        rc = dn_ratebank_emit(b, slots.data(), ridx.data(), n, kCap, state_out.get(), hop.get(), y.get(), s16, ys, nullptr);
        if (rc != DN_OK) die("dn_ratebank_emit", rc);
        for (size_t k = 0; k < ny; ++k)
            if (!s16 && !isfinite((float)y[k])) die("a sample out is not finite", (int)k);
    }
}

}  // namespace

int main() {
    dn_ratebank_cfg cfg{};
    cfg.plan_rate = 16000; cfg.hop = kHop; cfg.n_rates = 3; cfg.lowpass_filter_width = 6; cfg.rolloff = 0.99;
    cfg.rates[0] = 8000; cfg.rates[1] = 12000; cfg.rates[2] = 48000;
    dn_ratebank* b = nullptr;
    const int rc = dn_ratebank_create(&cfg, &b);
    if (rc != DN_OK) die("dn_ratebank_create", rc);
    const std::vector<int32_t> slots{4, 0, 2, 3}, ridx{2, -1, 1, 0};          // 48 kHz, the plan's rate, 12 kHz, and last the shortest: 8 kHz
    run<float>(b, slots, ridx);
    run<int16_t>(b, slots, ridx);
    run<float>(b, {1}, {0});
    run<int16_t>(b, {1}, {2});
    dn_ratebank_destroy(b);
    printf("ratebank_asan: ok\n");
    return 0;
}
