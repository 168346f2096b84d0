// TEST INFRASTRUCTURE ONLY -- the host layer (csrc/dn_api*.hip) under AddressSanitizer / UBSan / LeakSanitizer with resource creation failing at
// every point in turn.  tests/test_emu_host_faults.py compiles this file and the five dn_api*.hip units as host C++ against the emulation header
// (tests/emu/hip/hip_runtime.h) with -fsanitize=address,undefined and links the kernel launchers from the ordinary libdn_emu.so.
//
// One fixed scenario runs with the n-th resource-creating call (hipMalloc, hipHostMalloc, stream and event creation) failing, n = 1, 2, ... until
// it completes without reaching an n-th such call.  Every call must return DN_OK, or DN_ERR_HIP with a message; a failed call is repeated (the
// injection fires once) and must then succeed: a failure leaves its handle usable.  Whatever is held is destroyed at the end of each round, models
// and plans first (the pipes and pools hold their own references), so at exit LeakSanitizer sees every leak.
//   usage: host_faults WEIGHTS.bin      prints "injection points visited: N", exit status 0; anything else is a failure
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/dn_denoise.h"

namespace {

constexpr int B = 2, CAP = 3, N_ITER = 1;
constexpr float MOM = 0.99f;
int g_round = 0;

[[noreturn]] void die(const char* what, int rc) {
    fprintf(stderr, "host_faults: round %d: %s returned %d (%s)\n", g_round, what, rc, dn_last_error());
    exit(1);
}

// a call of the scenario: DN_OK, or the injected failure reported as DN_ERR_HIP with a message and DN_OK on the repeat
template <typename F>
void step(const char* what, F call) {
    int rc = call();
    if (rc == DN_OK) return;
    if (rc != DN_ERR_HIP || dn_last_error()[0] == 0 || dn_emu::fail_countdown() != 0) die(what, rc);      // (countdown 0: the injection has fired)
    rc = call();
    if (rc != DN_OK) die(what, rc);
}

struct Held {
    dn_model *m1 = nullptr, *m2 = nullptr;
    dn_dsp *d1024 = nullptr, *d512 = nullptr;
    dn_pipe *frame_pipe = nullptr, *stream_pipe = nullptr;
    dn_sessions* pool = nullptr;
    ~Held() {
        dn_model_destroy(m1); dn_model_destroy(m2);
        dn_dsp_destroy(d1024); dn_dsp_destroy(d512);
        dn_pipe_destroy(frame_pipe); dn_pipe_destroy(stream_pipe);
        dn_sessions_destroy(pool);
    }
};

void scenario(const std::vector<float>& w) {
    Held h;
    const dn_model_cfg mc{5, 1, 4, 17, 3, 2, 1, 6};
    const dn_dsp_cfg c1024{16000, 1024, 512, 80}, c512{16000, 512, 256, 16};
    step("dn_model_create", [&] { return dn_model_create(w.data(), w.size(), &mc, &h.m1); });
    step("dn_dsp_create(1024)", [&] { return dn_dsp_create(&c1024, nullptr, nullptr, nullptr, &h.d1024); });
    step("dn_dsp_create(512)", [&] { return dn_dsp_create(&c512, nullptr, nullptr, nullptr, &h.d512); });
    step("dn_pipe_create", [&] { return dn_pipe_create(h.m1, h.d512, B, DN_PHASE_FROM_INPUT, &h.frame_pipe); });
    step("dn_pipe_stream_create", [&] { return dn_pipe_stream_create(h.m1, h.d1024, B, 0, &h.stream_pipe); });
    step("dn_pipe_set_depth(2)", [&] { return dn_pipe_set_depth(h.stream_pipe, 2); });
    step("dn_pipe_set_depth(1)", [&] { return dn_pipe_set_depth(h.stream_pipe, 1); });
    step("dn_pipe_set_group(2)", [&] { return dn_pipe_set_group(h.stream_pipe, 2); });
    step("dn_pipe_set_group(0)", [&] { return dn_pipe_set_group(h.stream_pipe, 0); });
    step("dn_model_create(second)", [&] { return dn_model_create(w.data(), w.size(), &mc, &h.m2); });
    step("dn_pipe_set_model", [&] { return dn_pipe_set_model(h.stream_pipe, h.m2); });
    std::vector<float> hop_in((size_t)B * c1024.hop, 0.01f), hop_out((size_t)B * c1024.hop);
    for (int i = 0; i < 2; ++i) {
        uint64_t ticket = 0;
        step("dn_pipe_stream_push_host", [&] {
            return dn_pipe_stream_push_host(h.stream_pipe, hop_in.data(), 0, hop_out.data(), 0, 7, 0, N_ITER, MOM, DN_HOST_STAGED, nullptr, &ticket);
        });
        step("dn_pipe_stream_host_wait", [&] { return dn_pipe_stream_host_wait(h.stream_pipe, ticket); });
    }
    step("dn_sessions_create", [&] { return dn_sessions_create(h.m1, h.d1024, CAP, 0, &h.pool); });
    const int32_t ids[2] = {2, 0}, ids_back[2] = {1, 2};
    const size_t stride = dn_sessions_record_bytes(h.pool);
    std::vector<uint4> records(2 * stride / sizeof(uint4));       // (16-byte aligned)
    step("dn_sessions_open", [&] { return dn_sessions_open(h.pool, ids, 2, nullptr, nullptr); });
    step("dn_sessions_export", [&] { return dn_sessions_export(h.pool, ids, 2, records.data(), nullptr); });
    step("dn_sessions_import", [&] { return dn_sessions_import(h.pool, ids_back, 2, records.data(), nullptr, nullptr); });
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: host_faults WEIGHTS.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> w;
    float buf[4096];
    for (size_t n; (n = fread(buf, sizeof(float), 4096, f)) > 0;) w.insert(w.end(), buf, buf + n);
    fclose(f);
    for (g_round = 1; g_round < 100000; ++g_round) {
        dn_emu::fail_countdown() = g_round;
        scenario(w);
        if (dn_emu::fail_countdown() > 0) {          // the scenario made fewer than g_round such calls: every point has been visited
            printf("injection points visited: %d\n", g_round - 1);
            return 0;
        }
    }
    fprintf(stderr, "host_faults: the scenario never completed without an injected failure\n");
    return 1;
}
