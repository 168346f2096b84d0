// dn_dispatch.hpp -- which instantiation a launch takes, written once (host side; included by the kernel units, not by the C ABI layer).
// A kernel is built per transform size (n_fft 512, 1024, 1536) and often per model format (fp32 / bf16 weights, the usual C of the size / any C) and per
// mode (streaming, input phases).  Each helper turns one run-time value into a compile-time one and hands it to a callable as a
// std::integral_constant / std::bool_constant; the callable -- a generic lambda -- names the kernel once, with its grid, block and arguments:
//
//   with_nfft(d.n_fft, [&](auto n) { hipLaunchKernelGGL(some_kernel<decltype(n)::value>, grid, block, 0, st, ...); });
//
// (decltype(n)::value and not n.value: an unevaluated use, so a nested lambda reads an outer constant without capturing it.)
#pragma once
#include <type_traits>

namespace dn {

template <int N> using Size = std::integral_constant<int, N>;

// the compressed bin count C of the plan's usual mel count (80 mels at n_fft 1024, 64 at 512 and 1536): the one the model kernels unroll for
constexpr int usual_c(int n_fft) { return n_fft == 1024 ? 5 : 4; }

// run-time n_fft -> Size<1536> / Size<512> / Size<1024> (every other value is 1024's: dn_plan_create admits these three)
template <class F> void with_nfft(int n_fft, F&& f) {
    if (n_fft == 1536) f(Size<1536>{});
    else if (n_fft == 512) f(Size<512>{});
    else f(Size<1024>{});
}

// run-time bool -> std::true_type / std::false_type (streaming, input phases, bf16, ...)
template <class F> void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <class F> void with_bool(bool b1, bool b2, F&& f) {          // two at once: f(c1, c2)
    with_bool(b1, [&](auto c1) { with_bool(b2, [&](auto c2) { f(c1, c2); }); });
}
// the same for a flag that only the units built with ON can raise: the others instantiate nothing for it
template <bool ON, class F> void with_bool_if(bool b, F&& f) {
    if constexpr (ON) with_bool(b, f);
    else f(std::false_type{});
}

// (bf16, C) -> (BF16, CT): CT = the usual C of the size as a constant, or 0 = any C (run-time lengths in the model)
template <int NFFT, class F> void with_model(bool bf16, int C, F&& f) {
    constexpr int kUsual = usual_c(NFFT);
    with_bool(bf16, [&](auto bf) {
        if (C == kUsual) f(bf, Size<kUsual>{});
        else f(bf, Size<0>{});
    });
}

}  // namespace dn
