#!/usr/bin/env python3
"""Every ratio behind the constants R_HX, R_HX_NEAR and R_WAVE of the long-stream tests (tests/long_cases.py; tests/test_emu_long_stream.py,
tests/test_gpu_long_stream.py): runs dn_stream_step over the conversation on one tier and prints, per checkpoint, the kernel's hx error against
float64, the fp32 CPU oracle's own error e_ref, its running maximum E_k and the ratios; the two drift statistics; per window the waveform
errors, the yardstick e_ref_wave and the ratios; the int16 difference counts; per family the worst ratio and the factor the rule gives (10 x
the worst ratio, rounded up to a power of two: model_cases.guard_factor).  On the GPU it also reports whether dn_stft_mel_log1p,
dn_cell_forward and dn_synthesis composed give dn_process_frame's bits.

    python tools/long_stream_margins.py --tier emu        host emulation of the kernel sources, the 32-hop excerpt (no GPU)
    python tools/long_stream_margins.py --tier gpu        the built library on cuda:0, the whole runs

profiles/long_stream_margins.txt is the output of both.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (REPO, os.path.join(REPO, "tests"), os.path.join(REPO, "tests", "emu")):
    sys.path.insert(0, d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tier", choices=("emu", "gpu"), required=True)
    tier = ap.parse_args().tier
    import long_cases as lc
    import model_cases as mc
    rep = []
    print(f"# tier {tier}: hx max-abs error against float64 over the reference streams; e_ref = the fp32 CPU oracle's own at that frame, E_k its running "
          f"maximum, E_near its maximum over the last {lc.NEAR} frames")
    if tier == "emu":
        import emu
        import test_emu_long_stream as te
        run = lc.Runner(emu.load())
        for label in te.WINDOWS:
            te.excerpt(run, label, rep)
    else:
        import torch
        from audio_denoising_amd import _lib
        run = lc.Runner(_lib.get_lib(), torch.device("cuda:0"))
        for n_fft in lc.N_FFTS:
            d, F = lc.load(n_fft), lc.HOPS[n_fft]
            res = run.steps(run.plan(n_fft), lc.signal32(n_fft), 0, F, keep=set(d["cps"].tolist()))
            errs = lc.check_hx(res, d, tier, f"n_fft {n_fft}", rep)
            e_ref = d["e_ref"].max(axis=1)[d["cps"]]
            rep.append(("drift", f"drift n_fft {n_fft}: worst error second half / first half {lc.drift(errs, d['cps'], F):.3f}; the fp32 oracle's "
                        f"{lc.drift(e_ref, d['cps'], F):.3f}; error at the last frame {errs[-1]:.3e}, worst {max(errs):.3e}",
                        lc.drift(errs, d["cps"], F) / lc.drift(e_ref, d["cps"], F)))
            for i, f0 in enumerate(d["win_f0"]):
                y64 = lc.window64(n_fft, int(f0), d["win_hx64"][i], d["win_ola64"][i])[0]
                y = res["out"][:lc.B_REF, f0:f0 + lc.WINDOW_HOPS]
                what = f"n_fft {n_fft} {str(d['win_label'][i])!r} at frame {f0}"
                lc.check_window(y, y64, float(d["win_e_rel"][i]), float(d["win_e_abs"][i]), tier, what, rep)
                n = int((lc.s16_of_f32(y) != lc.s16_of(y64)).sum())
                ref = int((d["win_s16_ref32"][i] != lc.s16_of(y64)).sum())
                rep.append(("int16", f"int16 {what}: {n} of {y64.size} samples differ from the float64 truncation (the fp32 oracle: {ref})", 0.0))
            (hx_a, hx_b), (w_a, w_b) = lc.composed(run, n_fft)
            c = dict(hx=bool(np.array_equal(hx_a, hx_b)), wave=bool(np.array_equal(w_a, w_b)))
            rep.append(("composed", f"composed n_fft {n_fft}: dn_stft_mel_log1p -> dn_cell_forward -> dn_synthesis against dn_process_frame, bit for bit: "
                        f"hx {c['hx']}, waveform {c['wave']}", 0.0))
    for _, line, _ in rep:
        if line:
            print(line)
    print(f"# tier {tier}: per family -- worst ratio, rule = 10 x worst ratio rounded up to a power of two, R in use")
    for fam, used in (("hx", lc.R_HX), ("hx_near", lc.R_HX_NEAR), ("wave", lc.R_WAVE)):
        worst = max(r for f, _, r in rep if f == fam)
        print(f"{fam:8s} cases {sum(f == fam for f, _, _ in rep):4d}  worst ratio {worst:7.3f}  rule {mc.guard_factor(worst):g}  in use {used[tier]:g}")
    if tier == "gpu":
        print(f"drift    worst (kernel's statistic / the oracle's) {max(r for f, _, r in rep if f == 'drift'):.3f}  allowed {lc.DRIFT}")
    run.close()


if __name__ == "__main__":
    main()
