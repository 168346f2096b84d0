"""Time of the any-length Griffin-Lim (dn_griffinlim_general) in its two forms, beside the 3-column chain (dn_griffinlim), on one GPU.

Per n_fft, 32 iterations, injected phases:
    T = 3,  batch 256: dn_griffinlim  |  WHOLE  |  STEPS      (WHOLE / dn_griffinlim is the figure with an expectation: <= 1.5)
    T = 8,  batch 256: WHOLE  |  STEPS
    T = 94, batch 1 and 64: STEPS                              (a 3 s clip at 16 kHz and n_fft 1024)
--warmup untimed calls, then the median of --reps runs of --steps calls each, timed with events on the current stream; every call is enqueued
back to back (nothing synchronises inside a run).  One JSON line per n_fft, then a table.

    python tools/glg_time.py [--steps 200] [--reps 5] [--warmup 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--n-iter", type=int, default=32)
    args = ap.parse_args()
    from audio_denoising_amd import _lib
    from audio_denoising_amd.transforms import DspPlan
    dev = torch.device("cuda:0")
    lib = _lib.get_lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record()
            e1.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / args.steps)
        return round(float(np.median(runs)), 1), round(float(min(runs)), 1), round(float(max(runs)), 1)

    rows = []
    for n_fft in (512, 1024, 1536):
        plan = DspPlan(dev, 0, n_fft, n_fft // 2, 0)
        K, hop = n_fft // 2 + 1, n_fft // 2
        g = torch.Generator().manual_seed(n_fft)

        def general(B, T, flags):
            mag = (torch.rand(B, T, K, generator=g) * 46.0).to(dev)
            init = torch.rand(B, T, K, 2, generator=g).to(dev)
            wave = torch.empty(B, hop * (T - 1), device=dev)
            ws = torch.empty(int(lib.dn_griffinlim_general_workspace_bytes(plan.handle, B, T)), dtype=torch.uint8, device=dev)

            def fn():
                lib.check(lib.dn_griffinlim_general(plan.handle, mag.data_ptr(), init.data_ptr(), 0, 0, wave.data_ptr(), ws.data_ptr(), B, T, args.n_iter,
                                                    0.99, flags, st))
            res = timed(fn)
            assert torch.isfinite(wave).all()
            return res

        def hop_chain(B):
            mag = (torch.rand(B, 3, K, generator=g) * 46.0).to(dev)
            init = torch.rand(B, 3, K, 2, generator=g).to(dev)
            wave = torch.empty(B, n_fft, device=dev)

            def fn():
                lib.check(lib.dn_griffinlim(plan.handle, mag.data_ptr(), init.data_ptr(), 0, 0, None, wave.data_ptr(), B, args.n_iter, 0.99, st))
            return timed(fn)

        B = args.batch
        r = dict(n_fft=n_fft, batch=B, n_iter=args.n_iter, calls=args.steps * args.reps, unit="us per call: median, min, max of the runs")
        r["hop_chain_T3"] = hop_chain(B)
        r["whole_T3"] = general(B, 3, _lib.DN_GLG_WHOLE)
        r["steps_T3"] = general(B, 3, _lib.DN_GLG_STEPS)
        r["whole_T8"] = general(B, 8, _lib.DN_GLG_WHOLE)
        r["steps_T8"] = general(B, 8, _lib.DN_GLG_STEPS)
        r["steps_T94_B1"] = general(1, 94, _lib.DN_GLG_STEPS)
        r["steps_T94_B64"] = general(64, 94, _lib.DN_GLG_STEPS)
        r["whole_T3_over_hop_chain"] = round(r["whole_T3"][0] / r["hop_chain_T3"][0], 3)
        r["steps_T8_over_whole_T8"] = round(r["steps_T8"][0] / r["whole_T8"][0], 3)
        print(json.dumps(r), flush=True)
        rows.append(r)
    keys = ["hop_chain_T3", "whole_T3", "steps_T3", "whole_T8", "steps_T8", "steps_T94_B1", "steps_T94_B64"]
    print(f"{'n_fft':>6} " + " ".join(f"{k:>14}" for k in keys) + f"   (median us per call, {args.n_iter} iterations, batch {args.batch} unless named; {args.reps} x {args.steps} calls)")
    for r in rows:
        print(f"{r['n_fft']:>6} " + " ".join(f"{r[k][0]:>14.1f}" for k in keys) + f"   WHOLE / dn_griffinlim at T = 3: {r['whole_T3_over_hop_chain']:.3f}; STEPS / WHOLE at T = 8: {r['steps_T8_over_whole_T8']:.3f}")


if __name__ == "__main__":
    main()
