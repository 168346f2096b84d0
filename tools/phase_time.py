"""Input-phase mode (Denoiser(phase="input"); DN_PHASE_FROM_INPUT) beside the default random phases, timed in one run on one GPU:
n_fft 1024, 80 mels, 16 kHz, 256 and 1,024 streams.

Rows: the unpipelined hop (dn_stream_step: one launch, no added latency) at n_iter 0, 8 and 32 from input phases and 32 from random ones; the
one-hop pipe (dn_pipe_stream_push) and hop groups of four (dn_pipe_stream_push_group) at n_iter 8 and 32 in both modes.  Every row is timed with
events on the current stream around at least --seconds of work, after --warmup untimed steps; `enqueue` is the host's time per hop to issue a
burst of 16 calls onto an idle queue (no back-pressure: a row whose enqueue time is not well under its GPU time is bound by the host, not by the
kernels).  One JSON line per row, then a table.

    python tools/phase_time.py [--seconds 0.5] [--warmup 20] [--streams 256 1024]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--streams", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser, PipelinedStream
    from oracle import model_ref, pipeline_ref
    dev = torch.device("cuda:0")
    p = pipeline_ref.PARAMS_S
    sd = model_ref.unflatten_weights(np.fromfile(os.path.join(REPO, "tests", "golden", "weights_dari_tult.bin"), dtype=np.float32))
    model = GRUUNet2(p.num_compressed_bins, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
    model.load_state_dict(sd)
    model = model.eval().to(dev)

    def timed(step, hops_per_step):
        """-> (GPU us per hop, host enqueue us per hop, hops timed)"""
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            step()
        e1.record()
        e1.synchronize()
        n = max(50, int(np.ceil(1.2 * args.seconds * 1e3 / max(e0.elapsed_time(e1) / 50, 1e-3))))
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms >= 1e3 * args.seconds, ms
        bursts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(16):
                step()
            bursts.append((time.perf_counter() - t0) / 16)
        torch.cuda.synchronize()
        return 1e3 * ms / (n * hops_per_step), 1e6 * float(np.median(bursts)) / hops_per_step, n * hops_per_step

    rows = []

    def emit(**r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    for B in args.streams:
        g = torch.Generator().manual_seed(B)
        hops = (0.1 * torch.randn(4, B, p.hop, generator=g)).to(dev)
        for path, phase, n_iter in [("stream_step", "input", 0), ("stream_step", "input", 8), ("stream_step", "input", 32), ("stream_step", "random", 32)] + \
                [(path, phase, it) for path in ("pipe", "group4") for it in (8, 32) for phase in ("input", "random")]:
            dn = Denoiser(model, p.sample_rate, p.n_fft, p.hop, p.n_mels, n_iter=n_iter, phase=phase)
            if path == "stream_step":
                ring = (0.1 * torch.randn(B, p.n_fft, generator=g)).to(dev)
                ola, hx, out = torch.zeros(B, p.n_fft, device=dev), dn.init_hx(B), torch.empty(B, p.hop, device=dev)
                ws, mh, st = dn._workspace(B), model._native(dev), C.c_void_p(torch.cuda.current_stream().cuda_stream)
                ptrs = (hops[0].data_ptr(), ring.data_ptr(), ola.data_ptr(), hx.data_ptr(), out.data_ptr(), ws.data_ptr())
                fl, lib, plan = dn._flags(), dn.lib, dn.plan.handle

                def step():
                    lib.check(lib.dn_stream_step(mh, plan, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], None, 1, 0, n_iter, dn.momentum, ptrs[5], B, fl, st))
                per = 1
            else:
                pipe = PipelinedStream(dn, B, seed=1)
                if path == "group4":
                    pipe.set_group(4)
                    outs = torch.empty_like(hops)

                    def step():
                        pipe.push_group_(hops, outs, check_weights=False)
                    per = 4
                else:
                    out = torch.empty(B, p.hop, device=dev)

                    def step():
                        pipe.push_(hops[0], out, check_weights=False)
                    per = 1
            us, enq, n = timed(step, per)
            emit(streams=B, path=path, phase=phase, n_iter=n_iter, us_per_hop=round(us, 2), enqueue_us_per_hop=round(enq, 2), hops_timed=n,
                 frames_per_s=round(B * 1e6 / us))
            torch.cuda.synchronize()
            del dn, step
    print(f"\n{'streams':>7} {'path':>12} {'phase':>7} {'n_iter':>6} {'us / hop':>10} {'enqueue us':>11} {'frames / s':>12}   (>= {args.seconds} s of work per row)")
    for r in rows:
        print(f"{r['streams']:>7} {r['path']:>12} {r['phase']:>7} {r['n_iter']:>6} {r['us_per_hop']:>10.2f} {r['enqueue_us_per_hop']:>11.2f} {r['frames_per_s']:>12}")


if __name__ == "__main__":
    main()
