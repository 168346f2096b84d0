"""Hop time at n_fft 512 beside n_fft 1024, both at 16 kHz / 64 mels, in one run on one GPU.

Per size: the unpipelined hop (Denoiser.process_frame_, batch 256), the one-hop pipe (HopPipeline at depth 1, batch 256, its default head
start) and a session push (dn_sessions_push, DN_SESS_ONE_LAUNCH) of 256 and of 1,024 slots scattered over a pool of --capacity.  --warmup
untimed steps, then the median of --reps runs of --steps steps each (reps x steps >= 200 timed steps), timed with events on the current
stream.  One JSON line per size, then a table.

    python tools/nfft512_time.py [--steps 50] [--reps 5] [--warmup 20]
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--n", type=int, nargs="+", default=[256, 1024])
    args = ap.parse_args()
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd._lib import DN_SESS_ONE_LAUNCH
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser, HopPipeline
    from oracle import model_ref, pipeline_ref
    dev = torch.device("cuda:0")
    sd = model_ref.unflatten_weights(np.fromfile(os.path.join(REPO, "tests", "golden", "weights_dari_tult.bin"), dtype=np.float32))
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
        return float(np.median(runs))

    rows = []
    for n_fft in (512, 1024):
        p = pipeline_ref.Params(16000, n_fft, n_fft // 2, 64)
        m = GRUUNet2(p.num_compressed_bins, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
        m.load_state_dict(sd)
        dn = Denoiser(m.eval().to(dev), p.sample_rate, p.n_fft, p.hop, p.n_mels)
        lib, B = dn.lib, args.batch
        g = torch.Generator().manual_seed(n_fft)
        frames = (0.1 * torch.randn(B, p.n_fft, generator=g)).to(dev)
        out, hx = torch.empty(B, p.n_fft, device=dev), dn.init_hx(B)
        r = dict(n_fft=n_fft, n_mels=p.n_mels, batch=B, steps=args.steps * args.reps)
        r["hop_us"] = round(timed(lambda: dn.process_frame_(frames, hx, out, seed=1, stream_id0=0)), 1)
        pipe = HopPipeline(dn, B)
        r["pipe_us"] = round(timed(lambda: pipe.submit(frames, hx, out, seed=1, stream_id0=0, check_weights=False)), 1)
        pipe.flush()
        pool = SessionPool(dn, args.capacity, seed=1)
        for _ in range(args.capacity):               # (one small launch a slot, outside the timed region)
            pool.open()
        pool.set_schedule(DN_SESS_ONE_LAUNCH)
        rng = np.random.default_rng(1)
        for n in args.n:
            ids = rng.choice(args.capacity, n, replace=False).astype(np.int32)          # scattered over the pool, in no particular order
            hops = (0.1 * torch.randn(n, p.hop, generator=g)).to(dev)
            o = torch.empty(n, p.hop, device=dev)
            ip = ids.ctypes.data_as(C.c_void_p)

            def push():
                lib.check(lib.dn_sessions_push(pool.handle, ip, n, hops.data_ptr(), 0, o.data_ptr(), 0, None, 1, dn.n_iter, dn.momentum, st))
            r[f"sess{n}_us"] = round(timed(push), 1)             # (the warm-up primes the listed slots)
        torch.cuda.synchronize()
        print(json.dumps(r), flush=True)
        rows.append(r)
    keys = ["hop_us", "pipe_us"] + [f"sess{n}_us" for n in args.n]
    print(f"{'n_fft':>6} " + " ".join(f"{k:>12}" for k in keys) + f"   (us per step, batch {args.batch}, 64 mels, median of {args.reps} x {args.steps} steps)")
    for r in rows:
        print(f"{r['n_fft']:>6} " + " ".join(f"{r[k]:>12.1f}" for k in keys))
    print(f"{'ratio':>6} " + " ".join(f"{rows[0][k] / rows[1][k]:>12.3f}" for k in keys) + "   (512 / 1024)")


if __name__ == "__main__":
    main()
