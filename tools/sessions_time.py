"""Tick time of a session pool (dn_sessions_push) against dn_stream_step, n_fft 1024 (PARAMS_S).

For n listed slots scattered over a pool of --capacity (default 8,192) slots, every slot primed: one tick of the one-launch form (A), one of
the two-launch form (B), and -- the yardstick -- one dn_stream_step on a contiguous batch of the same n.  Median of --reps runs of --ticks
ticks each, timed with events on the current stream.  One JSON line per n, then a table.

    python tools/sessions_time.py [--n 256 1024 4096 8192] [--ticks 20] [--reps 5]
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
    ap.add_argument("--n", type=int, nargs="+", default=[256, 1024, 4096, 8192])
    ap.add_argument("--capacity", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from audio_denoising_amd import SessionPool
    from audio_denoising_amd._lib import DN_SESS_ONE_LAUNCH, DN_SESS_TWO_LAUNCHES
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser
    from oracle import model_ref, pipeline_ref
    dev = torch.device("cuda:0")
    p = pipeline_ref.PARAMS_S
    m = GRUUNet2(5, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
    m.load_state_dict(model_ref.unflatten_weights(np.fromfile(os.path.join(REPO, "tests", "golden", "weights_dari_tult.bin"), dtype=np.float32)))
    dn = Denoiser(m.eval().to(dev), p.sample_rate, p.n_fft, p.hop, p.n_mels)
    lib = dn.lib
    pool = SessionPool(dn, args.capacity, seed=1)
    ids_all = np.arange(args.capacity, dtype=np.int32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib.check(lib.dn_sessions_open(pool.handle, ids_all.ctypes.data_as(C.c_void_p), args.capacity, None, st))
    pool._open[:] = True
    g = torch.Generator().manual_seed(0)
    model_h = m._native(dev)

    def timed(fn):
        fn()                                         # warm
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.ticks):
                fn()
            e1.record()
            e1.synchronize()
            runs.append(e0.elapsed_time(e1) * 1e3 / args.ticks)
        return float(np.median(runs))

    rows = []
    rng = np.random.default_rng(1)
    for n in args.n:
        ids = np.sort(rng.choice(args.capacity, n, replace=False)).astype(np.int32)
        ids = ids[rng.permutation(n)]                # scattered over the pool, in no particular order
        hops = (0.1 * torch.randn(n, p.hop, generator=g)).to(dev)
        out = torch.empty(n, p.hop, device=dev)
        ip = ids.ctypes.data_as(C.c_void_p)

        def push():
            lib.check(lib.dn_sessions_push(pool.handle, ip, n, hops.data_ptr(), 0, out.data_ptr(), 0, None, 1, dn.n_iter, dn.momentum, st))
        pool.set_schedule(DN_SESS_ONE_LAUNCH)
        push()                                       # primes the listed slots
        t_a = timed(push)
        pool.set_schedule(DN_SESS_TWO_LAUNCHES)
        t_b = timed(push)
        ring = torch.zeros(n, p.n_fft, device=dev)
        ola = torch.zeros(n, p.n_fft, device=dev)
        hx = dn.init_hx(n)
        ws = dn._workspace(n)

        def step():
            lib.check(lib.dn_stream_step(model_h, dn.plan.handle, hops.data_ptr(), ring.data_ptr(), ola.data_ptr(), hx.data_ptr(), out.data_ptr(),
                                         None, 1, 0, dn.n_iter, dn.momentum, ws.data_ptr(), n, 0, st))
        t_s = timed(step)
        r = dict(n=n, capacity=args.capacity, one_launch_us=round(t_a, 1), two_launches_us=round(t_b, 1), stream_step_us=round(t_s, 1),
                 one_launch_vs_step=round(t_a / t_s, 4), two_vs_one=round(t_b / t_a, 4))
        print(json.dumps(r), flush=True)
        rows.append(r)
    print(f"{'n':>6} {'A one launch':>14} {'B two launches':>15} {'dn_stream_step':>15} {'A/step':>8} {'B/A':>7}   (us per tick)")
    for r in rows:
        print(f"{r['n']:>6} {r['one_launch_us']:>14.1f} {r['two_launches_us']:>15.1f} {r['stream_step_us']:>15.1f} {r['one_launch_vs_step']:>8.3f} "
              f"{r['two_vs_one']:>7.3f}")


if __name__ == "__main__":
    main()
