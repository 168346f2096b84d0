"""Clip mode (dn_clip_process: N hops of B streams per call) beside the hop-by-hop stream, in one run on one GPU.

Rows: a 3 s clip (N = 93 hops at 16 kHz / n_fft 1024 / 80 mels) for 1, 8, 64 and 256 streams, a 30 s clip (N = 937) for 1 and 8, one row
at 48 kHz / n_fft 1536 / 64 mels and one at 16 kHz / n_fft 512 / 64 mels; then the two chain schedules of n_fft 1024 (a wavefront per
column, a wavefront per frame) over 256 .. 24,000 frames a call, which is what sets the library's automatic choice.  Baselines, timed in the
same run and alternating with the clip call: DenoiserStream.push over the same hops (one dn_stream_step launch a hop) and, at 256 streams,
PipelinedStream.push_group in groups of four hops (whole groups only: 92 of the 93 hops).  --warmup untimed rounds, then the median of --reps
rounds, each timed with events on the current stream.  One JSON line per row, then a table.

    python tools/clip_time.py [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="the 3 s rows at 1 and 8 streams only")
    args = ap.parse_args()
    from audio_denoising_amd._lib import DN_CLIP_GL_PER_COLUMN, DN_CLIP_GL_PER_STREAM
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser, DenoiserStream, PipelinedStream
    from oracle import model_ref, pipeline_ref
    dev = torch.device("cuda:0")
    sd = model_ref.unflatten_weights(np.fromfile(os.path.join(REPO, "tests", "golden", "weights_dari_tult.bin"), dtype=np.float32))
    geos = {"S": pipeline_ref.PARAMS_S, "R1": pipeline_ref.PARAMS_R1, "L16": pipeline_ref.Params(16000, 512, 256, 64)}
    denoisers = {}

    def denoiser(tag):
        if tag not in denoisers:
            p = geos[tag]
            m = GRUUNet2(p.num_compressed_bins, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
            m.load_state_dict(sd)
            denoisers[tag] = Denoiser(m.eval().to(dev), p.sample_rate, p.n_fft, p.hop, p.n_mels)
        return denoisers[tag]

    def timed(fns):
        """the callables of `fns` take turns: -> the median time of each in ms"""
        for _ in range(args.warmup):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
        runs = [[] for _ in fns]
        for _ in range(args.reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                runs[k].append(e0.elapsed_time(e1))
        return [float(np.median(r)) for r in runs]

    def clip_fn(dn, B, N, gl=0):
        g = torch.Generator().manual_seed(B * 1000 + N)
        hops = (0.1 * torch.randn(B, N * dn.hop, generator=g)).to(dev)
        ring = (0.1 * torch.randn(B, dn.n_fft, generator=g)).to(dev)
        ola, hx = torch.zeros(B, dn.n_fft, device=dev), dn.init_hx(B)
        return hops, lambda: dn._clip(hops, ring, ola, hx, None, 1, 0, frame_cap=1 << 22, gl=gl)

    rows = []

    def emit(r):
        print(json.dumps(r), flush=True)
        rows.append(r)

    clips = [("S", 1, 93), ("S", 8, 93)] if args.quick else \
        [("S", 1, 93), ("S", 8, 93), ("S", 64, 93), ("S", 256, 93), ("S", 1, 937), ("S", 8, 937), ("R1", 8, 93), ("L16", 8, 93)]
    for tag, B, N in clips:
        dn = denoiser(tag)
        hops, clip = clip_fn(dn, B, N)
        stream = DenoiserStream(dn, B, seed=1)
        stream.push(hops[:, :dn.hop])                    # (primes the ring)
        fns = [clip, lambda: stream.push(hops)]
        if B == 256 and dn.n_fft == 1024:
            pipe = PipelinedStream(dn, B, seed=1)
            pipe.set_group(4)
            groups = hops[:, :(N // 4) * 4 * dn.hop].reshape(B, N // 4, 4, dn.hop).permute(1, 2, 0, 3).contiguous()
            outs = torch.empty_like(groups)

            def grouped():
                for k in range(groups.shape[0]):
                    pipe.push_group_(groups[k], outs[k], check_weights=False)
            fns.append(grouped)
        t = timed(fns)
        r = dict(row="clip", geometry=tag, n_fft=dn.n_fft, streams=B, hops=N, frames=B * N, clip_ms=round(t[0], 3), push_loop_ms=round(t[1], 3),
                 push_over_clip=round(t[1] / t[0], 2), clip_us_per_frame=round(1e3 * t[0] / (B * N), 2))
        if len(t) > 2:
            r["push_group4_ms"] = round(t[2], 3)
            r["push_group4_hops"] = (N // 4) * 4
        emit(r)
        del stream, clip, fns
        torch.cuda.empty_cache()
    if not args.quick:
        dn = denoiser("S")
        for B, N in ((8, 32), (8, 128), (64, 64), (250, 96)):
            _, col = clip_fn(dn, B, N, DN_CLIP_GL_PER_COLUMN)
            _, per = clip_fn(dn, B, N, DN_CLIP_GL_PER_STREAM)
            t = timed([col, per])
            emit(dict(row="chains", geometry="S", n_fft=1024, streams=B, hops=N, frames=B * N, per_column_ms=round(t[0], 3), per_stream_ms=round(t[1], 3),
                      column_over_stream=round(t[0] / t[1], 3)))
    print(f"\n{'geometry':>8} {'streams':>7} {'hops':>5} {'frames':>7} {'clip ms':>10} {'push loop ms':>13} {'loop / clip':>11} {'groups of 4 ms':>15}"
          f"   (median of {args.reps} alternating rounds)")
    for r in rows:
        if r["row"] == "clip":
            g4 = f"{r['push_group4_ms']:>15.3f}" if "push_group4_ms" in r else f"{'':>15}"
            print(f"{r['geometry']:>8} {r['streams']:>7} {r['hops']:>5} {r['frames']:>7} {r['clip_ms']:>10.3f} {r['push_loop_ms']:>13.3f} {r['push_over_clip']:>11.2f} {g4}")
    chains = [r for r in rows if r["row"] == "chains"]
    if chains:
        print(f"\n{'frames':>7} {'streams':>7} {'hops':>5} {'per column ms':>14} {'per stream ms':>14} {'column / stream':>16}   (n_fft 1024 chain schedules)")
        for r in chains:
            print(f"{r['frames']:>7} {r['streams']:>7} {r['hops']:>5} {r['per_column_ms']:>14.3f} {r['per_stream_ms']:>14.3f} {r['column_over_stream']:>16.3f}")


if __name__ == "__main__":
    main()
