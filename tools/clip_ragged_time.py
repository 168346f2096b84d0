"""The ragged clip call (dn_clip_process_ragged: clips of different lengths in one call) beside what a caller had before it, in one run on one GPU.

Workload: 16 kHz / n_fft 1024 / 80 mels, 32 iterations; 64 and 256 clips whose lengths are drawn once from a seeded generator, uniform in 1 s to 5 s.
Per row, with the frames each form runs:
  ragged     Denoiser.clip_ragged: one call, sum n_hops frames
  loop       one dn_clip_process call with B = 1 per clip, back to back on the stream: the same frames
  padded     dn_clip_process on the clips zero-padded to the longest: B x max n_hops frames (and the streams' state ends at the wrong hop)
--warmup untimed rounds, then the median of --reps rounds in which the three take turns, each timed with events on the current stream.  One JSON
line per row, then a table.

    python tools/clip_ragged_time.py [--reps 5] [--warmup 2]

The uniform call must not pay for the lookup: tools/clip_time.py run twice on the parent's library and twice on this one (alternating, the parent's
bound through DN_LIB_PATH), each output kept in a file, then

    python tools/clip_ragged_time.py --compare PARENT_1 NEW_1 PARENT_2 NEW_2

prints every `clip` row: the parent's two runs, their spread, this build's two runs, and the move of the mean against the parent's, in percent.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def compare(paths):
    runs = []
    for p in paths:
        with open(p) as f:
            rows = [json.loads(line) for line in f if line.startswith("{")]
        runs.append({(r["geometry"], r["streams"], r["hops"]): r["clip_ms"] for r in rows if r.get("row") == "clip"})
    print(f"{'geometry':>8} {'streams':>7} {'hops':>5} {'parent 1':>9} {'parent 2':>9} {'spread %':>9} {'new 1':>9} {'new 2':>9} {'move %':>8}"
          "   (dn_clip_process, ms; spread = |parent 1 - parent 2| / mean, move = new mean / parent mean - 1)")
    for key in runs[0]:
        p1, n1, p2, n2 = (r[key] for r in runs)
        pm, nm = (p1 + p2) / 2, (n1 + n2) / 2
        print(f"{key[0]:>8} {key[1]:>7} {key[2]:>5} {p1:>9.3f} {p2:>9.3f} {100 * abs(p1 - p2) / pm:>9.2f} {n1:>9.3f} {n2:>9.3f} {100 * (nm / pm - 1):>8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--compare", nargs=4, metavar="FILE", help="four outputs of tools/clip_time.py: parent, new, parent, new")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare)
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser
    from oracle import model_ref, pipeline_ref
    dev = torch.device("cuda:0")
    sd = model_ref.unflatten_weights(np.fromfile(os.path.join(REPO, "tests", "golden", "weights_dari_tult.bin"), dtype=np.float32))
    p = pipeline_ref.PARAMS_S
    m = GRUUNet2(p.num_compressed_bins, 1, (17, 17, 17, 17), (3, 3, 3, 3), (2, 2, 2, 2), (1, 1, 1, 1))
    m.load_state_dict(sd)
    dn = Denoiser(m.eval().to(dev), p.sample_rate, p.n_fft, p.hop, p.n_mels)

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

    rows = []
    for B in (64, 256):
        g = torch.Generator().manual_seed(1000 + B)
        lengths = torch.randint(p.sample_rate, 5 * p.sample_rate + 1, (B,), generator=g).tolist()
        n_hops = [dn.clip_hops(L) for L in lengths]
        F, longest = sum(n_hops), max(n_hops)
        packed = (0.1 * torch.randn(F * dn.hop, generator=g)).to(dev)
        ring = (0.1 * torch.randn(B, dn.n_fft, generator=g)).to(dev)
        ola, hx = torch.zeros(B, dn.n_fft, device=dev), dn.init_hx(B)
        off = np.concatenate([[0], np.cumsum(n_hops)])
        each = [(packed[off[b] * dn.hop:off[b + 1] * dn.hop][None].contiguous(), ring[b:b + 1].clone(), ola[b:b + 1].clone(), hx[b:b + 1].clone()) for b in range(B)]
        padded = torch.zeros(B, longest * dn.hop, device=dev)
        for b in range(B):
            padded[b, :n_hops[b] * dn.hop] = each[b][0][0]
        pring, pola, phx = ring.clone(), ola.clone(), hx.clone()

        def ragged():
            dn.clip_ragged(packed, n_hops, ring, ola, hx, seed=1, frame_cap=1 << 22)

        def loop():
            for b in range(B):
                dn._clip(*each[b], None, 1, b, frame_cap=1 << 22)

        def pad():
            dn._clip(padded, pring, pola, phx, None, 1, 0, frame_cap=1 << 22)
        t = timed([ragged, loop, pad])
        r = dict(row="ragged", geometry="S", n_fft=dn.n_fft, clips=B, min_hops=min(n_hops), max_hops=longest, ragged_frames=F, ragged_ms=round(t[0], 3),
                 loop_frames=F, loop_ms=round(t[1], 3), padded_frames=B * longest, padded_ms=round(t[2], 3), loop_over_ragged=round(t[1] / t[0], 2),
                 padded_over_ragged=round(t[2] / t[0], 2))
        print(json.dumps(r), flush=True)
        rows.append(r)
        del each, padded
        torch.cuda.empty_cache()
    print(f"\n{'clips':>6} {'hops':>9} {'ragged ms':>10} {'frames':>7} {'B = 1 loop ms':>14} {'frames':>7} {'padded ms':>10} {'frames':>7} {'loop / ragged':>14} {'padded / ragged':>16}"
          f"   (median of {args.reps} alternating rounds)")
    for r in rows:
        print(f"{r['clips']:>6} {str(r['min_hops']) + '-' + str(r['max_hops']):>9} {r['ragged_ms']:>10.3f} {r['ragged_frames']:>7} {r['loop_ms']:>14.3f} {r['loop_frames']:>7} "
              f"{r['padded_ms']:>10.3f} {r['padded_frames']:>7} {r['loop_over_ragged']:>14.2f} {r['padded_over_ragged']:>16.2f}")


if __name__ == "__main__":
    main()
