"""The device resampler (transforms.Resample: dn_resample) timed alone and inside clip mode, in one run on one GPU; the report goes to
profiles/resample_time.txt (--out).

Workload: 256 clips of 3 s, float32.
  alone      Resample at 48000 -> 16000, 16000 -> 48000 and 44100 -> 16000: time per call, the bytes a call has to move (every input sample read once,
             every output sample written once) over that time, beside the 6.29 TB/s a float4 copy reaches on this GPU
  clip       Denoiser.denoise_clip (16 kHz / n_fft 1024 / 80 mels, 32 iterations) of the same clips at 48 kHz with sample_rate=48000, against the
             same clips already at 16 kHz: what the two conversions add
--warmup untimed rounds, then the median of --reps rounds in which the forms of a section take turns, each timed with events on the current stream.
One JSON line per row, then tables.

    python tools/resample_time.py [--reps 7] [--warmup 2] [--out profiles/resample_time.txt]

The path without a rate must not have moved: `--clip-only` prints the one row of denoise_clip without sample_rate, and `--tree DIR` takes the package
from another checkout (a built parent).  Run it twice on the parent and twice on this tree, alternating, each output kept in a file, then

    python tools/resample_time.py --compare PARENT_1 NEW_1 PARENT_2 NEW_2 [--out FILE]   (appends to FILE)

prints the parent's two runs, their spread, this tree's two runs and the move of the mean against the parent's, in percent.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_RATE = 6.29e12          # bytes/s, float4 copy, measured on the MI355X
CLIPS, SECONDS = 256, 3


def compare(paths, out):
    runs = []
    for p in paths:
        with open(p) as f:
            rows = [json.loads(line) for line in f if line.startswith("{")]
        runs.append([r["ms"] for r in rows if r.get("row") == "clip_only"][0])
    p1, n1, p2, n2 = runs
    pm, nm = (p1 + p2) / 2, (n1 + n2) / 2
    text = (f"\ndenoise_clip without sample_rate, {CLIPS} clips of {SECONDS} s at 16 kHz, ms a call (spread = |parent 1 - parent 2| / mean, move = new mean / parent mean - 1)\n"
            f"{'parent 1':>9} {'parent 2':>9} {'spread %':>9} {'new 1':>9} {'new 2':>9} {'move %':>8}\n"
            f"{p1:>9.3f} {p2:>9.3f} {100 * abs(p1 - p2) / pm:>9.2f} {n1:>9.3f} {n2:>9.3f} {100 * (nm / pm - 1):>8.2f}\n")
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resample_time.txt"))
    ap.add_argument("--clip-only", action="store_true", help="only denoise_clip without sample_rate (works on a tree without the resampler)")
    ap.add_argument("--tree", default=REPO, help="the checkout whose package is timed")
    ap.add_argument("--compare", nargs=4, metavar="FILE", help="four --clip-only outputs: parent, new, parent, new")
    args = ap.parse_args()
    if args.compare:
        return compare(args.compare, args.out)
    sys.path.insert(0, os.path.abspath(args.tree))
    from audio_denoising_amd.gruunet2 import GRUUNet2
    from audio_denoising_amd.pipeline import Denoiser
    from oracle import model_ref, pipeline_ref
    assert torch.cuda.is_available(), "a timing needs the GPU"
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

    g = torch.Generator().manual_seed(2024)
    x16 = (0.1 * torch.randn(CLIPS, SECONDS * 16000, generator=g)).to(dev)
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(row)

    if args.clip_only:
        t, = timed([lambda: dn.denoise_clip(x16, seed=1)])
        emit(dict(row="clip_only", clips=CLIPS, seconds=SECONDS, ms=round(t, 3)))
        return
    from audio_denoising_amd.transforms import Resample
    text = [f"{CLIPS} clips of {SECONDS} s, float32; median of {args.reps} alternating rounds after {args.warmup} untimed ones\n"]
    text.append(f"{'pair':>15} {'o : n':>10} {'taps':>5} {'ms a call':>10} {'MB moved':>9} {'GB/s':>8} {'of the copy rate %':>19} {'GFLOP/s':>9}")
    for orig, new in ((48000, 16000), (16000, 48000), (44100, 16000)):
        r = Resample(orig, new)
        x = (0.1 * torch.randn(CLIPS, SECONDS * orig, generator=g)).to(dev)
        t, = timed([lambda: r(x)])
        moved = 4 * CLIPS * (x.shape[1] + r.out_len(x.shape[1]))
        flops = 2 * r.taps * CLIPS * r.out_len(x.shape[1])
        row = dict(row="alone", orig=orig, new=new, o=r.o, n=r.n, taps=r.taps, ms=round(t, 4), bytes=moved, bytes_per_s=round(moved / (t * 1e-3)),
                   of_copy_rate=round(moved / (t * 1e-3) / COPY_RATE, 4), flops=flops)
        emit(row)
        text.append(f"{str(orig) + '->' + str(new):>15} {str(r.o) + ' : ' + str(r.n):>10} {r.taps:>5} {t:>10.4f} {moved / 1e6:>9.1f} {moved / t / 1e6:>8.1f} "
                    f"{100 * moved / (t * 1e-3) / COPY_RATE:>19.2f} {flops / t / 1e6:>9.1f}")
        del x
    x48 = Resample(16000, 48000)(x16)
    t16, t48 = timed([lambda: dn.denoise_clip(x16, seed=1), lambda: dn.denoise_clip(x48, seed=1, sample_rate=48000)])
    emit(dict(row="clip", clips=CLIPS, seconds=SECONDS, at_16k_ms=round(t16, 3), at_48k_ms=round(t48, 3), added_ms=round(t48 - t16, 3), added=round(t48 / t16 - 1, 4)))
    text.append(f"\ndenoise_clip, ms a call: clips at 16 kHz {t16:.3f}; the same clips at 48 kHz with sample_rate=48000 {t48:.3f}; the two conversions add "
                f"{t48 - t16:.3f} ms ({100 * (t48 / t16 - 1):.2f} %)")
    report = "\n".join(text) + "\n"
    print("\n" + report)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(report)


if __name__ == "__main__":
    main()
