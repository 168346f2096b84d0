#!/usr/bin/env python3
"""Measured parity margins of the any-length Griffin-Lim tests on one tier: runs tests/test_emu_glg.py (--tier emu, no GPU) or
tests/test_gpu_glg.py (--tier gpu, one GPU) with the figures printed and reduces the `glg-margin` lines to the worst value per stage and
n_fft, then per stage -- what the guard bands in the two modules are ten times of.

    python tools/glg_margins.py --tier emu [raw-pytest-output-file]
    python tools/glg_margins.py --tier gpu [raw-pytest-output-file]
    python tools/glg_margins.py --reduce FILE          reduces a kept raw output instead of running

profiles/glg_parity_margins.txt is the output of both tiers, one after the other."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 900       # the emulation module runs in about three minutes, the GPU one in seconds; a run that takes this long hangs, and is killed


def main():
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--reduce":
        with open(args[1]) as f:
            return reduce(f.read(), 0)
    if len(args) < 2 or args[0] != "--tier" or args[1] not in ("emu", "gpu"):
        print(__doc__)
        return 2
    tier = args[1]
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", f"test_{tier}_glg.py"), "-s", "-q", "-p", "no:cacheprovider"]
    run = subprocess.run(cmd + (["-m", "gpu"] if tier == "gpu" else []), cwd=ROOT, capture_output=True, text=True, timeout=TIME_LIMIT_S)
    if len(args) > 2:
        with open(args[2], "w") as f:
            f.write(run.stdout + run.stderr)
    return reduce(run.stdout, run.returncode)


def reduce(stdout, returncode):
    cells, stages, bars, tiers = {}, {}, {}, set()
    for line in stdout.splitlines():
        # (pytest -q puts a finished test's mark in front of the next test's first line)
        m = re.match(r"[.FEsx]*?glg-margin (\S+)\s+(.*) value=(\S+) bar=(\S+)$", line)
        if not m:
            continue
        stage, where, value, bar = m.group(1), dict(kv.split("=", 1) for kv in m.group(2).split(" ") if "=" in kv), float(m.group(3)), float(m.group(4))
        tiers.add(where["tier"])
        key = (stage, int(where["n_fft"]))
        cells[key] = max(cells.get(key, 0.0), value)
        stages[stage] = max(stages.get(stage, 0.0), value)
        bars[stage] = max(bars.get(stage, 0.0), bar)
    tier = "/".join(sorted(tiers))
    print(f"# tier {tier}: worst value per stage and n_fft, in the unit of the stage's bar (*_rms, *_max: waveform error at scale max(1, RMS of the "
          f"float64 waveform); normalize0, direction, zero_iter_pair, t_spec, t_istft: relative to the peak; mag_rows: to max(1, max|ref|); glchain_hx: absolute)")
    for (stage, n_fft), v in sorted(cells.items()):
        print(f"{tier:<4} {stage:<15} n_fft {n_fft:>4} worst {v:.2e}")
    print(f"# tier {tier}: per stage")
    for stage, v in sorted(stages.items()):
        print(f"{tier:<4} worst {stage:<15} {v:.2e}   bar {bars[stage]:.2e}   10x = {10 * v:.2e}")
    print("# " + next(ln for ln in reversed(stdout.strip().splitlines()) if re.search(r"\d+ (passed|failed|error)", ln)))
    return returncode


if __name__ == "__main__":
    sys.exit(main())
