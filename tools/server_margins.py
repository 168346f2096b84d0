#!/usr/bin/env python3
"""Measured parity margins of the server-variant tests on one tier: runs tests/test_emu_server.py (--tier emu, no GPU) or
tests/test_gpu_server.py (--tier gpu, one GPU) with the figures printed and reduces the `server-margin` lines to the worst value per stage
and geometry, then per stage -- what the guard bands in the two modules are ten times of.

    python tools/server_margins.py --tier emu [raw-pytest-output-file]
    python tools/server_margins.py --tier gpu [raw-pytest-output-file]
    python tools/server_margins.py --reduce FILE          reduces a kept raw output instead of running

profiles/server_parity_margins.txt is the output of both tiers, one after the other."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 480       # either module runs in about a minute; a run that takes this long hangs, and is killed


def main():
    args = sys.argv[1:]
    if len(args) == 2 and args[0] == "--reduce":
        with open(args[1]) as f:
            return reduce(f.read(), 0)
    if len(args) < 2 or args[0] != "--tier" or args[1] not in ("emu", "gpu"):
        print(__doc__)
        return 2
    tier = args[1]
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", f"test_{tier}_server.py"), "-s", "-q", "-p", "no:cacheprovider"]
    run = subprocess.run(cmd + (["-m", "gpu"] if tier == "gpu" else []), cwd=ROOT, capture_output=True, text=True, timeout=TIME_LIMIT_S)
    if len(args) > 2:
        with open(args[2], "w") as f:
            f.write(run.stdout + run.stderr)
    return reduce(run.stdout, run.returncode)


def reduce(stdout, returncode):
    cells, stages, bars, tiers = {}, {}, {}, set()
    for line in stdout.splitlines():
        # (pytest -q puts a finished test's mark in front of the next test's first line)
        m = re.match(r"[.FEsx]*?server-margin (\S+)\s+(.*) value=(\S+) bar=(\S+)$", line)
        if not m:
            continue
        stage, where, value, bar = m.group(1), dict(kv.split("=", 1) for kv in m.group(2).split(" ") if "=" in kv), float(m.group(3)), float(m.group(4))
        tiers.add(where["tier"])
        key = (stage, int(where["n_fft"]), where.get("n_mels", "-"), where.get("window", "-"))
        cells[key] = max(cells.get(key, 0.0), value)
        stages[stage] = max(stages.get(stage, 0.0), value)
        bars[stage] = max(bars.get(stage, 0.0), bar)
    tier = "/".join(sorted(tiers))
    print(f"# tier {tier}: worst value per stage, geometry and window, in the unit of the stage's bar (spec, istft: relative to max|ref|; "
          f"rows: to max(1, max|ref|); chain_rms / chain_max: to max(1, RMS of the float64 waveform); logmel, chain_hx, direction: absolute)")
    for (stage, n_fft, n_mels, window), v in sorted(cells.items()):
        print(f"{tier:<4} {stage:<10} n_fft {n_fft:>4} n_mels {n_mels:>3} window {window:<5} worst {v:.2e}")
    print(f"# tier {tier}: per stage")
    for stage, v in sorted(stages.items()):
        print(f"{tier:<4} worst {stage:<10} {v:.2e}   bar {bars[stage]:.2e}   10x = {10 * v:.2e}")
    print("# " + next(ln for ln in reversed(stdout.strip().splitlines()) if re.search(r"\d+ (passed|failed|error)", ln)))
    return returncode


if __name__ == "__main__":
    sys.exit(main())
