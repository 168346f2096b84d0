#!/usr/bin/env python3
"""Measured parity margins of the window tests (tests/test_gpu_windows.py) on one GPU: runs the module with its figures printed and
reduces the `window-margin` lines to the worst value per stage, n_fft and window, then per stage -- what the guard bands in that module
are ten times of.  `python tools/window_margins.py [raw-pytest-output-file] > profiles/window_parity_margins.txt`; `--reduce FILE` reduces a kept raw output
instead of running."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 480       # the module runs in about a minute; a run that takes this long hangs, and is killed


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--reduce":          # a kept raw output of an earlier run
        with open(sys.argv[2]) as f:
            return reduce(f.read(), 0)
    run = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_windows.py"), "-m", "gpu", "-s", "-q",
                          "-p", "no:cacheprovider"], cwd=ROOT, capture_output=True, text=True, timeout=TIME_LIMIT_S)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(run.stdout + run.stderr)
    return reduce(run.stdout, run.returncode)


def reduce(stdout, returncode):
    cells, stages, bars, notes = {}, {}, {}, []
    for line in stdout.splitlines():
        line = line.lstrip(".FEsx")                      # (pytest -q puts a finished test's mark in front of the next test's first line)
        if not line.startswith("window-margin"):
            continue
        m = re.match(r"window-margin (\S+)\s+(.*) value=(\S+) bar=(\S+)$", line)
        if not m:
            notes.append(line)
            continue
        stage, where, value, bar = m.group(1), dict(kv.split("=", 1) for kv in m.group(2).split(" ") if "=" in kv), float(m.group(3)), float(m.group(4))
        key = (stage, where.get("n_fft", "1024"), where.get("window", "-"))
        cells[key] = max(cells.get(key, 0.0), value)
        stages[stage] = max(stages.get(stage, 0.0), value)
        bars[stage] = max(bars.get(stage, 0.0), bar)
    for (stage, n_fft, window), v in sorted(cells.items()):
        print(f"{stage:<18} n_fft {n_fft:>4} window {window:<8} worst {v:.2e}")
    print()
    for stage, v in sorted(stages.items()):
        print(f"worst {stage:<18} {v:.2e}   bar {bars[stage]:.2e}   10x = {10 * v:.2e}")
    for line in notes:
        print(line)
    print(next(l for l in reversed(stdout.strip().splitlines()) if re.search(r"\d+ (passed|failed|error)", l)))
    return returncode


if __name__ == "__main__":
    sys.exit(main())
