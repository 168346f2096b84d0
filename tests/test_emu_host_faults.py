"""The host layer (csrc/dn_api*.hip: every device allocation, event and copy queue of the handles) on its own, under AddressSanitizer, UBSan and
LeakSanitizer: tests/emu/host_faults.cpp runs one scenario over every handle with the n-th resource-creating call failing, for every n.  The five
host units and the program are compiled as host C++ against the emulation header with -fsanitize=address,undefined into one executable (nothing is
preloaded); the kernel launchers come from the ordinary emulation library.  What the program requires of each call is in its header comment."""
import glob
import os
import subprocess
import sys

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EXE = os.path.join(emu.HERE, "build", "host_faults")


def _build(lib):
    srcs = [os.path.join(emu.HERE, "host_faults.cpp")] + sorted(glob.glob(os.path.join(emu.CSRC, "dn_api*.hip")))
    deps = srcs + glob.glob(os.path.join(emu.CSRC, "*.hpp")) + [os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "dn_cpx.hpp"),
                                                                os.path.join(emu.REPO, "include", "dn_denoise.h"), lib]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-x", "c++", "-I", emu.HERE] + srcs + ["-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_host_layer_survives_a_failure_of_every_resource_creation():
    exe = _build(emu.build())
    r = subprocess.run([exe, os.path.join(GOLDEN, "weights_dari_tult.bin")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    points = int(r.stdout.split("injection points visited:")[1].split()[0])
    # the host-buffer transport alone makes 19 such calls (2 copy queues, 12 events, 4 staging buffers, the completion word) and the pool 11 (5 device
    # buffers, 2 page-locked ones, 4 events): fewer than 30 visited points means the injection did not reach them
    assert points >= 30, points
