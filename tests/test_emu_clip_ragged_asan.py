"""The ragged clip call under AddressSanitizer and UBSan: tests/emu/clip_ragged_asan.cpp, a stand-alone program, runs two ragged cases (one with a
zero-length stream between live ones, one with the wavefront-per-frame chains, one iteration each) on exactly sized heap buffers.  The program, the
host units and the two clip units (every clip kernel and the bodies it inlines) are compiled as host C++ against the emulation header with
-fsanitize=address,undefined into one executable, the way tests/test_emu_host_faults.py builds its program; what else the host layer refers to comes
from the ordinary emulation library.  Nothing is preloaded, and no sanitizer runs on anything loaded into Python."""
import glob
import os
import subprocess
import sys

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EXE = os.path.join(emu.HERE, "build", "clip_ragged_asan")


def _build(lib):
    srcs = [os.path.join(emu.HERE, "clip_ragged_asan.cpp")] + sorted(glob.glob(os.path.join(emu.CSRC, "dn_api*.hip"))) + \
        [os.path.join(emu.CSRC, "dn_clip.hip"), os.path.join(emu.CSRC, "dn_clip_glw.hip")]
    deps = srcs + glob.glob(os.path.join(emu.CSRC, "*.hpp")) + [os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "dn_cpx.hpp"),
                                                                os.path.join(emu.REPO, "include", "dn_denoise.h"), lib]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-x", "c++", "-I", emu.HERE] + srcs + ["-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_ragged_clip_calls_stay_inside_exactly_sized_buffers():
    exe = _build(emu.build())
    r = subprocess.run([exe, os.path.join(GOLDEN, "weights_dari_tult.bin")], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "clip_ragged_asan: ok" in r.stdout
