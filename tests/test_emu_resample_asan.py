"""The resampler's two entry points under AddressSanitizer and UBSan: tests/emu/resample_asan.cpp, a stand-alone program, calls dn_resample and
dn_resample_push (both kernel forms, float32 and int16) on exactly sized heap buffers -- L = 1, one block, one block more than the history.  The
program, the host units and the resampler unit are compiled as host C++ against the emulation header with -fsanitize=address,undefined into one
executable, the way tests/test_emu_clip_ragged_asan.py builds its program; what else the host layer refers to comes from the ordinary emulation
library.  Nothing is preloaded, and no sanitizer runs on anything loaded into Python."""
import glob
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EXE = os.path.join(emu.HERE, "build", "resample_asan")


def _build(lib):
    srcs = [os.path.join(emu.HERE, "resample_asan.cpp")] + sorted(glob.glob(os.path.join(emu.CSRC, "dn_api*.hip"))) + [os.path.join(emu.CSRC, "dn_resample.hip")]
    deps = srcs + glob.glob(os.path.join(emu.CSRC, "*.hpp")) + [os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "dn_cpx.hpp"),
                                                                os.path.join(emu.REPO, "include", "dn_denoise.h"), lib]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-x", "c++", "-I", emu.HERE] + srcs + ["-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_resampler_calls_stay_inside_exactly_sized_buffers():
    exe = _build(emu.build())
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "resample_asan: ok" in r.stdout
