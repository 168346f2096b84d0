"""The rate bank's two calls under AddressSanitizer and UBSan: tests/emu/ratebank_asan.cpp, a stand-alone program, calls dn_ratebank_ingest and
dn_ratebank_emit (float32 and int16, a mixed list whose last row is the shortest chunk, a one-row list) on exactly sized heap buffers.  The
program, the host units and the two resampler units are compiled as host C++ against the emulation header with -fsanitize=address,undefined
into one executable, the way tests/test_emu_resample_asan.py builds its program; what else the host layer refers to comes from the ordinary
emulation library.  Nothing is preloaded, and no sanitizer runs on anything loaded into Python."""
import glob
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
import emu  # noqa: E402

EXE = os.path.join(emu.HERE, "build", "ratebank_asan")


def _build(lib):
    srcs = [os.path.join(emu.HERE, "ratebank_asan.cpp")] + sorted(glob.glob(os.path.join(emu.CSRC, "dn_api*.hip"))) + \
           [os.path.join(emu.CSRC, "dn_resample.hip"), os.path.join(emu.CSRC, "dn_ratebank.hip")]
    deps = srcs + glob.glob(os.path.join(emu.CSRC, "*.hpp")) + [os.path.join(emu.HERE, "hip", "hip_runtime.h"), os.path.join(emu.HERE, "dn_cpx.hpp"),
                                                                os.path.join(emu.REPO, "include", "dn_denoise.h"), lib]
    if os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           "-x", "c++", "-I", emu.HERE] + srcs + ["-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", EXE]
    subprocess.run(cmd, check=True)
    return EXE


def test_ratebank_calls_stay_inside_exactly_sized_buffers():
    exe = _build(emu.build())
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "ratebank_asan: ok" in r.stdout
