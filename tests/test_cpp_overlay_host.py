"""The host half of the view stage's auxiliary lines under the address and undefined-behaviour sanitizers: tests/cpp/overlay_host_main.cpp, a
stand-alone program with its own main, is built from the host sources alone (halo_host.cpp with halo_overlay.h, compiled the way the library
compiles it: hipcc as a host compiler, no contraction) with -fsanitize=address,undefined and run on the CPU.  It sweeps all eleven lenses as views
over odd and even sizes, builds every pixel's sky coordinates and quad footprint and draws every layer with records at their limits, and tries
every refusal.  The library that Python loads is not involved, and no GPU."""
import os
import subprocess

from ice_halo_sim_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "overlay_host_main")


def test_overlay_host_functions_under_sanitizers():
    csrc = os.path.join(ROOT, "ice_halo_sim_amd", "csrc")
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", EXE,
                           os.path.join(ROOT, "tests", "cpp", "overlay_host_main.cpp"), os.path.join(csrc, "halo_host.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
