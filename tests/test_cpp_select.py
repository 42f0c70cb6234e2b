"""The kernel selection on the host (csrc/halo_select.h), without a GPU: tests/cpp/select_main.cpp runs select_kernel over every request of
tests/cpp/select_enum.h (331 776 000 of them) and prints, per (mode, geom, mono), one line per chosen instantiation of halo_trace_kernel and per
error code: how many requests chose it and a 64-bit hash of their ordinal numbers.  tests/golden/kernel_selection.txt is that output as recorded from
the launchers of the tree before the selection moved into the header (tools/record_ladder, which asks the COMPILED launchers which kernel they
launch): a line that differs names the kernel that gained or lost requests.  The program's last line counts the expander's round trips — every
id of the kernel set to template constants and back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "select_main")
GOLDEN = os.path.join(ROOT, "tests", "golden", "kernel_selection.txt")
KERNELS = 283   # instantiations of halo_trace_kernel in the library (the "Name:" lines of build/resource_usage_halo_trace_*.txt)


@pytest.fixture(scope="module")
def output():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "select_main.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout.splitlines()


def test_every_request_selects_the_recorded_kernel(output):
    want = open(GOLDEN).read().splitlines()
    got = output[:-1]
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "first differing line:\n  recorded %s\n  selected %s" % diff[0]
    assert len(got) == len(want)
    assert sum(int(line.split("requests")[1].split()[0]) for line in got) == 331776000


def test_expander_round_trips_every_kernel_of_the_set(output):
    assert output[-1] == "round trip %d of %d" % (KERNELS, KERNELS)


def test_every_kernel_of_the_set_is_selected_by_some_request(output):
    chosen = {line.split(": ")[1].split("  ")[0] for line in output[:-1] if "halo_trace_kernel<" in line}
    assert len(chosen) == KERNELS
