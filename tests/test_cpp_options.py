"""The option rules of halo_set_option on the host (csrc/halo_options.h), without a GPU: tests/cpp/options_main.cpp, a stand-alone program with its
own main, is built with g++ from that header alone — once plain, once under the address and undefined-behaviour sanitizers — and run on the CPU.  It
checks the 47 keys and their defaults (spec_root = 1 among them), every value rule at its edges, the refusals inside a session with their messages,
that a refused set leaves nothing behind (a legal set after it reports a change and the table-cache drop), what counts as "unchanged", and that rank,
ray_base and seed always act.  The library that Python loads is not involved."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "options_main.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "options_main")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_option_rules(flags):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
