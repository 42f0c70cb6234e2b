"""The stream order of a handle on the host (csrc/halo_order.h), without a GPU: tests/cpp/order_main.cpp, a stand-alone program with its own main, is
built with g++ from that header alone — once plain, once under the address and undefined-behaviour sanitizers — and run on the CPU.  It instantiates
the unit with a vector-clock model of streams and events and checks, with overlap and lean_events each 0 and 1: the fork and the join (and the markers
a join clears), the alternation of the trace streams, the hop from the main stream and when lean_events leaves it out, launches behind and under a
fold (the aux_seq rule), the markers, the plane-ownership rules between the two trace streams, the four markers behind a direct close, the dispatch
ring, and that every stream and event the unit creates goes again — after the streams were waited for, events before streams, from a partly created
handle too.  The library that Python loads is not involved."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "order_main.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "order_main")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_stream_order(flags):
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
