"""The shard entry points through the C++ adapter (hip_trace_backend.hpp SetShard / ExportFixed / ImportFixed): tests/cpp/shards_main.cpp traces one
deterministic session whole and as two shards, adds the exported words as integers, imports them into shard 0 and compares image bytes."""
import os
import subprocess

import pytest

from ice_halo_sim_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "shards_main")


def _build():
    backend.load_library()
    libdir = os.path.join(ROOT, "ice_halo_sim_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "shards_main.cpp"),
                           "-L" + libdir, "-lhalo_hip", "-ldl", "-Wl,-rpath," + libdir])


def test_shard_program_compiles_and_reports_unavailable_without_gpu():
    _build()
    r = subprocess.run([EXE], capture_output=True, text=True)
    if backend.load_library().halo_device_count() == 0:
        assert r.returncode == 3, r.stdout + r.stderr
        assert "BackendUnavailableError" in r.stdout


@pytest.mark.gpu
def test_two_shards_merged_through_the_adapter_give_the_whole_runs_bytes():
    _build()   # always: a binary that travelled with the snapshot may predate the header
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)   # (a hang must fail this test, not stall the suite)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "same_bytes 1" in r.stdout and "guarded 1" in r.stdout, r.stdout
