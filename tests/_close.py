"""Synthetic records for the closing form of the scalar per-tile pass (launch_log_route_close, halo_kernels.hip), through tests/cpp/close_shim.cpp.

  build_shim() / shim()   the host-only shim (libclose_shim.so, linked against libhalo_hip.so) and its ctypes signature
  tile_sums               what the pass holds per slot before it looks at the twin: float32(float64(sum of fix(w)) * 2^-F)
  with_twin               ... and after: float32(float64(t) + o) where the twin holds o != 0
  expected_image          float32(xyz_before + float32(coef_c * t)) at the pixel of every slot with t != 0, pixels below n_pix only

The buffers (Buf), the fixed point (fix / unfix / slot_sums), MonoSlot and the dealing of records to log regions are tests/_passes.py's.
Everything here is numpy and ctypes; nothing needs a GPU until ct_close is called.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import _passes as P

SHIM_SRC = os.path.join(P.ROOT, "tests", "cpp", "close_shim.cpp")
SHIM_SO = os.path.join(P.ROOT, "tests", "cpp", "libclose_shim.so")
SHIM_DEPS = [SHIM_SRC, os.path.join(P.PKG, "csrc", "halo_launch.h"), os.path.join(P.PKG, "csrc", "halo_device.h"), os.path.join(P.ROOT, "include", "halo_trace.h")]


def build_shim(force=False):
    """Compile the shim the way halo_backend.cpp is compiled (hipcc as a host compiler, no device code), when it is missing or older than its sources."""
    from ice_halo_sim_amd import build as hip_build
    if not force and os.path.exists(SHIM_SO) and all(os.path.getmtime(d) <= os.path.getmtime(SHIM_SO) for d in SHIM_DEPS):
        return SHIM_SO
    if not os.path.exists(hip_build.LIB):
        raise ImportError("libhalo_hip.so is not built — run `python -m ice_halo_sim_amd.build` (needs hipcc)")
    cmd = [hip_build.hipcc(), "-O2", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(P.ROOT, "include"), "-I", os.path.join(P.PKG, "csrc"), SHIM_SRC, "-o", SHIM_SO,
           "-L" + P.PKG, "-lhalo_hip", "-Wl,-rpath," + P.PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("close_shim.cpp failed to build:\n" + r.stdout + r.stderr)
    return SHIM_SO


_shim = None


def shim():
    global _shim
    if _shim is None:
        L = C.CDLL(build_shim())
        B, u32 = C.POINTER(P.PtBuf), C.c_uint32
        L.ct_device_count.restype = C.c_int; L.ct_device_count.argtypes = []
        L.ct_close.restype = C.c_int
        L.ct_close.argtypes = [B, u32, C.POINTER(C.c_float), B, B, u32, B, B, u32, u32, B, u32, B, u32, u32, u32, B, B, B, B]
        _shim = L
    return _shim


def tile_sums(slots, w, n_slots, frac_bits):
    return P.unfix(P.slot_sums(slots, P.fix(w, frac_bits), n_slots), frac_bits)


def with_twin(t, twin):
    """the fold's way with the twin: only where it holds something, one rounding of the fp64 sum"""
    t = np.asarray(t, dtype=np.float32)
    twin = np.asarray(twin, dtype=np.float64)
    return np.where(twin != 0.0, (t.astype(np.float64) + twin).astype(np.float32), t).astype(np.float32)


def expected_image(before, t, coef, n_pix, s):
    """before: float32 [>= n_pix, 3] (rows from n_pix on must stay as they are); t: float32 per slot of the plane of 1024 << s slots"""
    out = np.array(before, dtype=np.float32)
    pix = np.arange(n_pix, dtype=np.uint64)
    v = np.asarray(t, dtype=np.float32)[P.mono_slot(pix, s)]
    hit = v != 0.0   # (a NaN sum would count; the weights here never make one)
    for c in range(3):
        prod = (np.float32(coef[c]) * v).astype(np.float32)            # rounded once ...
        out[:n_pix, c] = np.where(hit, (out[:n_pix, c] + prod).astype(np.float32), out[:n_pix, c])   # ... and the add once more
    return out
