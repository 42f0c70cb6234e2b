"""Synthetic per-tile chunks for the closing pass of the per-tile append (launch_tile_route_close, halo_kernels.hip), through
tests/cpp/tile_close_shim.cpp.

  build_shim() / shim()   the host-only shim (libtile_close_shim.so, linked against libhalo_hip.so) and its ctypes signature
  deal_chunks             records dealt to chunk[tile][wg][cap] with the counts the trace kernel would report (records MET, so above cap where
                          a chunk overflowed); what lies behind a chunk's fill is poison that must never be read

The buffers (Buf), the fixed point and MonoSlot are tests/_passes.py's; the expected image is tests/_close.py's.  Everything here is numpy and
ctypes; nothing needs a GPU until tt_close is called.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import _passes as P

SHIM_SRC = os.path.join(P.ROOT, "tests", "cpp", "tile_close_shim.cpp")
SHIM_SO = os.path.join(P.ROOT, "tests", "cpp", "libtile_close_shim.so")
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
        raise RuntimeError("tile_close_shim.cpp failed to build:\n" + r.stdout + r.stderr)
    return SHIM_SO


_shim = None


def shim():
    global _shim
    if _shim is None:
        L = C.CDLL(build_shim())
        B, u32 = C.POINTER(P.PtBuf), C.c_uint32
        L.tt_device_count.restype = C.c_int; L.tt_device_count.argtypes = []
        L.tt_tiles_max.restype = u32; L.tt_tiles_max.argtypes = []
        L.tt_close.restype = C.c_int
        L.tt_close.argtypes = [B, u32, C.POINTER(C.c_float), B, B, B, B, u32, u32, u32, u32, u32, B, B, B]
        _shim = L
    return _shim


def deal_chunks(rng, counts, cap, tile_log2, weights, poison_w=1e6):
    """counts: int array [tiles, wgs] of records MET per chunk.  Returns (chunk uint32 [tiles * wgs * cap, 2], cnt uint32 [tiles * wgs], x, w) where
    x, w are the records the chunks HOLD (min(count, cap) each, slots drawn inside the chunk's tile, weights from `weights(n)`)."""
    counts = np.asarray(counts, dtype=np.int64)
    tiles, wgs = counts.shape
    held = np.minimum(counts, cap)
    n = int(held.sum())
    tile_of = np.repeat(np.repeat(np.arange(tiles, dtype=np.int64), wgs), held.ravel())
    x = ((tile_of << tile_log2) | rng.integers(0, 1 << tile_log2, size=n)).astype(np.uint32)
    w = np.asarray(weights(n), dtype=np.float32)
    chunk = np.zeros((tiles * wgs * cap, 2), dtype=np.uint32)
    every_tile = np.repeat(np.arange(tiles, dtype=np.int64), wgs * cap)
    chunk[:, 0] = ((every_tile << tile_log2) | rng.integers(0, 1 << tile_log2, size=len(chunk))).astype(np.uint32)   # poison: a valid slot of the tile ...
    chunk[:, 1] = np.float32(poison_w).view(np.uint32)                                                                # ... with a weight nobody could miss
    first = np.arange(tiles * wgs, dtype=np.int64) * cap
    at = np.repeat(first, held.ravel()) + (np.arange(n) - np.repeat(np.cumsum(held.ravel()) - held.ravel(), held.ravel()))
    chunk[at, 0] = x
    chunk[at, 1] = w.view(np.uint32)
    return chunk, counts.ravel().astype(np.uint32), x, w
