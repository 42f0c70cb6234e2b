"""halo_host_view_source_pos — halo_view.h view_source_pos, the code halo_view_filtered_kernel takes its tap positions from — against the float64
lens model (tests/_lens_model.py, pinned to the oracle and the reference), on the directions halo_host_view_direction gives for every pixel of
every view of _view_model.all_views, under every source of _view_filter_model.sources.  No GPU.

  * hit count: the model's, on every direction the model calls decidable (its committed margins _lens_model.DELTA: culls, overlap band, pixel edges);
  * floor(pos + 0.5), taken in fp32 as the projection takes it, is the model's pixel for the primary hit and the overlap write alike (the
    rectangular lens: after the wrap), on every decidable direction whose hit lies within _lens_model.GUARD of the frame;
  * the continuous coordinates are the model's `f` (the argument of its floor) less 0.5, within DELTA["px"] — plus, for the single-view
    equidistant and stereographic lenses, what DELTA["acos"] of the rotated axis component moves the hit (the model's own allowance, kind acos);
  * t is the float64 tent (max_abs_dz - |sz|) / (2 max_abs_dz) within 4 x 2^-24: one difference, one product, one quotient of values <= 1;
  * at most 1 % of a pair's lookups are undecidable, none where the view is the source (then floor(pos + 0.5) is the pixel itself).
Then the struct's layout, the NULL guards, and the same function under the address and undefined-behaviour sanitizers as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend, build
from tests import _lens_model as lm
from tests import _view_filter_model as fm
from tests import _view_model as vm
from tests.test_view_model import host_directions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SOURCES = fm.sources()
_dirs = {}


def directions(vid, view):
    if vid not in _dirs:
        _dirs[vid] = host_directions(view)
    return _dirs[vid]


def floor_half(v):
    """floor(v + 0.5) in fp32, as project_exit takes it."""
    return np.floor(np.asarray(v, F32) + F32(0.5)).astype(np.int64)


def check_positions(P_src, source, dirs, name, cap):
    """dirs: float32[n, 3] that have a direction.  Returns the undecidable share."""
    cnt, pos = fm.host_source_pos(source, dirs)
    H = lm.project(P_src, dirs.astype(np.float64))
    dec = H.decidable()
    share = float((~dec).mean())
    assert share <= cap, (name, share)
    assert (cnt[dec] == H.count[dec]).all(), (name, int((cnt[dec] != H.count[dec]).sum()))
    assert (pos[cnt == 0] == 0.0).all() and (pos[cnt < 2, 2:] == 0.0).all(), name
    allow = lm.DELTA["px"] + lm.DELTA["acos"] * H.amp
    for hit in range(2):
        m = dec & (H.count > hit) & H.near[:, hit]
        if not m.any():
            continue
        px, py = floor_half(pos[m, 2 * hit]), floor_half(pos[m, 2 * hit + 1])
        if P_src.t == abi.LENS_RECTANGULAR:
            px = np.mod(px, P_src.w)
        assert (px == H.pix[m, hit, 0]).all() and (py == H.pix[m, hit, 1]).all(), (name, hit, int(((px != H.pix[m, hit, 0]) | (py != H.pix[m, hit, 1])).sum()))
        dev = np.abs(pos[m, 2 * hit:2 * hit + 2].astype(np.float64) - (H.f[m, hit, :] - 0.5)).max(axis=1)
        assert (dev <= allow[m]).all(), (name, hit, float((dev - allow[m]).max()))
    two = cnt == 2
    if two.any():
        sz = np.abs(dirs[two, 2].astype(np.float64))
        tent = (P_src.mad - sz) / (2.0 * P_src.mad)
        assert (np.abs(pos[two, 4].astype(np.float64) - tent) <= fm.T_BAR).all(), (name, float(np.abs(pos[two, 4] - tent).max()))
        assert (pos[two, 4] > 0.0).all() and (pos[two, 4] <= 0.5).all(), name
    return share


@pytest.mark.parametrize("k", range(len(SOURCES)), ids=[s[0] for s in SOURCES])
def test_host_positions_against_the_lens_model(k):
    sid, src = SOURCES[k]
    P_src = lm.proj_of(src)
    worst, n = 0.0, 0
    for s2, _, vid, view in fm.cpu_pairs():
        if s2 != sid:
            continue
        has, dirs = directions(vid, view)
        if has.any():
            worst = max(worst, check_positions(P_src, src, dirs[has], sid + " <- " + vid, 0.01))
        n += 1
    print("%s: %d views, worst undecidable share %.4f %%" % (sid, n, 100.0 * worst))
    assert n >= len(vm.all_views()) - 4


def test_view_equal_to_source_gives_the_pixel_itself():
    for name, r in vm.identity_renders():
        has, dirs = directions("identity-" + name, r)
        assert has.any(), name
        P = lm.proj_of(r)
        assert check_positions(P, r, dirs[has], name, 0.0) == 0.0
        cnt, pos = fm.host_source_pos(r, dirs[has])
        p = np.flatnonzero(has)
        px = floor_half(pos[:, 0])
        if P.t == abi.LENS_RECTANGULAR:
            px = np.mod(px, P.w)
        assert (cnt >= 1).all() and (px == p % r.width).all() and (floor_half(pos[:, 1]) == p // r.width).all(), name


def test_the_model_alone_keeps_every_pair_decidable():
    """From the MODEL's directions (no product code): the share of view pixels whose source lookup the lens model calls undecidable stays below
    1 % on every pair the CPU and GPU tests use — a pair with more would test little, and is listed in _view_filter_model.DROPPED instead."""
    worst = 0.0
    for sid, src, vid, view in fm.cpu_pairs():
        P_src, P = lm.proj_of(src), lm.proj_of(view)
        x, y = vm.pixel_grid(P)
        I = vm.inverse64(P, x, y)
        s = vm.undecidable_share(P_src, I.dir, I.valid)
        worst = max(worst, s)
        assert s <= 0.01, (sid, vid, s)
    assert {(p[0], p[2]) for p in fm.gpu_pairs()} <= {(p[0], p[2]) for p in fm.cpu_pairs()}      # (the GPU tests' pairs are among them)
    print("worst undecidable share of a pair, model alone: %.4f %%" % (100.0 * worst))


def test_filter_struct_layout_and_guards():
    L = backend.load_library()
    assert L.halo_abi_sizeof(16) == C.sizeof(abi.HaloViewFilter) == 16
    assert abi.HaloViewFilter.filter.offset == 0 and abi.HaloViewFilter.blend.offset == 4 and abi.HaloViewFilter.reserved.offset == 8
    assert (abi.VIEW_NEAREST, abi.VIEW_BILINEAR) == (0, 1)
    assert L.halo_abi_sizeof(17) == 0 and L.halo_abi_version() == 6
    sid, src = SOURCES[1]
    d = (C.c_float * 3)(0.0, 0.6, -0.8)
    pos = (C.c_float * 5)(*[7.0] * 5)
    assert L.halo_host_view_source_pos(None, d, pos) == 0 and list(pos) == [0.0] * 5
    assert L.halo_host_view_source_pos(C.byref(src), None, pos) == 0 and L.halo_host_view_source_pos(C.byref(src), d, None) == 0
    n, p = backend.host_view_source_pos(src, (0.0, 0.6, -0.8))
    assert n == 1 and (p[2:] == 0.0).all() and 0.0 <= p[0] < src.width / 2 and 0.0 <= p[1] < src.height
    n, p = backend.host_view_source_pos(src, (0.0, 1.0, 0.0))          # on the horizon: inside the band, both hemispheres weigh the same
    assert n == 2 and p[4] == 0.5
    bad = abi.HaloRender()
    C.memmove(C.byref(bad), C.byref(src), C.sizeof(bad))
    bad.lens_type = 11
    assert backend.host_view_source_pos(bad, (0.0, 0.6, -0.8))[0] == 0


def test_source_positions_under_sanitizers():
    """tests/cpp/view_filter_host_main.cpp, a program of its own built from the host sources alone with -fsanitize=address,undefined: no Python, no
    preload, no GPU."""
    csrc = os.path.join(ROOT, "ice_halo_sim_amd", "csrc")
    exe = os.path.join(ROOT, "tests", "cpp", "view_filter_host_main")
    subprocess.check_call([build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "view_filter_host_main.cpp"), os.path.join(csrc, "halo_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
