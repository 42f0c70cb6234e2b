"""Host-side mirror of the reference's trace-backend seam over the C ABI (libhalo_hip.so).

`HipTraceBackend` follows `lumice::TraceBackend` (reference src/core/backend/trace_backend.hpp:367-641)
method for method: BeginSession / TraceLayer / Recombine / DrainExits / ReadbackXyzAccum / EndSession,
same state machine, `BackendUnavailableError` as the one recoverable error.  It is a thin ctypes layer:
all computing happens in the HIP library, and importing this module without the built library (or
without a gfx950 device at create time) fails loudly — there is no CPU fallback here.
"""
import ctypes as C
import math
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# HALO_LIB selects another build of the same library (tools/phase_probe.py loads the -DHALO_PROBE build); default = the product
LIB_PATH = os.environ.get("HALO_LIB") or os.path.join(_HERE, "libhalo_hip.so")
_lib = None


class BackendUnavailableError(RuntimeError):
    """Reference: BackendUnavailableError, trace_backend.hpp:140-158 (the only recoverable error)."""


class BackendError(RuntimeError):
    pass


def load_library():
    """dlopen the in-tree HIP library and declare every symbol of include/halo_trace.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libhalo_hip.so is not built — run `python -m ice_halo_sim_amd.build` (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    H = C.c_void_p
    f32p = C.POINTER(C.c_float)
    sig = {
        "halo_abi_version": (C.c_int, []),
        "halo_abi_sizeof": (C.c_uint64, [C.c_int]),
        "halo_device_count": (C.c_int, []),
        "halo_create": (C.c_int, [C.c_int, C.c_uint32, C.POINTER(H)]),
        "halo_destroy": (C.c_int, [H]),
        "halo_last_error": (C.c_char_p, [H]),
        "halo_set_option": (C.c_int, [H, C.c_char_p, C.c_int64]),
        "halo_set_stream": (C.c_int, [H, C.c_void_p]),
        "halo_bind_accumulator": (C.c_int, [H, C.c_void_p, C.c_uint64]),
        "halo_set_filters": (C.c_int, [H, C.POINTER(abi.HaloFilter), C.c_int32]),
        "halo_begin": (C.c_int, [H, C.POINTER(abi.HaloScene), C.POINTER(abi.HaloRender), C.POINTER(abi.HaloWl), C.c_uint64]),
        "halo_begin_spectrum": (C.c_int, [H, C.POINTER(abi.HaloScene), C.POINTER(abi.HaloRender), C.POINTER(abi.HaloWl), C.c_int32, C.c_uint64]),
        "halo_host_spectrum_entry": (C.c_uint32, [C.c_uint64, C.c_uint32, C.c_uint64]),
        "halo_trace_layer": (C.c_int, [H, C.c_uint64, C.POINTER(abi.HaloHostRays), C.POINTER(abi.HaloLayerStats)]),
        "halo_recombine": (C.c_int, [H, C.c_int, C.POINTER(C.c_uint64)]),
        "halo_drain_exits": (C.c_int, [H, C.POINTER(abi.HaloExitRecord), C.c_uint64, C.POINTER(C.c_uint64)]),
        "halo_end": (C.c_int, [H]),
        "halo_readback_xyz": (C.c_int, [H, f32p, C.c_int, C.c_int, f32p]),
        "halo_readback_xyz64": (C.c_int, [H, f32p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
        "halo_sync": (C.c_int, [H]),
        "halo_last_sample_counts": (C.c_int, [H, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "halo_last_route": (C.c_int, [H, C.POINTER(abi.HaloRouteInfo)]),
        "halo_last_root_profile": (C.c_int, [H, C.POINTER(C.c_uint32)]),
        "halo_direct_closes": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "halo_tile_appends": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "halo_tile_tickets": (C.c_int, [H, C.POINTER(C.c_uint64)]),
        "halo_host_ticket_size": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "halo_host_ticket_groups": (C.c_uint32, []),
        "halo_host_ticket_range": (None, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "halo_host_ticket_next": (C.c_uint32, [C.c_uint64, C.c_uint32]),
        "halo_set_color": (C.c_int, [H, C.POINTER(abi.HaloColorSet), C.c_int, C.POINTER(abi.HaloColorClass), C.c_int]),
        "halo_readback_class_lanes": (C.c_int, [H, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int]),
        "halo_generate_shapes": (C.c_int, [H, C.POINTER(abi.HaloCrystal), C.c_uint64, C.c_uint32, C.c_int, C.POINTER(abi.HaloGeomTables)]),
        "halo_collect_stats": (C.c_int, [H, C.POINTER(abi.HaloLayerStats)]),
        "halo_take_landed": (C.c_int, [H, C.POINTER(C.c_double)]),
        "halo_peek_fixed": (C.c_int, [H, C.c_int32, C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
        "halo_host_fixed_frac_bits": (C.c_uint32, [C.c_double, C.c_uint64]),
        "halo_set_shard": (C.c_int, [H, C.c_uint32, C.c_uint32]),
        "halo_host_shard_slice": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "halo_export_fixed": (C.c_int, [H, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "halo_import_fixed": (C.c_int, [H, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]),
        "halo_flush": (C.c_int, [H]),
        "halo_collect_timing": (C.c_int, [H, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "halo_consumer_fold": (C.c_int, [H]),
        "halo_consumer_consume": (C.c_int, [H, f32p, C.c_int, C.c_int, C.c_float, f32p, C.c_int]),
        "halo_consumer_snapshot": (C.c_int, [H, C.POINTER(abi.HaloDisplay), C.POINTER(C.c_uint8), f32p, C.POINTER(C.c_double)]),
        "halo_consumer_reset": (C.c_int, [H]),
        "halo_consumer_auto_ev": (C.c_int, [H, C.c_int32, C.c_float, C.POINTER(abi.HaloAutoEv)]),
        "halo_host_ev_auto": (C.c_float, [C.c_float, C.c_float, C.c_float]),
        "halo_consumer_stats": (C.c_int, [H, C.POINTER(abi.HaloStatsSpec), C.POINTER(abi.HaloImageStats)]),
        "halo_host_percentile_rank": (C.c_int, [C.c_double, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
        "halo_host_binned_sum": (C.c_int, [C.POINTER(C.c_uint64), C.c_int32, C.POINTER(C.c_double)]),
        "halo_consumer_view": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(C.c_uint8), f32p, C.POINTER(C.c_int32), f32p]),
        "halo_host_view_direction": (C.c_int, [C.POINTER(abi.HaloRender), C.c_int32, C.c_int32, f32p]),
        "halo_consumer_view_filtered": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(abi.HaloViewFilter), C.POINTER(C.c_uint8), f32p, C.POINTER(C.c_int32), f32p, f32p]),
        "halo_host_view_source_pos": (C.c_int, [C.POINTER(abi.HaloRender), f32p, f32p]),
        "halo_consumer_composite": (C.c_int, [H, C.POINTER(abi.HaloComposite), f32p, C.POINTER(C.c_uint8), f32p, C.POINTER(C.c_int32)]),
        "halo_consumer_load_lanes": (C.c_int, [H, f32p, C.c_int, C.c_int, C.c_int, C.c_double]),
        "halo_host_parse_composite_mode": (C.c_int, [C.c_char_p]),
        "halo_consumer_view_composite": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(abi.HaloViewFilter), C.POINTER(abi.HaloComposite), C.POINTER(C.c_uint8), f32p,
                                                   C.POINTER(C.c_int32), f32p, f32p, C.POINTER(C.c_int32)]),
        "halo_consumer_view_lanes": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(abi.HaloViewFilter), f32p, C.POINTER(C.c_int32), f32p]),
        "halo_host_view_overlay_defaults": (C.c_int, [C.c_float, f32p, C.POINTER(abi.HaloViewOverlay)]),
        "halo_consumer_view_overlay": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(abi.HaloViewFilter), C.POINTER(abi.HaloViewOverlay), C.POINTER(C.c_uint8), f32p, f32p,
                                                 f32p, C.POINTER(C.c_int32), f32p]),
        "halo_consumer_view_composite_overlay": (C.c_int, [H, C.POINTER(abi.HaloViewSpec), C.POINTER(abi.HaloViewFilter), C.POINTER(abi.HaloComposite),
                                                           C.POINTER(abi.HaloViewOverlay), C.POINTER(C.c_uint8), f32p, f32p, f32p, C.POINTER(C.c_int32), f32p, f32p, f32p,
                                                           C.POINTER(C.c_int32)]),
        "halo_host_view_sky": (C.c_int, [f32p, f32p, f32p]),
        "halo_host_view_overlay_pixel": (C.c_int, [C.POINTER(C.c_uint8), f32p, f32p, f32p, C.POINTER(abi.HaloViewOverlay), f32p]),
        "halo_host_prism_geometry": (C.c_int, [C.c_float, f32p, C.POINTER(abi.HaloGeomTables)]),
        "halo_host_pyramid_geometry": (C.c_int, [C.c_float] * 5 + [f32p, C.POINTER(abi.HaloGeomTables)]),
        "halo_host_shape_scalars": (C.c_int, [C.POINTER(abi.HaloCrystal), C.c_uint32, C.c_uint64, C.c_int, f32p]),
        "halo_host_build_lat_lut": (C.c_int, [C.POINTER(abi.HaloDist), f32p, f32p, f32p]),
        "halo_host_build_proj_params": (C.c_int, [C.POINTER(abi.HaloRender), C.c_void_p]),
        "halo_host_partition": (C.c_int, [f32p, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "halo_host_refractive_index": (C.c_double, [C.c_double]),
        "halo_reduce_accumulator": (C.c_int, [H, C.c_void_p, C.c_int, C.c_int]),
        "halo_host_illuminant_spd": (C.c_float, [C.c_int, C.c_float]),
        "halo_host_wl_pool": (C.c_int, [C.POINTER(abi.HaloWl), f32p, C.c_int]),
        "halo_host_reduce_raypath": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8)]),
        "halo_host_filter_fast_check": (C.c_int, [C.POINTER(abi.HaloFilter), C.POINTER(abi.HaloAxis), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                                  C.POINTER(C.c_int32)]),
        "halo_host_color_fast_mask": (C.c_int, [C.POINTER(abi.HaloColorSet), C.POINTER(abi.HaloAxis), C.POINTER(C.c_uint8), C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                                C.c_uint64, C.POINTER(C.c_uint64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError here = the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


EXPORTED_SYMBOLS = [
    "halo_abi_version", "halo_abi_sizeof", "halo_device_count", "halo_create", "halo_destroy", "halo_last_error",
    "halo_set_option", "halo_set_stream", "halo_bind_accumulator", "halo_set_filters", "halo_begin", "halo_trace_layer", "halo_recombine",
    "halo_drain_exits", "halo_end", "halo_readback_xyz", "halo_readback_xyz64", "halo_sync", "halo_flush", "halo_collect_timing", "halo_last_sample_counts", "halo_last_route", "halo_last_root_profile", "halo_direct_closes", "halo_tile_appends", "halo_tile_tickets", "halo_host_ticket_size", "halo_host_ticket_groups", "halo_host_ticket_range", "halo_host_ticket_next", "halo_set_color", "halo_readback_class_lanes", "halo_generate_shapes", "halo_collect_stats", "halo_take_landed", "halo_consumer_fold", "halo_consumer_consume", "halo_consumer_snapshot", "halo_consumer_reset", "halo_consumer_composite", "halo_consumer_load_lanes", "halo_host_parse_composite_mode", "halo_host_prism_geometry",
    "halo_host_pyramid_geometry", "halo_host_shape_scalars", "halo_host_build_lat_lut", "halo_host_build_proj_params", "halo_host_partition",
    "halo_host_refractive_index", "halo_host_reduce_raypath", "halo_host_filter_fast_check", "halo_host_color_fast_mask", "halo_host_illuminant_spd", "halo_host_wl_pool", "halo_reduce_accumulator",
    "halo_peek_fixed", "halo_host_fixed_frac_bits", "halo_begin_spectrum", "halo_host_spectrum_entry",
    "halo_consumer_auto_ev", "halo_host_ev_auto",
    "halo_consumer_stats", "halo_host_percentile_rank", "halo_host_binned_sum",
    "halo_consumer_view", "halo_host_view_direction", "halo_consumer_view_filtered", "halo_host_view_source_pos",
    "halo_consumer_view_composite", "halo_consumer_view_lanes",
    "halo_host_view_overlay_defaults", "halo_consumer_view_overlay", "halo_consumer_view_composite_overlay", "halo_host_view_sky", "halo_host_view_overlay_pixel",
    "halo_set_shard", "halo_host_shard_slice", "halo_export_fixed", "halo_import_fixed",
]


class HipTraceBackend:
    """One backend instance = one `Simulator::Run()` thread's backend (single-threaded use)."""

    def __init__(self, device=0, seed=42, **options):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.halo_create(int(device), int(seed) & 0xFFFFFFFF, C.byref(self._h))
        if rc == abi.HALO_UNAVAILABLE:
            raise BackendUnavailableError("no gfx950 device %d (halo_create)" % device)
        if rc != abi.HALO_OK:
            raise BackendError("halo_create failed")
        self._render = None
        self._scene = None
        self._pending_roots = 0
        for k, v in options.items():
            self.set_option(k, v)

    # --- plumbing ---
    def _check(self, rc):
        if rc == abi.HALO_OK:
            return
        msg = self._L.halo_last_error(self._h)
        msg = msg.decode() if msg else "?"
        if rc == abi.HALO_UNAVAILABLE:
            raise BackendUnavailableError(msg)
        raise BackendError(msg)

    def close(self):
        if self._h:
            self._L.halo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        self._check(self._L.halo_set_option(self._h, key.encode(), int(value)))

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.halo_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_filters(self, filters):
        """Filter table referenced by HaloEntry.filter_id (1-based; 0 = none)."""
        arr = (abi.HaloFilter * max(1, len(filters)))(*filters)
        self._check(self._L.halo_set_filters(self._h, arr, len(filters)))

    def set_color(self, sets, classes):
        """Raypath-colour tables: `sets` referenced by HaloEntry.color_id (1-based), `classes` define the Y lanes."""
        sa = (abi.HaloColorSet * max(1, len(sets)))(*sets)
        ca = (abi.HaloColorClass * max(1, len(classes)))(*classes)
        self._check(self._L.halo_set_color(self._h, sa, len(sets), ca, len(classes)))
        self._n_classes = len(classes)

    def ReadbackClassLanes(self):
        """TraceBackend::ReadbackClassLanes: (class_count, H, W) float32 Y lanes; zeroes the device lanes."""
        w, h, n = self._render.width, self._render.height, getattr(self, "_n_classes", 0)
        out = np.zeros((n, h, w), np.float32)
        if n:
            self._check(self._L.halo_readback_class_lanes(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), w, h, n))
        return out

    def bind_accumulator(self, device_ptr, n_floats):
        self._check(self._L.halo_bind_accumulator(self._h, C.c_void_p(device_ptr), int(n_floats)))

    def sync(self):
        self._check(self._L.halo_sync(self._h))

    def collect_timing(self):
        """(trace_ms, post_ms, launches) of the sessions' LAST layers since the previous call: the trace kernels' own spans (HIP events on the
        launch's stream) and those of their accumulation passes."""
        t, p, n = C.c_double(), C.c_double(), C.c_uint64()
        self._check(self._L.halo_collect_timing(self._h, C.byref(t), C.byref(p), C.byref(n)))
        return t.value, p.value, n.value

    def flush(self):
        """Queue the pending closing folds and make the backend's stream wait for them (no host wait): what is queued on that stream afterwards
        sees the finished image — the call a holder of a BOUND accumulator makes before it touches its memory when option defer_fold is on."""
        self._check(self._L.halo_flush(self._h))

    def generate_shapes(self, crystal, first_index, n, on_device=True):
        """`n` sampled instances of `crystal` as HaloGeomTables (device generator or the host builder)."""
        out = (abi.HaloGeomTables * n)()
        self._check(self._L.halo_generate_shapes(self._h, C.byref(crystal), int(first_index), int(n), int(on_device), out))   # 0 host | 1 general records | 2 prism records
        return out

    def last_sample_counts(self):
        """(stochastic crystal instances sampled, rays whose orientation was drawn) in the session traced last."""
        a, b = C.c_uint64(), C.c_uint64()
        self._check(self._L.halo_last_sample_counts(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_route(self):
        """HaloRouteInfo of the session traced last: which kernel instantiations and accumulation routes really ran."""
        r = abi.HaloRouteInfo()
        self._check(self._L.halo_last_route(self._h, C.byref(r)))
        return r

    def last_root_profile(self):
        """abi.ROOT_* bits of the root-generation profiles that ran as compile-time constants in the session traced last (0 = none did)."""
        m = C.c_uint32()
        self._check(self._L.halo_last_root_profile(self._h, C.byref(m)))
        return m.value

    def direct_closes(self):
        """Launches of this backend, ever, that closed their session in their own per-tile pass (option close_direct): a cumulative count."""
        n = C.c_uint64()
        self._check(self._L.halo_direct_closes(self._h, C.byref(n)))
        return n.value

    def tile_appends(self):
        """Launches of this backend, ever, whose trace kernel appended its records per tile (option tile_append): a cumulative count."""
        n = C.c_uint64()
        self._check(self._L.halo_tile_appends(self._h, C.byref(n)))
        return n.value

    def tile_tickets(self):
        """Launches of this backend, ever, whose trace kernel drew its rays by wave tickets (option tile_ticket): a cumulative count."""
        n = C.c_uint64()
        self._check(self._L.halo_tile_tickets(self._h, C.byref(n)))
        return n.value

    def collect_stats(self):
        """Summed tallies of every layer traced since the previous call (waits for the stream); the only source of
        exit / pixel-hit / kernel-time numbers for layers traced with option async=1."""
        st = abi.HaloLayerStats()
        self._check(self._L.halo_collect_stats(self._h, C.byref(st)))
        return st

    def take_landed(self):
        v = C.c_double()
        self._check(self._L.halo_take_landed(self._h, C.byref(v)))
        return v.value

    def peek_fixed(self, plane=0):
        """The pending fixed-point planes of deterministic sessions (option deterministic = 1, after EndSession, lazy_fold = 1, own accumulator)
        as the integers they are: (sums uint64[H, W] of `plane` in pixel order, frac_bits, landed uint64 scalar, landed_frac_bits).  A plane
        value is sums * 2**-frac_bits, the landed weight landed * 2**-landed_frac_bits.  Folds, zeroes and takes nothing; BackendError when
        no fixed-point planes are pending."""
        w, h = self._render.width, self._render.height
        sums = np.empty((h, w), np.uint64)
        f, fl, landed = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self._L.halo_peek_fixed(self._h, int(plane), sums.ctypes.data_as(C.POINTER(C.c_uint64)), w * h, C.byref(f), C.byref(landed), C.byref(fl)))
        return sums, f.value, np.uint64(landed.value), fl.value

    # --- shards: N handles trace one session's rays between them (halo_set_shard, halo_export_fixed, halo_import_fixed) ---
    def set_shard(self, index, count):
        """This handle is shard `index` of `count` ((0, 1) = the default, everything): BeginSession / TraceLayer then take the WHOLE session's
        ray count, the handle plans it as one rank would and launches its slice of every crystal entry's share (host_shard_slice).  Not inside
        a session; BackendError for what sharding refuses."""
        self._check(self._L.halo_set_shard(self._h, int(index), int(count)))

    def fixed_words(self, planes=None):
        """Words halo_export_fixed writes for the current render: planes * W * H + 1 (planes: default the last session's plane count)."""
        n = self.last_route().plane_cnt if planes is None else int(planes)
        return n * self._render.width * self._render.height + 1

    def export_fixed(self, out):
        """MOVE the pending fixed-point planes of this handle's deterministic sessions into device memory: `out` is a torch.int64 device tensor of
        fixed_words() elements (anything with data_ptr() and numel()) or a (device pointer, n_words) pair.  Words [p * W * H, (p + 1) * W * H)
        are plane p in pixel order, the last word the landed integer nobody has taken yet.  The planes are left zero and not pending, the
        landed integer taken.  Returns (plane_cnt, frac_bits, landed_frac_bits).  Waits for the device."""
        ptr, n = (out.data_ptr(), out.numel()) if hasattr(out, "data_ptr") else (int(out[0]), int(out[1]))
        pc, f, fl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._check(self._L.halo_export_fixed(self._h, C.c_void_p(ptr), n, C.byref(pc), C.byref(f), C.byref(fl)))
        return pc.value, f.value, fl.value

    def import_fixed(self, words, plane_cnt, frac_bits, landed_frac_bits, rays):
        """ADD exported words (a torch.int64 device tensor or a (device pointer, n_words) pair; e.g. the integer sum of every shard's export) into
        the planes of this handle's last deterministic session, modulo 2^64, in stream order; the planes become pending, the landed word joins
        the handle's untaken landed integer, `rays` count against the 2^30-ray budget.  flush() / ReadbackXyzAccum() then fold as after the
        handle's own session.  BackendError for a layout that is not the handle's."""
        ptr, n = (words.data_ptr(), words.numel()) if hasattr(words, "data_ptr") else (int(words[0]), int(words[1]))
        self._check(self._L.halo_import_fixed(self._h, C.c_void_p(ptr), n, int(plane_cnt), int(frac_bits), int(landed_frac_bits), int(rays)))

    # --- the seam (trace_backend.hpp:374-632) ---
    def SupportsDeviceXyzAccum(self):
        return True

    def SupportsThirdClockDrain(self):
        return True

    def BeginSession(self, scene, render, wl, ray_num=0):
        self._render = render
        self._scene = scene
        self._lanes_shape = None   # the session's lanes take the render's size
        self._check(self._L.halo_begin(self._h, C.byref(scene), C.byref(render), C.byref(wl), int(ray_num)))

    def BeginSpectrumSession(self, scene, render, wls, ray_num=0):
        """One session for a whole discrete spectrum (halo_begin_spectrum): `wls` is a sequence of 1..255 discrete abi.HaloWl.  Root r of a crystal
        entry's share of m roots takes entry min(r // ceil(m / len(wls)), len(wls) - 1) — blocks of consecutive roots, no draw; everything after
        BeginSession (TraceLayer, Recombine, EndSession, readbacks) is the same.  One entry is that wavelength's discrete session."""
        wls = list(wls)
        arr = (abi.HaloWl * max(1, len(wls)))(*wls)
        self._render = render
        self._scene = scene
        self._lanes_shape = None
        self._check(self._L.halo_begin_spectrum(self._h, C.byref(scene), C.byref(render), arr, len(wls), int(ray_num)))

    def TraceLayer(self, count=0, host_rays=None):
        """First layer: `count` self-generated roots, or injected crystal-local rays (d, p, w, tf arrays).
        Later layers: consumes the continuation from Recombine.  Returns HaloLayerStats."""
        stats = abi.HaloLayerStats()
        if host_rays is None:
            self._check(self._L.halo_trace_layer(self._h, int(count), None, C.byref(stats)))
            self._pending_roots += int(stats.root_count)
            return stats
        d, p, w, tf = (np.ascontiguousarray(host_rays[0], np.float32), np.ascontiguousarray(host_rays[1], np.float32),
                       np.ascontiguousarray(host_rays[2], np.float32), np.ascontiguousarray(host_rays[3], np.uint32))
        n = w.shape[0]
        crystal = host_rays[4] if len(host_rays) > 4 else None      # HostRayBatch::crystal: an abi.HaloGeomTables, or None = the entry's own
        hr = abi.HaloHostRays(d.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_float)),
                              w.ctypes.data_as(C.POINTER(C.c_float)), tf.ctypes.data_as(C.POINTER(C.c_uint32)),
                              C.cast(C.pointer(crystal), C.c_void_p) if crystal is not None else None)
        self._check(self._L.halo_trace_layer(self._h, n, C.byref(hr), C.byref(stats)))
        self._pending_roots += int(stats.root_count)
        return stats

    def Recombine(self, shuffle=True):
        n = C.c_uint64()
        self._check(self._L.halo_recombine(self._h, 1 if shuffle else 0, C.byref(n)))
        return n.value

    def DrainExits(self, max_records=None):
        """Captured exit records since the last drain (only with option capture_exits=1); destructive.  With max_records the
        drain is piecewise: at most that many records now, the rest stays pending (halo_drain_exits)."""
        n = C.c_uint64()
        self._check(self._L.halo_drain_exits(self._h, None, 0, C.byref(n)))   # pending count, nothing consumed
        take = n.value if max_records is None else min(n.value, int(max_records))
        buf = (abi.HaloExitRecord * max(1, int(take)))()
        if take:
            self._check(self._L.halo_drain_exits(self._h, buf, int(take), C.byref(n)))
            take = n.value
        self._pending_roots = 0
        return np.frombuffer(buf, dtype=EXIT_DTYPE, count=int(take)).copy()

    def ReadbackXyzAccum(self, width=None, height=None):
        """Returns (xyz[H,W,3] float32, landed_weight float64) and zeroes the device accumulator."""
        w, h = (width or self._render.width), (height or self._render.height)
        img = np.empty((h, w, 3), np.float32)
        landed = C.c_double()
        self._check(self._L.halo_readback_xyz64(self._h, img.ctypes.data_as(C.POINTER(C.c_float)), w, h, C.byref(landed)))
        return img, landed.value

    def EndSession(self):
        self._check(self._L.halo_end(self._h))

    # --- consumer on device (RenderConsumer, reference src/server/render.cpp) ---
    def ConsumeDeviceFused(self):
        """Fold the device accumulator into the Neumaier running image and zero it (render.cpp:138-201)."""
        self._check(self._L.halo_consumer_fold(self._h))

    def Consume(self, xyz, landed, lanes=None):
        """RenderConsumer::ConsumeDeviceFused(const SimData&) for a drained image the caller holds: xyz float32[H,W,3] is Neumaier-folded
        into the running image, `landed` added to the total intensity, lanes float32[classes,H,W] (optional) added to the class lanes."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        h, w = xyz.shape[0], xyz.shape[1]
        lp, nc = None, 0
        if lanes is not None:
            lanes = np.ascontiguousarray(lanes, np.float32)
            lp, nc = lanes.ctypes.data_as(C.POINTER(C.c_float)), lanes.shape[0]
        self._check(self._L.halo_consumer_consume(self._h, xyz.ctypes.data_as(C.POINTER(C.c_float)), w, h, float(landed), lp, nc))
        self._cons_size = (w, h)

    def AutoEv(self, downsample=8, target_white=135.0):
        """The reference GUI's Adaptive Brightness anchor on the device consumer (halo_consumer_auto_ev: gui_ev_auto.hpp ComputeP99Y over the
        `downsample`-times coarser box sums of Y, ComputeEvAuto against the per-pixel landed intensity).  Returns a dict: p99_y (fine-equivalent),
        per_pixel_intensity, ev_auto (stops in [-6, 6]; 0 without data), produced (False = "auto: no data"), value_count, coarse_w, coarse_h
        (0, 0 = the fine path).  Reads the consumer only; apply it with Snapshot(intensity_factor=factor * 2 ** ev_auto) or Snapshot(auto_ev=True)."""
        r = abi.HaloAutoEv()
        self._check(self._L.halo_consumer_auto_ev(self._h, int(downsample), float(target_white), C.byref(r)))
        return {"p99_y": r.p99_y, "per_pixel_intensity": r.per_pixel_intensity, "ev_auto": r.ev_auto, "produced": bool(r.produced),
                "value_count": int(r.value_count), "coarse_w": int(r.coarse_w), "coarse_h": int(r.coarse_h)}

    def ImageStats(self, percentiles=abi.STATS_TOOL_PERCENTILES, plane=None, norm=None):
        """Exact percentiles and moments of the positive values of the consumer's Y (plane=None) or of class lane `plane`, computed where the
        image lies (halo_consumer_stats).  percentiles: up to 16 numbers in [0, 100], numpy's default interpolation; norm: the divisor of the
        normalised view and of the saturation test (None: the per-pixel intensity, as AutoEv reports it).  Returns a dict with the raw fields
        (pixel_count, positive_count, saturated_count, sum, sum_sq, max_raw, norm, produced, rank, lo, hi, frac, value — lists in the order
        asked) and the view the reference's stats tool prints, every value divided by norm: percentiles (a list), mean, std (population, from the
        exact sums), cv, max, saturation_rate = saturated / positive, non_zero_count.  Without a positive value, or without landed intensity
        when norm is None, produced is False and the view is all zeros, like the tool's.  Reads the consumer only."""
        pct = [float(p) for p in percentiles]
        if len(pct) > abi.STATS_MAX_PERCENTILES:
            raise ValueError("at most %d percentiles per call" % abi.STATS_MAX_PERCENTILES)
        spec, r = abi.HaloStatsSpec(), abi.HaloImageStats()
        spec.plane = abi.STATS_PLANE_Y if plane is None else int(plane)
        spec.percentile_count = len(pct)
        for j, p in enumerate(pct):
            spec.percentiles[j] = p
        spec.norm = 0.0 if norm is None else float(norm)
        self._check(self._L.halo_consumer_stats(self._h, C.byref(spec), C.byref(r)))
        k, n, nm = len(pct), int(r.positive_count), float(r.norm)
        out = {"pixel_count": int(r.pixel_count), "positive_count": n, "non_zero_count": n, "saturated_count": int(r.saturated_count),
               "sum": r.sum, "sum_sq": r.sum_sq, "max_raw": r.max, "norm": r.norm, "produced": bool(r.produced),
               "rank": [int(r.rank[j]) for j in range(k)], "lo": [r.lo[j] for j in range(k)], "hi": [r.hi[j] for j in range(k)],
               "frac": [r.frac[j] for j in range(k)], "value": [r.value[j] for j in range(k)]}
        if r.produced:
            mean = r.sum / n
            var = max(r.sum_sq / n - mean * mean, 0.0)
            std = math.sqrt(var) if math.isfinite(var) else float("nan")
            out.update(percentiles=[r.value[j] / nm for j in range(k)], mean=mean / nm, std=std / nm, cv=std / mean if mean > 0.0 else 0.0,
                       max=r.max / nm, saturation_rate=r.saturated_count / n)
        else:
            out.update(percentiles=[0.0] * k, mean=0.0, std=0.0, cv=0.0, max=0.0, saturation_rate=0.0)
        return out

    def Snapshot(self, intensity_factor=1.0, ray_color=(-1.0, -1.0, -1.0), background=(0.0, 0.0, 0.0), want_xyz=True, auto_ev=False, target_white=135.0):
        """PrepareSnapshot + PostSnapshot: returns (rgb uint8[H,W,3], xyz float32[H,W,3] | None, total_intensity).  auto_ev=True: the image is
        exposed with intensity_factor * 2 ** ev_auto (AutoEv(8, target_white)) and the EV comes back as a FOURTH value; without it the
        three-tuple is what it always was."""
        if auto_ev:
            ev = self.AutoEv(8, target_white)["ev_auto"]
            return self.Snapshot(float(intensity_factor) * 2.0 ** ev, ray_color, background, want_xyz) + (ev,)
        w, h = getattr(self, "_cons_size", None) or (self._render.width, self._render.height)
        d = abi.HaloDisplay(float(intensity_factor), (C.c_float * 3)(*ray_color), (C.c_float * 3)(*background))
        rgb = np.empty((h, w, 3), np.uint8)
        xyz = np.empty((h, w, 3), np.float32) if want_xyz else None
        tot = C.c_double()
        self._check(self._L.halo_consumer_snapshot(self._h, C.byref(d), rgb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   xyz.ctypes.data_as(C.POINTER(C.c_float)) if want_xyz else None, C.byref(tot)))
        return rgb, xyz, tot.value

    def View(self, view, source=None, intensity_factor=1.0, ray_color=(-1.0, -1.0, -1.0), background=(0.0, 0.0, 0.0), want=("rgb",), filter="nearest", blend=False):
        """The consumer's image through another lens (halo_consumer_view): `view` is a HaloRender (scenes.render) to look through, `source` the
        render the image was accumulated under (None: this handle's last session's).  Per view pixel the direction of its centre under the view's
        lens, the source pixel that direction lands on, that pixel's raw XYZ and its display transform — a gather on the device, no ray is traced.
        want: any of "rgb" (uint8[H,W,3]), "xyz" (float32[H,W,3]), "map" (int32[H,W]: row-major source pixel, -1 for none), "dir"
        (float32[H,W,3]: world exit direction, zeros for none); returns a dict of the arrays asked for.  The display arguments are Snapshot's
        (an automatic exposure is the CONSUMER's: intensity_factor * 2 ** AutoEv()["ev_auto"]).
        filter="bilinear": four taps around the continuous source position instead of the copy; blend=True: a dual-fisheye source's overlap band is
        cross-faded in as the reference's preview does; want may then name "tap" (float32[H,W,5]: fx0, fy0, fx1, fy1, t — what the values were
        made from).  Any of the three makes the call halo_consumer_view_filtered; the defaults are halo_consumer_view and its bytes."""
        unknown = set(want) - {"rgb", "xyz", "map", "dir", "tap"}
        if unknown:
            raise ValueError("View: unknown output %r" % sorted(unknown))
        if filter not in abi.VIEW_FILTERS:
            raise ValueError("View: unknown filter %r (nearest | bilinear)" % (filter,))
        filtered = filter != "nearest" or bool(blend) or "tap" in want
        spec = abi.HaloViewSpec()
        spec.view = view
        spec.has_source = 0 if source is None else 1
        if source is not None:
            spec.source = source
        spec.display = abi.HaloDisplay(float(intensity_factor), (C.c_float * 3)(*ray_color), (C.c_float * 3)(*background))
        h, w = max(int(view.height), 0), max(int(view.width), 0)
        big = w * h > 1 << 25   # (refused by the library: nothing of that size is allocated here)
        shapes = {"rgb": ((h, w, 3), np.uint8), "xyz": ((h, w, 3), np.float32), "map": ((h, w), np.int32), "dir": ((h, w, 3), np.float32),
                  "tap": ((h, w, 5), np.float32)}
        out = {k: np.empty((0,) if big else shapes[k][0], shapes[k][1]) for k in want}

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        if filtered:
            f = abi.HaloViewFilter(abi.VIEW_FILTERS[filter], 1 if blend else 0)
            self._check(self._L.halo_consumer_view_filtered(self._h, C.byref(spec), C.byref(f), ptr("rgb", C.c_uint8), ptr("xyz", C.c_float), ptr("map", C.c_int32),
                                                            ptr("dir", C.c_float), ptr("tap", C.c_float)))
        else:
            self._check(self._L.halo_consumer_view(self._h, C.byref(spec), ptr("rgb", C.c_uint8), ptr("xyz", C.c_float), ptr("map", C.c_int32), ptr("dir", C.c_float)))
        return out

    def ResetConsumer(self):
        self._check(self._L.halo_consumer_reset(self._h))

    # --- display-side composite of the class lanes (reference src/server/component_compositor.cpp) ---
    def LoadClassLanes(self, lanes, total_intensity=-1.0):
        """Replace the device lanes with (class_count, H, W) float32 host values (lanes summed over ranks, a saved consumer);
        total_intensity >= 0 replaces the consumer's total intensity too."""
        lanes = np.ascontiguousarray(lanes, np.float32)
        n, h, w = lanes.shape
        self._check(self._L.halo_consumer_load_lanes(self._h, lanes.ctypes.data_as(C.POINTER(C.c_float)), w, h, n, float(total_intensity)))
        self._lanes_shape = (n, h, w)

    def CompositeColorClasses(self, classes, mode="painter", display_exposure_scale=1.0, intensity_factor=1.0, want_srgb=True):
        """CompositeColorClassesLinear + LinearRgbToSrgbU8 on the device lanes (which stay).  Returns (produced, linear_rgb[H,W,3]
        float32, srgb[H,W,3] uint8 | None, participating_p99_y)."""
        n, h, w = getattr(self, "_lanes_shape", None) or (getattr(self, "_n_classes", 0), self._render.height, self._render.width)
        spec = abi.composite(classes, mode, display_exposure_scale, intensity_factor)
        lin = np.zeros((h, w, 3), np.float32)
        srgb = np.zeros((h, w, 3), np.uint8) if want_srgb else None
        p99, produced = C.c_float(-1.0), C.c_int32(0)
        self._check(self._L.halo_consumer_composite(self._h, C.byref(spec), lin.ctypes.data_as(C.POINTER(C.c_float)),
                                                    srgb.ctypes.data_as(C.POINTER(C.c_uint8)) if want_srgb else None, C.byref(p99), C.byref(produced)))
        return bool(produced.value), lin, srgb, p99.value

    def _lane_view_spec(self, who, view, source, filter, want, known):
        unknown = set(want) - set(known)
        if unknown:
            raise ValueError("%s: unknown output %r" % (who, sorted(unknown)))
        if filter not in abi.VIEW_FILTERS:
            raise ValueError("%s: unknown filter %r (nearest | bilinear)" % (who, filter))
        spec = abi.HaloViewSpec()
        spec.view = view
        spec.has_source = 0 if source is None else 1
        if source is not None:
            spec.source = source
        h, w = max(int(view.height), 0), max(int(view.width), 0)
        return spec, h, w

    def ViewComposite(self, view, classes, mode="painter", display_exposure_scale=1.0, intensity_factor=1.0, source=None, filter="nearest", blend=False, want=("srgb",)):
        """The class composite through another lens (halo_consumer_view_composite): CompositeColorClasses' image of the device lanes — `classes`,
        `mode` and the two factors are its arguments — gathered as View gathers the consumer's image, the way the reference's preview shows it in
        RGB mode.  `source` is the render the LANES lie under (None: this handle's last session's).  want: any of "srgb" (uint8[H,W,3]), "value"
        (float32[H,W,3]: the sampled value in byte units, srgb = floor(value + 0.5)), "map" (int32[H,W]) and "tap" (float32[H,W,5]), View's.
        Returns a dict of the arrays asked for plus "produced" (bool) and "p99" (float), CompositeColorClasses' two: with produced False "srgb" is
        None (no composite) and "value" is zeros.  The lanes stay as they are."""
        spec, h, w = self._lane_view_spec("ViewComposite", view, source, filter, want, ("srgb", "value", "map", "tap"))
        comp = abi.composite(classes, mode, display_exposure_scale, intensity_factor)
        big = w * h > 1 << 25   # (refused by the library: nothing of that size is allocated here)
        shapes = {"srgb": ((h, w, 3), np.uint8), "value": ((h, w, 3), np.float32), "map": ((h, w), np.int32), "tap": ((h, w, 5), np.float32)}
        out = {k: np.zeros((0,) if big else shapes[k][0], shapes[k][1]) for k in want}

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        f = abi.HaloViewFilter(abi.VIEW_FILTERS[filter], 1 if blend else 0)
        p99, produced = C.c_float(0.0), C.c_int32(0)
        self._check(self._L.halo_consumer_view_composite(self._h, C.byref(spec), C.byref(f), C.byref(comp), ptr("srgb", C.c_uint8), ptr("value", C.c_float),
                                                         ptr("map", C.c_int32), ptr("tap", C.c_float), C.byref(p99), C.byref(produced)))
        if not produced.value and "srgb" in out:
            out["srgb"] = None
        out["produced"], out["p99"] = bool(produced.value), p99.value
        return out

    def ViewLanes(self, view, source=None, filter="nearest", blend=False, want=("lanes",)):
        """The class lanes through another lens (halo_consumer_view_lanes): "lanes" float32[classes, H, W] — per class the same sample of the raw
        lane, no exposure, no composite — "map" and "tap" as ViewComposite's.  Returns a dict of the arrays asked for.  The lanes stay."""
        spec, h, w = self._lane_view_spec("ViewLanes", view, source, filter, want, ("lanes", "map", "tap"))
        n = getattr(self, "_n_classes", 0)   # (set_color's: the library's lane count)
        big = w * h > 1 << 25 or n * w * h > 1 << 27
        shapes = {"lanes": ((n, h, w), np.float32), "map": ((h, w), np.int32), "tap": ((h, w, 5), np.float32)}
        out = {k: np.zeros((0,) if big else shapes[k][0], shapes[k][1]) for k in want}

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        f = abi.HaloViewFilter(abi.VIEW_FILTERS[filter], 1 if blend else 0)
        self._check(self._L.halo_consumer_view_lanes(self._h, C.byref(spec), C.byref(f), ptr("lanes", C.c_float), ptr("map", C.c_int32), ptr("tap", C.c_float)))
        return out

    def ViewOverlay(self, view, overlay, source=None, intensity_factor=1.0, ray_color=(-1.0, -1.0, -1.0), background=(0.0, 0.0, 0.0), filter="nearest", blend=False,
                    want=("rgb",)):
        """View's image with the auxiliary lines on it (halo_consumer_view_overlay): `overlay` is an abi.HaloViewOverlay (view_overlay makes one) —
        horizon, altitude / azimuth grid, circles around the sun, zenith and nadir rings, a sun marker, drawn on the device from the direction of each
        view pixel.  The other arguments are View's.  want: any of "rgb" (uint8[H,W,3]), "value" (float32[H,W,3]: the colour after the last layer in
        byte units, rgb = floor(clamp(value) + 0.5)), "sky" (float32[H,W,6]: alt, az, dist and their pixel footprints, degrees), "marks" (float32[3,3]:
        x, y, present of zenith, nadir, sun in view pixels), "map" and "dir" (View's).  Returns a dict of the arrays asked for."""
        unknown = set(want) - {"rgb", "value", "sky", "marks", "map", "dir"}
        if unknown:
            raise ValueError("ViewOverlay: unknown output %r" % sorted(unknown))
        if filter not in abi.VIEW_FILTERS:
            raise ValueError("ViewOverlay: unknown filter %r (nearest | bilinear)" % (filter,))
        spec = abi.HaloViewSpec()
        spec.view = view
        spec.has_source = 0 if source is None else 1
        if source is not None:
            spec.source = source
        spec.display = abi.HaloDisplay(float(intensity_factor), (C.c_float * 3)(*ray_color), (C.c_float * 3)(*background))
        h, w = max(int(view.height), 0), max(int(view.width), 0)
        big = w * h > 1 << 25   # (refused by the library: nothing of that size is allocated here)
        shapes = {"rgb": ((h, w, 3), np.uint8), "value": ((h, w, 3), np.float32), "sky": ((h, w, 6), np.float32), "map": ((h, w), np.int32),
                  "dir": ((h, w, 3), np.float32)}
        out = {k: np.zeros((3, 3) if k == "marks" else (0,) if big else shapes[k][0], np.float32 if k == "marks" else shapes[k][1]) for k in want}

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        f = abi.HaloViewFilter(abi.VIEW_FILTERS[filter], 1 if blend else 0)
        self._check(self._L.halo_consumer_view_overlay(self._h, C.byref(spec), C.byref(f), C.byref(overlay), ptr("rgb", C.c_uint8), ptr("value", C.c_float),
                                                       ptr("sky", C.c_float), ptr("marks", C.c_float), ptr("map", C.c_int32), ptr("dir", C.c_float)))
        return out

    def ViewCompositeOverlay(self, view, overlay, classes, mode="painter", display_exposure_scale=1.0, intensity_factor=1.0, source=None, filter="nearest", blend=False,
                             want=("srgb",)):
        """ViewComposite's image with ViewOverlay's lines on it (halo_consumer_view_composite_overlay).  want: any of "srgb", "value" (the colour
        after the last layer), "sky", "marks", "map", "tap", "dir"; "produced" and "p99" as ViewComposite gives them: with produced False "srgb" is
        None and nothing is drawn."""
        spec, h, w = self._lane_view_spec("ViewCompositeOverlay", view, source, filter, want, ("srgb", "value", "sky", "marks", "map", "tap", "dir"))
        comp = abi.composite(classes, mode, display_exposure_scale, intensity_factor)
        big = w * h > 1 << 25   # (refused by the library: nothing of that size is allocated here)
        shapes = {"srgb": ((h, w, 3), np.uint8), "value": ((h, w, 3), np.float32), "sky": ((h, w, 6), np.float32), "map": ((h, w), np.int32),
                  "tap": ((h, w, 5), np.float32), "dir": ((h, w, 3), np.float32)}
        out = {k: np.zeros((3, 3) if k == "marks" else (0,) if big else shapes[k][0], np.float32 if k == "marks" else shapes[k][1]) for k in want}

        def ptr(k, t):
            return out[k].ctypes.data_as(C.POINTER(t)) if k in out else None
        f = abi.HaloViewFilter(abi.VIEW_FILTERS[filter], 1 if blend else 0)
        p99, produced = C.c_float(0.0), C.c_int32(0)
        self._check(self._L.halo_consumer_view_composite_overlay(self._h, C.byref(spec), C.byref(f), C.byref(comp), C.byref(overlay), ptr("srgb", C.c_uint8),
                                                                 ptr("value", C.c_float), ptr("sky", C.c_float), ptr("marks", C.c_float), ptr("map", C.c_int32),
                                                                 ptr("tap", C.c_float), ptr("dir", C.c_float), C.byref(p99), C.byref(produced)))
        if not produced.value and "srgb" in out:
            out["srgb"] = None
        out["produced"], out["p99"] = bool(produced.value), p99.value
        return out


def view_overlay(fov, sun_alt_az=None, layers=(), circles=None, grid_step=None):
    """An abi.HaloViewOverlay with the reference's defaults (halo_host_view_overlay_defaults; no device needed) for a view of `fov` degrees and the
    sun at sun_alt_az = (altitude, azimuth) degrees (None: the zenith).  layers: names of abi.VIEW_OVERLAY_LAYERS to switch on (horizon, grid,
    circles, zenith, sun); circles: the angular distances from the sun (default 22, 46); grid_step: degrees (default: by the field of view)."""
    o = abi.HaloViewOverlay()
    sun = None if sun_alt_az is None else (C.c_float * 2)(float(sun_alt_az[0]), float(sun_alt_az[1]))
    size = load_library().halo_host_view_overlay_defaults(float(fov), sun, C.byref(o))
    if size != C.sizeof(abi.HaloViewOverlay):
        raise BackendError("HaloViewOverlay is %d bytes in the library, %d here" % (size, C.sizeof(abi.HaloViewOverlay)))
    for name in layers:
        if name not in abi.VIEW_OVERLAY_LAYERS:
            raise ValueError("view_overlay: unknown layer %r (%s)" % (name, " | ".join(abi.VIEW_OVERLAY_LAYERS)))
        setattr(o, abi.VIEW_OVERLAY_LAYERS[name], 1)
    if circles is not None:
        circles = [float(v) for v in circles]
        if len(circles) > abi.VIEW_MAX_SUN_CIRCLES:
            raise ValueError("view_overlay: at most %d sun circles" % abi.VIEW_MAX_SUN_CIRCLES)
        o.sun_circle_count = len(circles)
        for i in range(abi.VIEW_MAX_SUN_CIRCLES):
            o.sun_circle_deg[i] = circles[i] if i < len(circles) else 0.0
    if grid_step is not None:
        o.grid_step_deg = float(grid_step)
    return o


def host_view_sky(direction, sun_dir):
    """halo_host_view_sky: float32[3] = altitude, azimuth, angular distance from the sun (degrees) of the travel direction `direction`, by the
    overlay's own code on the host (no device needed)."""
    d, s = np.ascontiguousarray(direction, np.float32), np.ascontiguousarray(sun_dir, np.float32)
    sky = np.zeros(3, np.float32)
    f32p = C.POINTER(C.c_float)
    load_library().halo_host_view_sky(d.ctypes.data_as(f32p), s.ctypes.data_as(f32p), sky.ctypes.data_as(f32p))
    return sky


def host_view_overlay_pixel(base_rgb, sky6, pixel_xy, marks, overlay):
    """halo_host_view_overlay_pixel: float32[3], the colour in byte units after the last layer of one pixel that has a direction (no device needed)."""
    b = np.ascontiguousarray(base_rgb, np.uint8)
    s, xy, m = (np.ascontiguousarray(v, np.float32).reshape(-1) for v in (sky6, pixel_xy, marks))
    v = np.zeros(3, np.float32)
    f32p = C.POINTER(C.c_float)
    if not load_library().halo_host_view_overlay_pixel(b.ctypes.data_as(C.POINTER(C.c_uint8)), s.ctypes.data_as(f32p), xy.ctypes.data_as(f32p), m.ctypes.data_as(f32p),
                                                       C.byref(overlay), v.ctypes.data_as(f32p)):
        raise ValueError("host_view_overlay_pixel: refused (a circle count outside 0 .. 16)")
    return v


def host_view_direction(view, px, py):
    """halo_host_view_direction: (has a direction, float32[3]) of pixel (px, py) of the HaloRender `view`, by the view stage's own code on the host
    (no device needed)."""
    d = np.zeros(3, np.float32)
    ok = load_library().halo_host_view_direction(C.byref(view), int(px), int(py), d.ctypes.data_as(C.POINTER(C.c_float)))
    return bool(ok), d


def host_spectrum_entry(m, count, r):
    """halo_host_spectrum_entry: the spectrum entry of root r among the m roots of a crystal entry's share, `count` entries (no device needed)."""
    return int(load_library().halo_host_spectrum_entry(int(m), int(count), int(r)))


def host_shard_slice(share, clock, index, count):
    """halo_host_shard_slice: (first, n) — the rays shard `index` of `count` takes of a crystal entry's share of `share` rays, cut in units of
    `clock` rays (no device needed).  ValueError for arguments the library refuses."""
    first, n = C.c_uint64(), C.c_uint64()
    for name, v, top in (("share", share, 1 << 64), ("clock", clock, 1 << 32), ("index", index, 1 << 32), ("count", count, 1 << 32)):
        if not 0 <= int(v) < top:
            raise ValueError("host_shard_slice: %s = %r out of range" % (name, v))
    if load_library().halo_host_shard_slice(int(share), int(clock), int(index), int(count), C.byref(first), C.byref(n)) != abi.HALO_OK:
        raise ValueError("host_shard_slice: refused (clock %r, index %r, count %r)" % (clock, index, count))
    return first.value, n.value


def host_ev_auto(p99_y, per_pixel_intensity, target_white=135.0):
    """halo_host_ev_auto: ComputeEvAuto of the reference (gui_ev_auto.hpp:143-155) in fp32 (no device needed)."""
    return float(load_library().halo_host_ev_auto(float(p99_y), float(per_pixel_intensity), float(target_white)))


def host_fixed_frac_bits(max_w, hits):
    """halo_host_fixed_frac_bits: the scale F of a 64-bit fixed-point sum of up to `hits` addends of at most `max_w` (no device needed)."""
    return int(load_library().halo_host_fixed_frac_bits(float(max_w), int(hits)))


def host_ticket_size(total, seen, waves, lo, hi):
    """halo_host_ticket_size: the wave-passes a wave of a ticketed launch asks for, the kernel's own rule (no device needed)."""
    return int(load_library().halo_host_ticket_size(int(total), int(seen), int(waves), int(lo), int(hi)))


def host_ticket_groups():
    """halo_host_ticket_groups: the ranges, each with a counter, that a ticketed launch's wave-passes are cut into."""
    return int(load_library().halo_host_ticket_groups())


def host_ticket_range(all_passes, g):
    """halo_host_ticket_range: (first, n) of range g of a launch of all_passes wave-passes."""
    first, n = C.c_uint32(), C.c_uint32()
    load_library().halo_host_ticket_range(int(all_passes), int(g), C.byref(first), C.byref(n))
    return first.value, n.value


def host_ticket_next(open_mask, home):
    """halo_host_ticket_next: the range a wave at home on range `home` turns to, given the mask of ranges with passes left."""
    return int(load_library().halo_host_ticket_next(int(open_mask), int(home)))


EXIT_DTYPE = np.dtype([("dir", np.float32, 3), ("weight", np.float32), ("root", np.uint32), ("seq", np.uint16),
                       ("layer", np.uint8), ("path_len", np.uint8), ("path", np.uint8, abi.PATH_CAP),
                       ("pixel", np.int32), ("crystal_id", np.uint16), ("wl_idx", np.uint16), ("color_mask", np.uint64)])
assert EXIT_DTYPE.itemsize == C.sizeof(abi.HaloExitRecord)


def host_view_source_pos(source, direction):
    """halo_host_view_source_pos: (hit count, float32[5] = fx0, fy0, fx1, fy1, t) of the exit direction `direction` under the HaloRender `source`,
    by the filtered view's own code on the host (no device needed)."""
    d = np.ascontiguousarray(direction, np.float32)
    pos = np.zeros(5, np.float32)
    n = load_library().halo_host_view_source_pos(C.byref(source), d.ctypes.data_as(C.POINTER(C.c_float)), pos.ctypes.data_as(C.POINTER(C.c_float)))
    return int(n), pos
