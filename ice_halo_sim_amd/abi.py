"""ctypes mirror of include/halo_trace.h (the C-ABI boundary).  Plumbing only: no compute here.

Struct layouts follow the header field-for-field; `tests/test_abi_layout.py` checks sizes against the
compiled library (`halo_abi_sizeof`).
"""
import ctypes as C

HALO_OK, HALO_UNAVAILABLE, HALO_FATAL = 0, 1, 2
MAX_LAYERS, MAX_ENTRIES, MAX_HITS, MAX_FACES, MAX_FACE_VTX, MAX_TRIS = 4, 16, 64, 20, 12, 64
HALO_MAX_LAYERS, HALO_MAX_ENTRIES, HALO_MAX_HITS = MAX_LAYERS, MAX_ENTRIES, MAX_HITS
LUT_NODES, WL_POOL_MAX, PATH_CAP = 257, 255, 64

DIST_NONE, DIST_UNIFORM, DIST_GAUSS, DIST_ZIGZAG, DIST_LAPLACIAN, DIST_GAUSS_LEGACY = range(6)
CRYSTAL_PRISM, CRYSTAL_PYRAMID = 0, 1
(LENS_LINEAR, LENS_FISHEYE_EQUAL_AREA, LENS_FISHEYE_EQUIDISTANT, LENS_FISHEYE_STEREOGRAPHIC,
 LENS_DUAL_FISHEYE_EQUAL_AREA, LENS_DUAL_FISHEYE_EQUIDISTANT, LENS_DUAL_FISHEYE_STEREOGRAPHIC,
 LENS_RECTANGULAR, LENS_FISHEYE_ORTHOGRAPHIC, LENS_DUAL_FISHEYE_ORTHOGRAPHIC, LENS_GLOBE) = range(11)
VISIBLE_UPPER, VISIBLE_LOWER, VISIBLE_FULL = 0, 1, 2
ILLUM = {"D50": 0, "D55": 1, "D65": 2, "D75": 3, "A": 4, "E": 5}


class HaloDist(C.Structure):
    _fields_ = [("type", C.c_int32), ("center", C.c_float), ("spread", C.c_float)]


class HaloAxis(C.Structure):
    _fields_ = [("azimuth", HaloDist), ("latitude", HaloDist), ("roll", HaloDist)]


class HaloCrystal(C.Structure):
    _fields_ = [("kind", C.c_int32), ("height", HaloDist * 3), ("face_dist", HaloDist * 6),
                ("sync_group", C.c_int32 * 9), ("wedge_upper_deg", C.c_float), ("wedge_lower_deg", C.c_float)]


class HaloEntry(C.Structure):
    _fields_ = [("crystal", HaloCrystal), ("axis", HaloAxis), ("proportion", C.c_float),
                ("crystal_config_id", C.c_int32), ("filter_id", C.c_int32), ("color_id", C.c_int32)]


FILTER_MAX_OR, FILTER_MAX_TERMS = 64, 64
FILTER_NONE, FILTER_RAYPATH, FILTER_ENTRY_EXIT, FILTER_DIRECTION, FILTER_CRYSTAL = range(5)
SYM_P, SYM_B, SYM_D = 1, 2, 4


class HaloFilterTerm(C.Structure):
    _fields_ = [("type", C.c_int32), ("raypath_len", C.c_int32), ("raypath", C.c_uint8 * MAX_HITS), ("has_entry", C.c_int32),
                ("entry", C.c_int32), ("has_exit", C.c_int32), ("exit_face", C.c_int32), ("min_len", C.c_uint32),
                ("max_len", C.c_uint32), ("az", C.c_float), ("el", C.c_float), ("radii", C.c_float), ("crystal_id", C.c_int32)]


class HaloFilter(C.Structure):
    _fields_ = [("action", C.c_int32), ("symmetry", C.c_int32), ("is_complex", C.c_int32), ("or_count", C.c_int32),
                ("and_counts", C.c_int32 * FILTER_MAX_OR), ("terms", HaloFilterTerm * FILTER_MAX_TERMS)]


COLOR_MAX_TERMS, COLOR_MAX_CLASSES = 16, 16


class HaloColorTerm(C.Structure):
    _fields_ = [("predicate", HaloFilterTerm), ("symmetry", C.c_int32), ("bit", C.c_int32)]


class HaloColorSet(C.Structure):
    _fields_ = [("term_count", C.c_int32), ("reserved", C.c_int32), ("terms", HaloColorTerm * COLOR_MAX_TERMS)]


class HaloColorClass(C.Structure):
    _fields_ = [("bits", C.c_uint64), ("combine_all", C.c_int32), ("reserved", C.c_int32)]


class HaloLayer(C.Structure):
    _fields_ = [("prob", C.c_float), ("entry_count", C.c_int32), ("entries", HaloEntry * MAX_ENTRIES)]


class HaloScene(C.Structure):
    _fields_ = [("sun_altitude", C.c_float), ("sun_azimuth", C.c_float), ("sun_diameter", C.c_float),
                ("max_hits", C.c_int32), ("layer_count", C.c_int32), ("layers", HaloLayer * MAX_LAYERS)]


class HaloRender(C.Structure):
    _fields_ = [("lens_type", C.c_int32), ("fov", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("lens_shift", C.c_int32 * 2), ("view_az", C.c_float), ("view_el", C.c_float),
                ("view_ro", C.c_float), ("visible", C.c_int32), ("overlap", C.c_float)]


class HaloWl(C.Structure):
    _fields_ = [("wavelength", C.c_float), ("weight", C.c_float), ("illuminant", C.c_int32),
                ("pool_size", C.c_int32)]


class HaloHostRays(C.Structure):
    _fields_ = [("d", C.POINTER(C.c_float)), ("p", C.POINTER(C.c_float)), ("w", C.POINTER(C.c_float)),
                ("tf", C.POINTER(C.c_uint32)), ("crystal", C.c_void_p)]   # crystal: HaloGeomTables* or NULL


class HaloLayerStats(C.Structure):
    _fields_ = [("root_count", C.c_uint64), ("exit_count", C.c_uint64), ("continuation_count", C.c_uint64),
                ("exit_w_sum", C.c_double), ("kernel_ms", C.c_double), ("pixel_hits", C.c_uint64), ("launches", C.c_uint64)]


class HaloExitRecord(C.Structure):
    _fields_ = [("dir", C.c_float * 3), ("weight", C.c_float), ("root", C.c_uint32), ("seq", C.c_uint16),
                ("layer", C.c_uint8), ("path_len", C.c_uint8), ("path", C.c_uint8 * PATH_CAP),
                ("pixel", C.c_int32), ("crystal_id", C.c_uint16), ("wl_idx", C.c_uint16), ("color_mask", C.c_uint64)]


class HaloRouteInfo(C.Structure):
    _fields_ = [("launches", C.c_uint32), ("mode_mask", C.c_uint32), ("geom_mask", C.c_uint32), ("accum_mask", C.c_uint32),
                ("source_mask", C.c_uint32), ("plane_cnt", C.c_uint32), ("plane_copies", C.c_uint32), ("shuffle_chunk", C.c_uint32),
                ("spec_mask", C.c_uint32), ("generic_launches", C.c_uint32)]


MODE_PLAIN, MODE_FILTER, MODE_CAPTURE, MODE_GENERIC, MODE_COLOR = 1, 2, 4, 8, 16   # HaloRouteInfo.mode_mask bits
SPEC_LAST, SPEC_LENS, SPEC_VIS, SPEC_NOGATE = 1, 2, 4, 8                           # HaloRouteInfo.spec_mask bits
ROOT_GEN, ROOT_TRANSIT = 1, 2                                                      # halo_last_root_profile bits
CLOSE_AUTO, CLOSE_NEVER, CLOSE_ALWAYS = -1, 0, 1                                          # option "close_direct" (halo_direct_closes counts the launches it took)


ACCUM_XYZ, ACCUM_SCALAR, ACCUM_BIN1, ACCUM_BIN2, ACCUM_LOG, ACCUM_LOG_XYZ, ACCUM_NONE = 1, 2, 4, 8, 16, 32, 64   # HaloRouteInfo.accum_mask bits
ACCUM_FIXED = 128   # ... fixed-point planes (option "deterministic"): beside it ACCUM_NONE, and ACCUM_LOG or ACCUM_LOG_XYZ for launches that took the hit log's integer twins
FIX_BUDGET_RAYS = 1 << 30   # rays one unfolded fixed-point plane set takes: the longest run between two folds (or exchanges: halo_export_fixed / halo_import_fixed) that is exact
ACCUM_FIXED_LOG, ACCUM_FIXED_LOG_XYZ = ACCUM_FIXED | ACCUM_LOG, ACCUM_FIXED | ACCUM_LOG_XYZ   # a deterministic session whose launches were logged (scalar plane; X, Y, Z planes)


class HaloGeomTables(C.Structure):
    _fields_ = [("face_cnt", C.c_int32), ("face_n", C.c_float * (MAX_FACES * 3)), ("face_d", C.c_float * MAX_FACES),
                ("face_number", C.c_int32 * MAX_FACES), ("tri_cnt", C.c_int32), ("tri_v", C.c_float * (MAX_TRIS * 9)),
                ("tri_n", C.c_float * (MAX_TRIS * 3)), ("tri_area", C.c_float * MAX_TRIS),
                ("tri_face", C.c_int32 * MAX_TRIS)]


class HaloDisplay(C.Structure):
    _fields_ = [("intensity_factor", C.c_float), ("ray_color", C.c_float * 3), ("background", C.c_float * 3)]


class HaloAutoEv(C.Structure):
    """halo_consumer_auto_ev's result (reference gui/gui_ev_auto.hpp: ComputeP99Y + ComputeEvAuto)."""
    _fields_ = [("p99_y", C.c_float), ("per_pixel_intensity", C.c_float), ("ev_auto", C.c_float), ("produced", C.c_int32),
                ("value_count", C.c_uint32), ("coarse_w", C.c_int32), ("coarse_h", C.c_int32)]


STATS_MAX_PERCENTILES = 16
STATS_PLANE_Y = -1
# the eleven percentiles of the reference's scripts/dump_xyz_stats.py, and the keys it files them under
STATS_TOOL_PERCENTILES = (50.0, 70.0, 90.0, 95.0, 99.0, 99.3, 99.5, 99.7, 99.9, 99.95, 99.99)
STATS_TOOL_KEYS = ("p50", "p70", "p90", "p95", "p99", "p99_3", "p99_5", "p99_7", "p99_9", "p99_95", "p99_99")


class HaloStatsSpec(C.Structure):
    """What halo_consumer_stats is asked for: plane (STATS_PLANE_Y or a class lane), up to 16 percentiles, the saturation divisor (<= 0: the
    per-pixel intensity)."""
    _fields_ = [("plane", C.c_int32), ("percentile_count", C.c_int32), ("percentiles", C.c_double * STATS_MAX_PERCENTILES), ("norm", C.c_float),
                ("reserved", C.c_int32)]


class HaloImageStats(C.Structure):
    """halo_consumer_stats's result: counts, exact sums, max, and per percentile the lower rank, the two order statistics, the fraction between
    them and the interpolated value (numpy's default rule)."""
    _fields_ = [("pixel_count", C.c_uint64), ("positive_count", C.c_uint64), ("saturated_count", C.c_uint64), ("sum", C.c_double), ("sum_sq", C.c_double),
                ("max", C.c_float), ("norm", C.c_float), ("produced", C.c_int32), ("percentile_count", C.c_int32),
                ("rank", C.c_uint64 * STATS_MAX_PERCENTILES), ("lo", C.c_float * STATS_MAX_PERCENTILES), ("hi", C.c_float * STATS_MAX_PERCENTILES),
                ("frac", C.c_double * STATS_MAX_PERCENTILES), ("value", C.c_double * STATS_MAX_PERCENTILES)]


class HaloViewSpec(C.Structure):
    """What halo_consumer_view looks through: the view render, the render the consumer's image was accumulated under (has_source = 0: the
    handle's last session's), the snapshot's display transform."""
    _fields_ = [("view", HaloRender), ("has_source", C.c_int32), ("source", HaloRender), ("display", HaloDisplay)]


VIEW_NEAREST, VIEW_BILINEAR = 0, 1
VIEW_FILTERS = {"nearest": VIEW_NEAREST, "bilinear": VIEW_BILINEAR}


class HaloViewFilter(C.Structure):
    """halo_consumer_view_filtered's filter: VIEW_NEAREST | VIEW_BILINEAR, blend 0 | 1 (a dual-fisheye source's overlap band), two zero words."""
    _fields_ = [("filter", C.c_int32), ("blend", C.c_int32), ("reserved", C.c_int32 * 2)]


VIEW_MAX_SUN_CIRCLES = 16
VIEW_OVERLAY_LAYERS = {"horizon": "show_horizon", "grid": "show_grid", "circles": "show_sun_circles", "zenith": "show_zenith_nadir", "sun": "show_sun_marker"}


class HaloViewOverlay(C.Structure):
    """halo_consumer_view_overlay's record: the five layer switches, the grid step, the sun's travel direction, the sun circles' angles, per layer a
    colour and an alpha in [0, 1], the ring and marker radii in view pixels, two zero words.  halo_host_view_overlay_defaults fills the reference's."""
    _fields_ = [("show_horizon", C.c_int32), ("show_grid", C.c_int32), ("show_sun_circles", C.c_int32), ("show_zenith_nadir", C.c_int32),
                ("show_sun_marker", C.c_int32), ("grid_step_deg", C.c_float), ("sun_dir", C.c_float * 3), ("sun_circle_count", C.c_int32),
                ("sun_circle_deg", C.c_float * VIEW_MAX_SUN_CIRCLES),
                ("horizon_color", C.c_float * 3), ("horizon_alpha", C.c_float), ("grid_color", C.c_float * 3), ("grid_alpha", C.c_float),
                ("sun_circles_color", C.c_float * 3), ("sun_circles_alpha", C.c_float), ("zenith_nadir_color", C.c_float * 3), ("zenith_nadir_alpha", C.c_float),
                ("sun_marker_color", C.c_float * 3), ("sun_marker_alpha", C.c_float), ("zenith_nadir_radius_px", C.c_float), ("sun_marker_radius_px", C.c_float),
                ("reserved", C.c_int32 * 2)]


COMPOSITE_DOMINANT, COMPOSITE_ADDITIVE, COMPOSITE_PAINTER = 0, 1, 2


class HaloCompositeClass(C.Structure):
    """Display half of a ColorClass (reference config/color_class_table.hpp:21-35)."""
    _fields_ = [("color", C.c_float * 3), ("z_order", C.c_int32), ("visible", C.c_int32), ("solo", C.c_int32)]


class HaloComposite(C.Structure):
    _fields_ = [("mode", C.c_int32), ("display_exposure_scale", C.c_float), ("intensity_factor", C.c_float), ("class_count", C.c_int32),
                ("classes", HaloCompositeClass * COLOR_MAX_CLASSES)]


def composite(classes, mode="painter", display_exposure_scale=1.0, intensity_factor=1.0):
    """HaloComposite from [{"color": (r, g, b), "visible": True, "solo": False, "z_order": i}, ...] (z_order defaults to the list
    position, like BuildColorClassTable) and a mode name or HALO_COMPOSITE_* value."""
    names = {"dominant": COMPOSITE_DOMINANT, "additive": COMPOSITE_ADDITIVE, "painter": COMPOSITE_PAINTER}
    spec = HaloComposite()
    spec.mode = mode if isinstance(mode, int) else names.get(mode, COMPOSITE_PAINTER)   # ParseCompositeMode: unknown -> painter
    spec.display_exposure_scale = float(display_exposure_scale)
    spec.intensity_factor = float(intensity_factor)
    spec.class_count = len(classes)
    for i, c in enumerate(classes):
        k = spec.classes[i]
        k.color = (C.c_float * 3)(*[float(v) for v in c.get("color", (1.0, 1.0, 1.0))])
        k.z_order = int(c.get("z_order", i))
        k.visible = 1 if c.get("visible", True) else 0
        k.solo = 1 if c.get("solo", False) else 0
    return spec


class ProjParams(C.Structure):
    """lm_proj::ProjParams — reference src/core/shared/projection_shared.h:106-118 (76 bytes)."""
    _fields_ = [("proj_type", C.c_int32), ("img_w", C.c_int32), ("img_h", C.c_int32), ("visible_range", C.c_int32),
                ("lens_shift_x", C.c_int32), ("lens_shift_y", C.c_int32), ("scale", C.c_float), ("az0", C.c_float),
                ("r_scale", C.c_float), ("max_abs_dz", C.c_float), ("rot", C.c_float * 9)]


def dist(spec=None, default=0.0, default_spread=0.0):
    """HaloDist from a JSON-style value: number | {"type","mean","std"} (reference doc/configuration.md).
    An object overwrites only the keys it carries: a missing "mean" / "std" keeps the DESTINATION slot's seeded value
    (`default` / `default_spread`), exactly like from_json(Distribution&) (reference src/core/math.cpp:593-630) — e.g. axis
    roll is seeded uniform / 0 / 360 (math.cpp:692-714), so {"type": "uniform"} there means a full turn, not spread 0."""
    d = HaloDist()
    if spec is None:
        d.type, d.center, d.spread = DIST_NONE, float(default), 0.0
    elif isinstance(spec, (int, float)):
        d.type, d.center, d.spread = DIST_NONE, float(spec), 0.0
    elif isinstance(spec, HaloDist):
        return spec
    else:
        names = {"none": DIST_NONE, "uniform": DIST_UNIFORM, "gauss": DIST_GAUSS, "zigzag": DIST_ZIGZAG,
                 "laplacian": DIST_LAPLACIAN, "gauss_legacy": DIST_GAUSS_LEGACY}
        d.type = names[spec["type"]]
        d.center = float(spec.get("mean", default))
        d.spread = float(spec.get("std", default_spread))
    return d
