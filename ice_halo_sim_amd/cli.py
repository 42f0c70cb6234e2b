"""Command-line front end for the HIP trace backend: run a Lumice JSON config through the path and, with --benchmark,
print the reference's one-line `[BENCHMARK] {json}` record (reference src/main.cpp:342-573; rate definition
doc/performance-testing.md:86-131: Σ root rays over wavelengths / steady seconds, setup excluded).

  python -m ice_halo_sim_amd.cli -f examples/config_example.json --render 4 --benchmark
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

from . import abi, config
from .backend import BackendError, BackendUnavailableError, HipTraceBackend

DISPATCH_RAYS = 1 << 26  # rays per TraceLayer call (the reference's GPU dispatch is 2^18, server.cpp:151; we batch far larger)
DISPATCH_RAYS_MULTI = 1 << 24  # ... for scenes with more than one scattering layer: the continuation pools are sized for roots x max_hits,
                               # and a one-shot CLI run pays for their allocation (64 Mi roots x 8 hits: two pools of 10 GB, 0.5 s of hipMalloc)


def run_job(job, render_id=None, seed=42, device=0, max_rays=None, progress=None, canonical_order=False, deterministic=False, spectrum_session=False, shard=None):
    """Trace `job` (config.TraceJob) on one GPU. Returns dict(rays, setup_sec, active_sec, backend, render).  canonical_order: option
    cont_order = 1 (the continuation pool of every layer but the last in (root, interaction) order).  deterministic: option deterministic = 1
    (fixed-point accumulation; with it a multi-layer document takes cont_order = 1 as well) — BackendError when the document needs what that
    route refuses.  spectrum_session: a document whose spectrum is a list of discrete wavelengths is traced as spectrum sessions
    (HipTraceBackend.BeginSpectrumSession) — one session chain per dispatch of len(wavelengths) x n rays, n rays of every wavelength in it —
    instead of one session per wavelength; ignored for an illuminant (which is one session already) and for a single wavelength.
    shard = (rank, world), with deterministic: this process is one rank of `world` (torch.distributed is initialised); the same sessions go
    through dist.ExactShardedTracer, the ranks' integer planes are exchanged where this function's one-rank run folds them, and rank 0 ends
    up with the one-rank run's consumer, bit for bit — the other ranks with an empty one."""
    if not job.renders:
        raise config.ConfigError("config has no render entry")
    rid = render_id if render_id is not None else sorted(job.renders)[0]  # the seam supports ONE renderer (simulator.cpp:937-944)
    render = job.renders[rid]
    t0 = time.perf_counter()
    tracer = None
    if shard is not None:
        from .dist import ExactShardedTracer
        tracer = ExactShardedTracer(job.scene, render, seed=seed, device=device, rank=shard[0], world=shard[1])
        be = tracer.backend
        be.set_shard(0, 1)   # the warm-up below is every rank's own, whole: the counters move as they do on one rank
    else:
        be = HipTraceBackend(device=device, seed=seed)
    if canonical_order or (deterministic and job.scene.layer_count > 1):
        be.set_option("cont_order", 1)
    if deterministic:
        be.set_option("deterministic", 1)
    if job.geom_clock:
        be.set_option("geom_clock", job.geom_clock)
    be.set_filters(job.filters)
    if job.color_classes:
        be.set_color(job.color_sets, job.color_classes)
    total = job.ray_num if job.ray_num is not None else (max_rays or 0)
    if max_rays is not None:
        total = min(total, max_rays)
    n_wl = max(1, len(job.wavelengths))
    per_wl = -(-total // n_wl)
    # warm-up pass outside the timed window: first launch pays module load / context init (main.cpp GPU warm-up pass)
    be.BeginSession(job.scene, render, job.wavelengths[0], 1024)
    be.TraceLayer(1024)
    be.EndSession()
    be.ReadbackXyzAccum()
    if job.color_classes:
        be.ReadbackClassLanes()   # the warm-up rays must not stay in the lanes
    if tracer is not None:
        be.set_shard(shard[0], shard[1])
    setup = time.perf_counter() - t0
    t1 = time.perf_counter()
    rays = 0
    spectrum = spectrum_session and len(job.wavelengths) > 1 and all(wl.illuminant < 0 for wl in job.wavelengths)
    left = per_wl if spectrum else 0
    while left > 0:   # spectrum sessions: every dispatch holds n rays of each wavelength, block by block within each crystal entry's share
        n = min(left, max(1, (DISPATCH_RAYS if job.scene.layer_count == 1 else DISPATCH_RAYS_MULTI) // n_wl))
        if tracer is not None:
            tracer.trace_session(list(job.wavelengths), n * n_wl)
        else:
            be.BeginSpectrumSession(job.scene, render, job.wavelengths, n * n_wl)
            for li in range(job.scene.layer_count):
                be.TraceLayer(n * n_wl if li == 0 else 0)
                if li + 1 < job.scene.layer_count:
                    be.Recombine(True)
            be.EndSession()
        left -= n
        rays += n * n_wl
        if left == 0:
            if tracer is not None:
                tracer.exchange()   # where the one-rank run folds its planes: the consumer's fold is a reader of the image
            be.ConsumeDeviceFused()  # drain window
        if progress:
            progress(rays)
    for wl in ([] if spectrum else job.wavelengths):
        left = per_wl
        while left > 0:
            n = min(left, DISPATCH_RAYS if job.scene.layer_count == 1 else DISPATCH_RAYS_MULTI)
            if tracer is not None:
                tracer.trace_session(wl, n)
            else:
                be.BeginSession(job.scene, render, wl, n)
                for li in range(job.scene.layer_count):
                    be.TraceLayer(n if li == 0 else 0)
                    if li + 1 < job.scene.layer_count:
                        be.Recombine(True)
                be.EndSession()
            left -= n
            rays += n
        if tracer is not None:
            tracer.exchange()
        be.ConsumeDeviceFused()  # drain window
        if progress:
            progress(rays)
    be.sync()
    active = time.perf_counter() - t1
    return {"rays": rays, "setup_sec": setup, "active_sec": active, "backend": be, "render": render, "render_id": rid}


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def write_image(path, rgb, fmt, quality):
    """stbi_write_jpg / stbi_write_png of main.cpp:262-273 (JPEG: quality as given, no chroma subsampling above 90 like stb)"""
    from PIL import Image
    if fmt == "png":
        Image.fromarray(rgb).save(path, "PNG")
    else:
        Image.fromarray(rgb).save(path, "JPEG", quality=int(quality), subsampling=0 if quality > 90 else 2)
    print("Saved: %s (%dx%d)" % (path, rgb.shape[1], rgb.shape[0]))


def exposure_factor(be, rid, factor, args):
    """--auto-ev: the config's intensity_factor times 2^ev_auto of the device consumer (HipTraceBackend.AutoEv: the reference GUI's Adaptive
    Brightness, P99 of the 8 x 8 box sums against the per-pixel landed intensity), and the line that says which EV was chosen."""
    if not args.auto_ev:
        return factor
    a = be.AutoEv(8, args.target_white)
    if a["produced"]:
        print("ev_auto (render %d): %+.2f EV (p99_y=%.6g, per_pixel_intensity=%.6g)" % (rid, a["ev_auto"], a["p99_y"], a["per_pixel_intensity"]))
    else:
        print("ev_auto (render %d): (auto: no data)" % rid)
    return factor * 2.0 ** a["ev_auto"]


def view_overlay(args, job, view):
    """--view-overlay: the HaloViewOverlay for `view`, or None.  The sun is the configuration's."""
    if not args.view_overlay:
        return None
    layers = [v.strip() for v in args.view_overlay.split(",") if v.strip()]
    unknown = [v for v in layers if v not in abi.VIEW_OVERLAY_LAYERS]
    if unknown:
        raise config.ConfigError("--view-overlay: unknown layer %r (horizon, grid, circles, zenith, sun)" % unknown[0])
    try:
        circles = [float(v) for v in args.view_circles.split(",")] if args.view_circles else None
        step = None if args.view_grid_step == "auto" else float(args.view_grid_step)
    except ValueError:
        raise config.ConfigError("--view-circles wants DEG,DEG,... and --view-grid-step auto or DEG")
    if circles is not None and len(circles) > abi.VIEW_MAX_SUN_CIRCLES:
        raise config.ConfigError("--view-circles: at most %d" % abi.VIEW_MAX_SUN_CIRCLES)
    from .backend import view_overlay as make
    return make(view.fov, (job.scene.sun_altitude, job.scene.sun_azimuth), layers, circles, step)


def view_render(args, source):
    """--out-view: the HaloRender to look through.  What is not given keeps the traced render's value (size, view direction, visible range,
    overlap) or the lens's usual field of view; the lens shift is none."""
    from . import scenes
    lens = config.LENS_NAMES[args.view_lens] if args.view_lens else source.lens_type
    if args.view_size:
        try:
            w, h = (int(v) for v in args.view_size.lower().split("x"))
        except ValueError:
            raise config.ConfigError("--view-size wants WxH, got %r" % args.view_size)
    else:
        w, h = source.width, source.height
    if args.view_fov is not None:
        fov = args.view_fov
    elif lens == source.lens_type:
        fov = source.fov
    else:
        fov = {abi.LENS_LINEAR: 90.0, abi.LENS_GLOBE: 60.0, abi.LENS_RECTANGULAR: 360.0}.get(lens, 180.0)
    pick = lambda v, d: d if v is None else v
    return scenes.render(lens, w, h, fov=fov, az=pick(args.view_az, source.view_az), el=pick(args.view_el, source.view_el), ro=pick(args.view_roll, source.view_ro),
                         visible=config.VISIBLE_NAMES[args.view_visible] if args.view_visible else source.visible,
                         overlap=pick(args.view_overlap, source.overlap))


def image_stats_record(be, config_path):
    """--stats: the per-scene record of the reference's scripts/dump_xyz_stats.py for the consumer's image — Y over the per-pixel intensity,
    the tool's eleven percentiles, mean / std / cv, max and the saturated share of the positive pixels — computed on the device
    (HipTraceBackend.ImageStats).  The tool's all-zero record when the image has no positive pixel."""
    s = be.ImageStats(abi.STATS_TOOL_PERCENTILES)
    return {"scene": os.path.splitext(os.path.basename(config_path))[0], "config": config_path, "pixel_count": s["pixel_count"],
            "non_zero_count": s["non_zero_count"], "percentiles": dict(zip(abi.STATS_TOOL_KEYS, s["percentiles"])), "mean": s["mean"], "std": s["std"],
            "cv": s["cv"], "max": s["max"], "saturation_rate": s["saturation_rate"]}


def save_all_renders(job, args):
    """`-f cfg -o dir [--format png] [--quality q]`: what the reference CLI leaves in the output directory (SaveRenderResults /
    SaveCompositeResults, main.cpp:251-315): img_<id>.<fmt> per render entry, img_<id>_components.<fmt> with raypath_color."""
    if not os.path.isdir(args.output_dir):   # the reference fails on an output directory that does not exist (test_errors.py: nonexistent output dir)
        print("Error: output directory does not exist: %s" % args.output_dir, file=sys.stderr)
        return 2
    if not job.renders:
        raise config.ConfigError("config has no render entry")
    rc = 0
    for rid in sorted(job.renders):
        try:
            res = run_job(job, rid, args.seed, args.device, args.max_rays, canonical_order=args.canonical_order, deterministic=args.deterministic,
                          spectrum_session=args.spectrum_session)
        except BackendUnavailableError as e:
            print("backend unavailable: %s" % e, file=sys.stderr)
            return 3
        except BackendError as e:
            if not args.deterministic:
                raise
            print("refused: %s" % e, file=sys.stderr)
            return 4
        be = res["backend"]
        meta = job.render_meta.get(rid, {})
        rgb, xyz, total_intensity = be.Snapshot(intensity_factor=exposure_factor(be, rid, meta.get("intensity_factor", 1.0), args),
                                                ray_color=meta.get("ray_color", (-1.0, -1.0, -1.0)),
                                                background=meta.get("background", (0.0, 0.0, 0.0)), want_xyz=args.deterministic)
        if args.deterministic:
            print("xyz sha256 (render %d): %s" % (rid, hashlib.sha256(xyz.tobytes()).hexdigest()))
        write_image(os.path.join(args.output_dir, "img_%02d.%s" % (rid, args.format)), rgb, args.format, args.quality)
        if job.color_classes:
            ok, _, srgb, p99 = be.CompositeColorClasses(job.color_meta, job.color_mode, 2.0 ** args.display_ev, meta.get("intensity_factor", 1.0))
            if ok:
                write_image(os.path.join(args.output_dir, "img_%02d_components.%s" % (rid, args.format)), srgb, args.format, args.quality)
        be.close()
    return rc


def main(argv=None):
    ap = argparse.ArgumentParser(prog="ice_halo_sim_amd.cli")
    ap.add_argument("-f", "--config", required=True, help="Lumice JSON configuration file")
    ap.add_argument("--render", type=int, default=None, help="render id to trace (default: lowest id)")
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--max-rays", type=int, default=None, help="cap the total root rays (required for ray_num: infinite)")
    ap.add_argument("--benchmark", action="store_true", help="print the [BENCHMARK] JSON line")
    ap.add_argument("-o", "--output-dir", default=None, help="the reference CLI's output contract (main.cpp:196-315): write img_<id>.<fmt> for EVERY "
                    "render entry of the config (one run per entry: the seam carries one renderer) and, for raypath_color configs, img_<id>_components.<fmt>")
    ap.add_argument("--format", default="jpg", choices=("jpg", "png"), help="image format of -o (default jpg)")
    ap.add_argument("--quality", type=int, default=95, help="JPEG quality of -o (default 95, 4:4:4 like stb_image_write above 90)")
    ap.add_argument("--backend", default="hip", help="accepted for the reference's command lines (auto | cpu | metal | cuda | hip); this engine has one backend")
    ap.add_argument("--out-rgb", default=None, help="write the sRGB image as binary PPM")
    ap.add_argument("--out-xyz", default=None, help="write the raw XYZ snapshot as .npy")
    ap.add_argument("--out-view", default=None, metavar="FILE.ppm",
                    help="write the traced image seen through another lens as binary PPM: per pixel of the view the traced image is read where that "
                    "pixel's direction lands (a gather on the device, nearest neighbour; no ray is traced).  Trace into a full-sky equal-area render "
                    "(dual_fisheye_equal_area) and every view shows radiance.  The --view-* options say what to look through; --auto-ev / "
                    "--target-white expose it as they expose --out-rgb (the EV is the traced image's)")
    ap.add_argument("--view-lens", default=None, choices=sorted(config.LENS_NAMES), help="lens of --out-view (default: the traced render's)")
    ap.add_argument("--view-fov", type=float, default=None, help="field of view of --out-view in degrees (default: the traced render's for the same lens, "
                    "else 90 linear, 60 globe, 180 fisheye)")
    ap.add_argument("--view-az", type=float, default=None, help="view azimuth of --out-view in degrees (default: the traced render's)")
    ap.add_argument("--view-el", type=float, default=None, help="view elevation of --out-view")
    ap.add_argument("--view-roll", type=float, default=None, help="view roll of --out-view")
    ap.add_argument("--view-size", default=None, metavar="WxH", help="size of --out-view (default: the traced render's)")
    ap.add_argument("--view-visible", default=None, choices=sorted(config.VISIBLE_NAMES), help="visible range of --out-view (default: the traced render's)")
    ap.add_argument("--view-overlap", type=float, default=None, help="dual-fisheye overlap of --out-view (default: the traced render's)")
    ap.add_argument("--view-filter", default="nearest", choices=("nearest", "bilinear"),
                    help="how --out-view reads the traced image: nearest copies the source pixel under each view pixel (default); bilinear weighs the four "
                    "around the exact spot, as the reference's preview does — for views that magnify the traced image")
    ap.add_argument("--view-blend", action="store_true",
                    help="--out-view of a dual-fisheye render traced with an overlap: cross-fade the two hemispheres across the overlap band, as the "
                    "reference's preview does, so that no seam shows at the horizon (changes nothing without an overlap)")
    ap.add_argument("--out-lanes", default=None, help="raypath_color configs: write the per-class Y lanes (classes, H, W) as .npy")
    ap.add_argument("--out-composite", default=None, help="raypath_color configs: write the class composite (the config's mode: dominant | additive | "
                    "painter; component_compositor.cpp) as binary PPM, composited on the device")
    ap.add_argument("--view-overlay", default=None, metavar="LAYERS",
                    help="draw auxiliary lines over --out-view and --out-view-composite, on the device: a comma-separated list of horizon, grid (altitude / "
                    "azimuth), circles (of constant angular distance from the sun), zenith (zenith and nadir rings) and sun (a marker); the sun is the "
                    "configuration's")
    ap.add_argument("--view-circles", default=None, metavar="DEG,DEG", help="angular distances of --view-overlay circles from the sun (default 22,46; at most 16)")
    ap.add_argument("--view-grid-step", default="auto", metavar="auto|DEG", help="spacing of the --view-overlay grid in degrees (auto: by the view's field of view)")
    ap.add_argument("--out-view-composite", default=None, metavar="FILE.ppm",
                    help="raypath_color configs: write the class composite seen through another lens as binary PPM — --out-composite's image gathered "
                    "on the device the way --out-view gathers the traced one (the --view-* arguments, --view-filter and --view-blend apply; "
                    "--display-ev is the composite's)")
    ap.add_argument("--canonical-order", action="store_true",
                    help="multi-scattering configs: hand every layer's continuing rays to the next layer in canonical (root ray, interaction) "
                    "order, so a fixed --seed traces the same second- and third-layer rays on every run (option cont_order = 1; costs a sort of the "
                    "continuation pool per layer).  It does not make the image bit-identical: pixel sums are fp32 atomics in whatever order the GPU "
                    "adds them; a multi-GPU run is canonical per rank")
    ap.add_argument("--deterministic", action="store_true",
                    help="bit-reproducible image: pixel sums and the landed weight are 64-bit fixed-point integers from the first add to the fold "
                    "(option deterministic = 1; multi-scattering configs take cont_order = 1 with it), so a fixed --seed gives the same XYZ bytes on "
                    "every run, whose sha256 is printed.  A config that needs what the route does not cover (raypath_color, a filter outside the fast "
                    "form) is refused with the reason and a non-zero exit; a multi-GPU run is reproducible per rank")
    ap.add_argument("--ranks", type=int, default=1,
                    help="with --deterministic: trace the job as N ranks, one per GPU, that share every session's rays (each rank plans the whole "
                    "session and launches its slice) and exchange their integer pixel sums where one rank folds them — the XYZ bytes, and the sha256 "
                    "printed, are those of the run without --ranks.  Started plainly, the command launches its own N ranks (torch.distributed.run); "
                    "HALO_DIST_BACKEND=gloo lets the ranks share one device (a rehearsal; default nccl = RCCL, one device per rank).  Single-layer "
                    "configs; not with -o")
    ap.add_argument("--spectrum-session", action="store_true",
                    help="a spectrum that is a list of discrete wavelengths: trace it as spectrum sessions — every dispatch one session that holds rays of "
                    "ALL the wavelengths, dealt out in blocks of consecutive rays — instead of one session per wavelength (which cannot fill the GPU "
                    "when the rays per wavelength are few).  The same rays when the scene has one crystal entry; ignored for an illuminant")
    ap.add_argument("--auto-ev", action="store_true",
                    help="expose the mono images of -o and --out-rgb automatically: the config's intensity_factor times 2^ev_auto, the reference GUI's "
                    "Adaptive Brightness computed on the device (P99 of the 8 x 8 box sums of Y against the per-pixel landed intensity, mapped to "
                    "--target-white, clamped to +-6 EV).  The EV chosen is printed per render; the class composite keeps its own P99 anchor")
    ap.add_argument("--stats", default=None, metavar="FILE",
                    help="write the statistics of the rendered image as one JSON object with the keys of the reference's scripts/dump_xyz_stats.py "
                    "(scene, config, pixel_count, non_zero_count, percentiles p50 .. p99_99, mean, std, cv, max, saturation_rate of Y over the "
                    "per-pixel intensity), computed on the device; with --render or a single render entry, with or without --auto-ev")
    ap.add_argument("--target-white", type=float, default=135.0, help="sRGB level (0, 255] the P99 maps to with --auto-ev (default 135)")
    ap.add_argument("--display-ev", type=float, default=0.0, help="display-time EV of the composite (display_exposure_scale = 2^EV)")
    args = ap.parse_args(argv)
    if not 0.0 < args.target_white <= 255.0:
        print("Error: --target-white must lie in (0, 255], got %g" % args.target_white, file=sys.stderr)
        return 2
    if not 1 <= args.quality <= 100:
        print("Error: --quality must be between 1 and 100, got %d" % args.quality, file=sys.stderr)
        return 2
    if args.stats and args.output_dir is not None and not args.benchmark and args.render is None:
        print("Error: --stats describes one rendered image: pass --render, not -o alone", file=sys.stderr)
        return 2
    shard = None
    if args.ranks < 1 or (args.ranks > 1 and not args.deterministic):
        print("Error: --ranks needs --deterministic and N >= 1 (ranks are merged exactly only through the fixed-point sums)", file=sys.stderr)
        return 2
    if args.ranks > 1:
        if args.output_dir is not None and not args.benchmark and args.render is None:
            print("Error: --ranks traces one render entry: pass --render (or --benchmark), not -o alone", file=sys.stderr)
            return 2
        if "WORLD_SIZE" not in os.environ:
            return launch_ranks(args.ranks, sys.argv[1:] if argv is None else list(argv))
        shard = join_ranks(args)
        if shard is None:
            return 2
    rank0 = shard is None or shard[0] == 0
    try:
        job = config.load_config(args.config)
        for w in getattr(job, "warnings", []) if rank0 else []:
            print("[warning] " + w)
        if job.ray_num is None and args.max_rays is None:
            raise config.ConfigError('ray_num is "infinite": pass --max-rays')
        if args.output_dir is not None and not args.benchmark and args.render is None:
            return save_all_renders(job, args)
        if args.output_dir is not None:
            print("[warning] -o / --output-dir is ignored with --render / --benchmark (nothing is saved)", file=sys.stderr)
        wall0 = time.perf_counter()
        res = run_job(job, args.render, args.seed, args.device, args.max_rays, canonical_order=args.canonical_order, deterministic=args.deterministic,
                      spectrum_session=args.spectrum_session, shard=shard)
    except BackendUnavailableError as e:
        print("backend unavailable: %s" % e, file=sys.stderr)
        return 3
    except config.ConfigError as e:
        print("config error: %s" % e, file=sys.stderr)
        return 2
    except BackendError as e:
        if not args.deterministic:
            raise
        if rank0 or shard is not None:
            print("refused: %s%s" % (e, "" if shard is None else " [rank %d]" % shard[0]), file=sys.stderr)
        if shard is not None:
            leave_ranks(barrier=False)   # (no barrier: a refusal need not be every rank's — the launcher ends the ranks that are left)
        return 4
    be = res["backend"]
    if not rank0:   # the image is rank 0's
        be.close()
        leave_ranks()
        return 0
    meta = job.render_meta.get(res["render_id"], {})
    display = dict(intensity_factor=exposure_factor(be, res["render_id"], meta.get("intensity_factor", 1.0), args),
                   ray_color=meta.get("ray_color", (-1.0, -1.0, -1.0)), background=meta.get("background", (0.0, 0.0, 0.0)))
    rgb, xyz, total_intensity = be.Snapshot(**display)
    wall = time.perf_counter() - wall0
    if args.deterministic:
        print("xyz sha256: %s" % hashlib.sha256(xyz.tobytes()).hexdigest())
    if args.stats:
        with open(args.stats, "w") as f:
            json.dump(image_stats_record(be, args.config), f, indent=2)
            f.write("\n")
    if args.out_rgb:
        write_ppm(args.out_rgb, rgb)
    if args.out_xyz:
        np.save(args.out_xyz, xyz)
    if args.out_view:
        try:
            view = view_render(args, res["render"])
            overlay = view_overlay(args, job, view)
            if overlay is None:
                write_ppm(args.out_view, be.View(view, res["render"], filter=args.view_filter, blend=args.view_blend, **display)["rgb"])
            else:
                write_ppm(args.out_view, be.ViewOverlay(view, overlay, res["render"], filter=args.view_filter, blend=args.view_blend, **display)["rgb"])
        except config.ConfigError as e:
            print("config error: %s" % e, file=sys.stderr)
            be.close()
            return 2
    if args.out_composite and job.color_classes:   # before the lanes are drained: the composite reads them where they are
        ok, _, srgb, p99 = be.CompositeColorClasses(job.color_meta, job.color_mode, 2.0 ** args.display_ev, meta.get("intensity_factor", 1.0))
        if ok:
            write_ppm(args.out_composite, srgb)
        else:
            print("no composite: the participating classes hold no energy (P99 %.3g)" % p99, file=sys.stderr)
    if args.out_view_composite and job.color_classes:   # ... and so does its view
        try:
            view = view_render(args, res["render"])
            overlay = view_overlay(args, job, view)
            if overlay is None:
                out = be.ViewComposite(view, job.color_meta, job.color_mode, 2.0 ** args.display_ev, meta.get("intensity_factor", 1.0),
                                       source=res["render"], filter=args.view_filter, blend=args.view_blend)
            else:
                out = be.ViewCompositeOverlay(view, overlay, job.color_meta, job.color_mode, 2.0 ** args.display_ev, meta.get("intensity_factor", 1.0),
                                              source=res["render"], filter=args.view_filter, blend=args.view_blend)
        except config.ConfigError as e:
            print("config error: %s" % e, file=sys.stderr)
            be.close()
            return 2
        if out["produced"]:
            write_ppm(args.out_view_composite, out["srgb"])
        else:
            print("no composite: the participating classes hold no energy (P99 %.3g)" % out["p99"], file=sys.stderr)
    if args.out_lanes and job.color_classes:
        np.save(args.out_lanes, be.ReadbackClassLanes())
    if args.benchmark:
        active = res["active_sec"]
        basis = "steady" if active >= 0.05 else "active_short"
        out = {"mode": "multi", "workers": 1, "cores": os.cpu_count(), "rays": res["rays"], "wall_sec": round(wall, 3),
               "setup_sec": round(res["setup_sec"], 3), "active_sec": round(active, 3),
               "rays_per_sec": round(res["rays"] / max(active, 1e-9), 1), "rate_basis": basis, "backend": "hip",
               "resolution": [res["render"].width, res["render"].height]}
        print("[BENCHMARK] " + json.dumps(out))
    else:
        print("traced %d root rays in %.3f s (setup %.3f s); landed intensity %.6g" % (res["rays"], res["active_sec"], res["setup_sec"], total_intensity))
    be.close()
    if shard is not None:
        leave_ranks()
    return 0


def launch_ranks(n, argv):
    """`--ranks N` started plainly: re-run this command line as N ranks under torch.distributed.run (as bench.py --gpus N does) and return its
    exit code.  Under RCCL every rank needs a device of its own; HALO_DIST_BACKEND=gloo lets them share."""
    import socket
    import subprocess
    import torch
    nccl = os.environ.get("HALO_DIST_BACKEND", "nccl") == "nccl"   # (the launcher itself opens no device when the ranks share them)
    have = torch.cuda.device_count() if nccl and torch.cuda.is_available() else 0
    if nccl and have < n:
        print("Error: --ranks %d: only %d HIP device(s) visible (one rank per GPU under RCCL; HALO_DIST_BACKEND=gloo shares devices)" % (n, have), file=sys.stderr)
        return 2
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), "-m", "ice_halo_sim_amd.cli"] + list(argv)
    env = dict(os.environ, OMP_NUM_THREADS=os.environ.get("OMP_NUM_THREADS", "1"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    return subprocess.call(cmd, env=env)


def join_ranks(args):
    """This process is one of the launcher's ranks: take its device, join the process group.  Returns (rank, world)."""
    import torch
    import torch.distributed as dist
    world, rank, local = int(os.environ["WORLD_SIZE"]), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.ranks:
        print("Error: --ranks %d but the launcher started WORLD_SIZE=%d ranks" % (args.ranks, world), file=sys.stderr)
        return None
    backend = os.environ.get("HALO_DIST_BACKEND", "nccl")
    args.device = local % max(1, torch.cuda.device_count()) if backend != "nccl" else local
    torch.cuda.set_device(args.device)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if backend == "nccl":
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", args.device))
    else:
        dist.init_process_group(backend=backend)
    return rank, world


def leave_ranks(barrier=True):
    """Leave the process group: after the job with a barrier; after a refusal without one — this rank may be the only one that was refused, and
    the others may already wait in a collective: torch.distributed.run ends the remaining ranks when one exits with an error."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        if barrier:
            dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main())
