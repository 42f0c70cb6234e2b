/*
 * halo_trace.h — C ABI of the MI355X-native ice-halo trace backend (libhalo_hip.so).
 *
 * This is the drop-in boundary for ONE path of Lumice (LoveDaisy/ice_halo_sim): the per-ray trace
 * hot path behind `lumice::TraceBackend` (reference: src/core/backend/trace_backend.hpp:367-641).
 * The reference has no C-ABI plugin loader (backends are C++ classes compiled in and picked by
 * `CreateBackend`, src/core/simulator.cpp:854-919); this header is the stable C boundary we put
 * UNDER a thin C++ adapter (`ice_halo_sim_amd/csrc/hip_trace_backend.hpp`).
 *
 * Each entry point names the reference virtual it replaces.  Plain pointers and sizes only.
 * All functions return HALO_OK (0), HALO_UNAVAILABLE (1 → adapter throws BackendUnavailableError,
 * trace_backend.hpp:140-158) or HALO_FATAL (2).  One handle = one backend instance; a handle is
 * single-threaded (trace_backend.hpp:114-116, simulator.cpp:970-979).
 *
 * Everything crossing this boundary is WORLD-space (trace_backend.hpp:71-89) except injected golden
 * rays, which follow the reference's host-ingest convention: crystal-local, identity rotation
 * (src/core/backend/cpu_trace_backend.cpp:121-144).
 */
#ifndef HALO_TRACE_H_
#define HALO_TRACE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALO_ABI_VERSION 6   /* 2: HaloFilter holds up to 64 OR-clauses / 64 terms (was 8 / 16); 3: halo_last_route, piecewise
                                halo_drain_exits, option "shuffle_chunk", exit records carry full 64-face paths; 4: HaloRouteInfo
                                names the kernel mode (5 modes) and its specialisation, option "filter_fast"; 5: halo_consumer_composite /
                                halo_consumer_load_lanes (additive: nothing that existed changed); 6: HaloHostRays::crystal (the
                                seam's HostRayBatch::crystal), halo_consumer_consume (ConsumeDeviceFused of a drained image the CALLER holds) */

enum { HALO_OK = 0, HALO_UNAVAILABLE = 1, HALO_FATAL = 2 };

/* Compile-time caps — reference src/core/def.hpp:23-31 (kMaxMsNum, kMaxHits, kMaxCrystalNum). */
#define HALO_MAX_LAYERS 4
#define HALO_MAX_ENTRIES 16
#define HALO_MAX_HITS 64
#define HALO_MAX_FACES 20        /* CrystalGeom face slots, src/core/crystal.hpp:78 */
#define HALO_MAX_FACE_VTX 12     /* kCrystalGeomMaxVtxPerFace */
#define HALO_MAX_TRIS 64         /* lm_pcg::kMaxTriPerKernel, src/core/shared/pcg_shared.h:71 */
#define HALO_LUT_NODES 257       /* LatLut::kNodes, src/core/lat_lut.hpp:31 */
#define HALO_WL_POOL_MAX 255     /* kWlPoolSizeMax, src/core/backend/wl_pool.hpp:41 */
#define HALO_PATH_CAP 64         /* face numbers kept per exit record = the reference's ExitFaceSeq::kCap (exit_seam.hpp:22) */

/* DistributionType — src/core/math.hpp:123-130 (values are wire values, pcg_shared.h:64-69). */
enum {
  HALO_DIST_NONE = 0,
  HALO_DIST_UNIFORM = 1,   /* spread = FULL range */
  HALO_DIST_GAUSS = 2,
  HALO_DIST_ZIGZAG = 3,
  HALO_DIST_LAPLACIAN = 4,
  HALO_DIST_GAUSS_LEGACY = 5
};

/* Distribution{type, center, spread} — src/core/math.hpp:165-190. */
typedef struct HaloDist {
  int32_t type;
  float center;
  float spread;
} HaloDist;

/* AxisDistribution — src/core/math.hpp:271-310.  Degrees.  `latitude` is the INTERNAL latitude
 * (JSON `zenith` = 90 - latitude, src/core/math.cpp:679-714). */
typedef struct HaloAxis {
  HaloDist azimuth;
  HaloDist latitude;
  HaloDist roll;
} HaloAxis;

enum { HALO_CRYSTAL_PRISM = 0, HALO_CRYSTAL_PYRAMID = 1 };

/* PrismCrystalParam / PyramidCrystalParam — src/config/crystal_config.hpp.
 * Shape-scalar slot order = RNG draw order (src/core/simulator.cpp:405-425):
 *   prism  : height[0]=h, face_dist[0..5]
 *   pyramid: height[0]=upper_h, height[1]=prism_h, height[2]=lower_h, face_dist[0..5]
 * sync_group[k] (0 = independent) indexes [h0,h1,h2,d0..d5]; members of one group share one draw
 * (src/core/simulator.cpp:344-393). */
typedef struct HaloCrystal {
  int32_t kind;
  HaloDist height[3];
  HaloDist face_dist[6];
  int32_t sync_group[9];
  float wedge_upper_deg; /* pyramid only */
  float wedge_lower_deg;
} HaloCrystal;

/* One scattering-layer entry: MsInfo::setting_[ci] — src/config/proj_config.hpp:27-38. */
typedef struct HaloEntry {
  HaloCrystal crystal;
  HaloAxis axis;
  float proportion;
  int32_t crystal_config_id;
  int32_t filter_id;  /* 0 = no filter (pass-all); k > 0 = filters[k-1] of the table given to halo_set_filters */
  int32_t color_id;   /* 0 = no raypath-colour predicates; k > 0 = colour set k-1 of the table given to halo_set_color */
} HaloEntry;

/* Emit-gate filters — FilterConfig (src/config/filter_config.hpp:20-86) as the device matcher consumes it
 * (DeviceFilterDesc, src/core/device_filter_desc.hpp:60-100).  Face ids are crystal face NUMBERS. */
/* The reference's physical complex filters keep their AND-term counts in a flat host-built buffer (any number of OR-clauses up
 * to a 4096 sanity cap, device_filter_desc.hpp:56-79; its fixed 8 is the colour path's).  Here a complex filter is one
 * fixed-size record staged in LDS: up to 64 OR-clauses and 64 simple terms in all — the reference's test configs use at
 * most 12 (test/e2e/configs/parity_big_or_with_color.json). */
#define HALO_FILTER_MAX_OR 64
#define HALO_FILTER_MAX_TERMS 64  /* total simple terms over all AND-clauses of one complex filter */
enum { HALO_FILTER_NONE = 0, HALO_FILTER_RAYPATH = 1, HALO_FILTER_ENTRY_EXIT = 2, HALO_FILTER_DIRECTION = 3,
       HALO_FILTER_CRYSTAL = 4 };
enum { HALO_SYM_P = 1, HALO_SYM_B = 2, HALO_SYM_D = 4 }; /* FilterConfig::kSymP/B/D */
typedef struct HaloFilterTerm { /* SimpleFilterParam */
  int32_t type;
  int32_t raypath_len;
  uint8_t raypath[HALO_MAX_HITS]; /* raypath: face-number sequence */
  int32_t has_entry, entry, has_exit, exit_face; /* entry_exit: wildcards when has_* == 0 */
  uint32_t min_len, max_len;      /* entry_exit: path length bounds; max_len 0 = unbounded */
  float az, el, radii;            /* direction: degrees */
  int32_t crystal_id;             /* crystal: CrystalConfig::id_ */
} HaloFilterTerm;
typedef struct HaloFilter {
  int32_t action;    /* 0 = filter_in (match passes), 1 = filter_out */
  int32_t symmetry;  /* HALO_SYM_* bitmask */
  int32_t is_complex;
  int32_t or_count;  /* complex: number of OR-clauses; terms[] holds their AND-terms back to back */
  int32_t and_counts[HALO_FILTER_MAX_OR];
  HaloFilterTerm terms[HALO_FILTER_MAX_TERMS]; /* simple filter: terms[0] */
} HaloFilter;

/* Raypath colour (reference "Design 2", src/config/color_gate_table.hpp:25-81, cuda_trace_backend.cu:498-556): every
 * emitted exit carries a 64-bit component mask; a crystal entry's colour set lists predicates (SimpleFilterParam + P/B/D
 * symmetry) and the mask bit each sets when it matches the exit's raypath / direction / crystal; masks accumulate across
 * scattering layers (they ride with the continuation).  A colour CLASS is a bit set with an any/all rule; each in-frame
 * pixel hit of an exit whose mask satisfies class c adds cmf_y*w to lane c (class_count x W x H floats). */
#define HALO_COLOR_MAX_TERMS 16    /* predicates per crystal entry (ColorGatePlacement) */
#define HALO_COLOR_MAX_CLASSES 16
typedef struct HaloColorTerm { /* ColorGateEntry: predicate_, symmetry_, bit_ */
  HaloFilterTerm predicate;
  int32_t symmetry; /* HALO_SYM_* bitmask */
  int32_t bit;      /* 0..63 */
} HaloColorTerm;
typedef struct HaloColorSet {
  int32_t term_count;
  int32_t reserved;
  HaloColorTerm terms[HALO_COLOR_MAX_TERMS];
} HaloColorSet;
typedef struct HaloColorClass { /* ColorGateParams::color_class_bits / color_class_combine */
  uint64_t bits;
  int32_t combine_all; /* 0 = any bit of `bits` set, 1 = all of them */
  int32_t reserved;
} HaloColorClass;

typedef struct HaloLayer {
  float prob; /* MsInfo::prob_ — continuation probability to the next layer */
  int32_t entry_count;
  HaloEntry entries[HALO_MAX_ENTRIES];
} HaloLayer;

/* SceneConfig fields read on the path (sun: src/config/light_config.hpp SunParam). Degrees. */
typedef struct HaloScene {
  float sun_altitude;
  float sun_azimuth;
  float sun_diameter;
  int32_t max_hits; /* counts surface interactions INCLUDING the entry face (simulator.cpp:1308) */
  int32_t layer_count;
  HaloLayer layers[HALO_MAX_LAYERS];
} HaloScene;

/* LensParam::LensType integer values — src/core/shared/projection_shared.h:136-146. */
enum {
  HALO_LENS_LINEAR = 0,
  HALO_LENS_FISHEYE_EQUAL_AREA = 1,
  HALO_LENS_FISHEYE_EQUIDISTANT = 2,
  HALO_LENS_FISHEYE_STEREOGRAPHIC = 3,
  HALO_LENS_DUAL_FISHEYE_EQUAL_AREA = 4,
  HALO_LENS_DUAL_FISHEYE_EQUIDISTANT = 5,
  HALO_LENS_DUAL_FISHEYE_STEREOGRAPHIC = 6,
  HALO_LENS_RECTANGULAR = 7,
  HALO_LENS_FISHEYE_ORTHOGRAPHIC = 8,
  HALO_LENS_DUAL_FISHEYE_ORTHOGRAPHIC = 9,
  HALO_LENS_GLOBE = 10
};
enum { HALO_VISIBLE_UPPER = 0, HALO_VISIBLE_LOWER = 1, HALO_VISIBLE_FULL = 2 };

/* RenderConfig fields read by BuildProjParams — src/core/lens_proj_build.hpp:79-137,
 * src/config/render_config.hpp:71-103.  Degrees. */
typedef struct HaloRender {
  int32_t lens_type;
  float fov;
  int32_t width;
  int32_t height;
  int32_t lens_shift[2];
  float view_az;
  float view_el;
  float view_ro;
  int32_t visible;
  float overlap; /* dual-fisheye overlap band (max |dz|), 0 = off */
} HaloRender;

/* Illuminants — src/util/illuminant_data.hpp:12-19. */
enum { HALO_ILLUM_D50 = 0, HALO_ILLUM_D55 = 1, HALO_ILLUM_D65 = 2, HALO_ILLUM_D75 = 3, HALO_ILLUM_A = 4, HALO_ILLUM_E = 5 };

/* WlParam (discrete: one session per wavelength) or illuminant pool
 * (src/core/backend/wl_pool.hpp:67-91: M mid-point wavelengths on [380,780], per-ray pick). */
typedef struct HaloWl {
  float wavelength; /* nm; used when illuminant < 0 */
  float weight;     /* spectral weight; used when illuminant < 0 */
  int32_t illuminant; /* -1 = discrete wavelength, else HALO_ILLUM_* */
  int32_t pool_size;  /* illuminant pool entries M (0 → 64 default, cap 255) */
} HaloWl;

/* HostRayBatch — src/core/backend/trace_backend.hpp:230-239.  Crystal-local golden-ray ingest. */
typedef struct HaloHostRays {
  const float* d;      /* 3*count */
  const float* p;      /* 3*count */
  const float* w;      /* count */
  const uint32_t* tf;  /* count — compact polygon-face id of the entry face */
  const struct HaloGeomTables* crystal;   /* HostRayBatch::crystal (trace_backend.hpp:230-239): the crystal the rays were sampled on, or NULL =
                                             the entry's own.  A supplied crystal is traced as it is — it consumes no MakeCrystal draw, so it is
                                             not a stochastic sample (test_cpu_trace_backend.cpp:737-777) — whatever the entry's shape distributions */
} HaloHostRays;

/* LayerStats — trace_backend.hpp:296-299 (+ continuation count from LayerHandle). */
typedef struct HaloLayerStats {
  uint64_t root_count;
  uint64_t exit_count;       /* exits emitted to the image (or captured) in this layer */
  uint64_t continuation_count;
  double exit_w_sum;
  double kernel_ms;          /* HIP-event time of this layer's kernels on the backend stream */
  uint64_t pixel_hits;       /* in-frame pixel writes (primary + overlap): 3 fp32 accumulator RMWs each */
  uint64_t launches;         /* kernel launches this layer took */
} HaloLayerStats;

/* ExitRayRecord — src/core/exit_seam.hpp:40-53, trimmed to what the parity tests read.
 * Only produced when option "capture_exits" is on (test path; production accumulates on device). */
typedef struct HaloExitRecord {
  float dir[3];     /* world-space exit direction */
  float weight;
  uint32_t root;    /* root-ray index within the layer (entries are laid out back to back) */
  uint16_t seq;     /* 2*interaction_index + child (0 = reflected, 1 = refracted); 0 = entry-face external reflection */
  uint8_t layer;
  uint8_t path_len;
  uint8_t path[HALO_PATH_CAP]; /* crystal face NUMBERS (1..8 prism; pyramid 1,2,3-8,13-18,23-28) */
  int32_t pixel;    /* flat pixel index of the primary hit, -1 = culled / out of frame */
  uint16_t crystal_id;
  uint16_t wl_idx;
  uint64_t color_mask; /* raypath-colour component mask of the exit (0 without halo_set_color) */
} HaloExitRecord;

typedef struct HaloBackend* halo_handle_t;

/* --- lifecycle ---------------------------------------------------------------------------- */
/* Number of visible HIP devices (CudaDeviceAvailable analogue, cuda_trace_backend.cu:147-193). */
int halo_device_count(void);
/* CreateBackend(BackendKind) — simulator.cpp:854-919.  seed must be non-zero (effective_seed_,
 * simulator.cpp:782-798); the backend seeds ONCE and keeps monotone ray counters across sessions
 * (cpu_trace_backend.hpp:131-140, cuda_trace_backend.cu:3724-3741). */
int halo_create(int device_ordinal, uint32_t seed, halo_handle_t* out);
int halo_destroy(halo_handle_t h);
const char* halo_last_error(halo_handle_t h);
/* Options: "capture_exits" (0/1), "geom_clock" (rays per sampled shape, default 32 — simulator.hpp:144),
 * "seed" (re-seed the engine between sessions: the reference's backends are seeded by the first non-zero SessionSpec::seed,
 * cpu_trace_backend.cpp:248-257), "rank"/"world" (shard id mixed into the ray counters so ranks draw disjoint streams), "ray_base" (the 64-bit index of the next
 * root ray — SplitPcgRayBase, trace_backend.hpp:184; counters run on from it, across 2^32 with the carry of pcg_advance_hi),
 * "chunk" (max rays per kernel launch, default 256 Mi), "aggregate" (0 plain atomics, 1 LDS pixel cache [default], 2 diagnostic no-accumulate),
 * "mono" (one-channel accumulation for discrete-wavelength sessions, default 1), "mono_copies" (privatised copies of that
 * plane, power of two, default 8), "async" (queue final-layer dispatches without a host sync, see halo_collect_stats),
 * "bin" (binned accumulation: hits staged in LDS and flushed to per-tile hit lists by the trace kernel — one level of lists up to
 * 512 tiles of 16 Ki accumulator slots, two levels (coarse lists, split pass) beyond; -1 [default] = only for the full-sky
 * launches >= 2 Mi rays of sessions with one plane per pool entry ("lambda_planes" = 1), where the hit log cannot go; 0 = never;
 * 1 = always when applicable), "bin_l1" (coarse lists of the two-level route, default 128), "stoch_chunk" (rays per launch with
 * device-generated crystal pools; default 64 Mi),
 * "lambda_planes" (illuminant sessions: -1 [default] = batches >= 2 Mi rays on images above 512 Ki pixels keep X/Y/Z planes and
 * their launches log {slot, pool entry, weight}, the log's per-tile pass makes X, Y, Z; other batches >= 8 Mi rays keep one
 * scalar plane per wavelength-pool entry, CMF applied by the closing fold; the rest X/Y/Z planes by direct atomics; 0 = never
 * per-entry planes nor the X/Y/Z log; 1 = always per-entry planes),
 * "host_shapes" (1 = build stochastic shape pools on the host and upload them; default 0 = device generator),
 * "blocks_per_cu" (cap on workgroups per CU of one launch, default 24; launches are sized for >= 32 ray-loop passes per
 * workgroup below that cap; small launches take one workgroup per CU up to 3 x 2^17 rays and two up to 2^22),
 * "lazy_fold" (1 [default]: halo_end of a session on the backend's OWN accumulator leaves its planes unfolded; every reader of the
 * image — readback, consumer fold, reduce, take_landed, bind — folds first, and so does halo_begin of a session with other planes
 * (wavelength, image size, plane or copy count): many small equal sessions cost one fold per readback; an accumulator bound with
 * halo_bind_accumulator is always folded at halo_end, its owner reads it without asking; 0: fold at every halo_end),
 * "gen_serial" (0 [default]: stochastic pyramids are built by teams of 32 lanes per crystal; 1: one thread per crystal — the
 * same builder the host runs; records are bit-identical either way, A/B knob),
 * "hit_log" (-1 [default]: production-mode launches >= 2 Mi rays on one scalar plane (>= 512 Ki rays when the render's visible range is
 * FULL: every exit of a full-sky render lands, and that many direct atomics cost more than the log's passes), or on the X/Y/Z planes of an illuminant
 * session (>= 2 Mi rays, image above 512 Ki pixels), append the hits that miss the pixel cache to a log region per workgroup — plain stores instead of
 * memory-side fp32 atomics — which a split pass and a per-tile LDS pass then add to the plane(s); 0 = never (direct atomics),
 * 1 = whenever applicable.  In a DETERMINISTIC session (option "deterministic" below) the log has integer twins: the trace kernel keeps its
 * integer pixel cache and flushes it onto the integer planes itself, a hit that loses the cache claim leaves as a raw {slot, fp32 weight} record,
 * and the split and per-tile passes quantise the records with the session's F and add integers — the planes end up holding, bit for bit, the
 * integers of the direct deterministic route.  There -1 takes the log from 2 Mi rays per launch on either plane layout (whatever the
 * visible range; any image the log's tiles fit: up to 4 Mi slots on a scalar plane, 2 Mi on X, Y, Z), 0 = every miss an integer atomic, 1 = whenever applicable —
 * and only there also with "aggregate" = 0, where every hit is a record), "hit_log_cap" (test knob: records per log region, 0 [default] = sized from the launch; what runs
 * over a region or a tile list is added directly),
 * "hex_fast" (1 [default]: one-shape dispatches of a REGULAR hexagonal prism run the instantiation whose next-face search has the
 * normals as literals; 0: the table-driven search — same candidates, order and comparisons, A/B knob),
 * "entry_fast" (1 [default]: one-shape dispatches of a full 8-face prism pick the entry face slab by slab, in registers;
 * 0: the generic walk over faces — same uniform, same cumulative order, A/B knob),
 * "spec_root" (1 [default]: a last-layer logged launch of a discrete-wavelength session over one regular hexagonal prism, whose lens, visible range
 * and closed gate are already compile-time constants, also takes its root generation as constants when the entry's axis is "latitude by the LUT,
 * azimuth and roll uniform" — over generated roots or over the continuation pool; same draws, same stream slots, same rays; 0: the run-time
 * form everywhere, A/B knob; halo_last_root_profile tells which ran),
 * "pool_entry_fast" (1 [default]: logged launches over sampled PRISMS pick the entry face of every full eight-face prism slab by slab, from tables
 * its half-wave rebuilds each pass; 0: the walk over the fan triangles — same uniform, same cumulative order; the same prisms, when their slab normals are the regular prism's, search their next face with literal normals — same candidates and comparisons as the table-driven search; A/B knob),
 * "rehit_strategy" (which of the reference's two next-face strategies the trace follows where they part, src/core/shared/traversal_shared.h:23-29:
 * 1 [default] = its CUDA backend's — the child that leaves through the face the ray stands on is an outgoing candidate where it is; 0 = its
 * legacy CPU path's, PropagateSlab optics.cpp:64-158 — that child is propagated over all faces, the source face included, with the relaxed
 * accept threshold, and one that "re-hits" goes on as a segment.  The two agree on a convex crystal whose entry points lie on their faces'
 * planes; they part on a fan the vertex merge moved off its plane.  0 runs every launch on the generic kernels (no exit queue, no hit log:
 * several times slower) — for a caller that needs SURVEY's stated ground truth ray for ray; not inside a session),
 * "shuffle_chunk" (Recombine's shuffle permutes chunks of this many consecutive continuation-pool entries; power of two in
 * [1, 64], default 32 = one 128-byte line per plane read; 1 = the reference's per-ray permutation, cu:1633-1657),
 * "cont_order" (additive in ABI 6, no struct changed: 0 [default] = the continuation pool in append order, which wave scheduling decides;
 * 1 = canonical order — after every layer but the last, halo_recombine sorts the pool by (layer-global root index, exit seq) — the index
 * HaloExitRecord::root reports, on the device and in stream order; shuffle, shuffle_chunk and the transit streams keep their meaning, so a
 * fixed seed traces the same rays on every layer of every run (the image is still a float sum in scheduling order — unless option "deterministic" is on).  Layers before the last
 * then accumulate with direct atomics, and every layer of a multi-layer session returns synchronously (option async does not defer the last
 * one: the layer ends with the check of the order's invariants — a broken one, like a pool overflow, is HALO_FATAL); needs rehit_strategy = 1;
 * not inside a session),
 * "deterministic" (additive in ABI 6, no struct changed: 0 [default] = the float routes above; 1 = every accumulating launch of every layer runs the
 * fixed-point route — a hit's value v (the weight on a scalar plane, the fp32 products cmf * weight on X, Y, Z) enters every sum as the 64-bit
 * integer floor(double(v) * 2^F + 0.5), in the workgroup's pixel cache, in the global planes and in the landed-weight tally alike, and integer
 * sums do not depend on the order of their adds.  A discrete session keeps one scalar plane, an illuminant session X, Y, Z planes; bin,
 * lambda_planes and mono_copies are ignored, hit_log chooses between the direct route and the hit log's integer twins (same integers either way).  REPRODUCIBLE: the integer plane sums and the landed integer of a session depend only on the set of
 * rays traced into them — not on chunk, blocks_per_cu, small_blocks_per_cu, overlap, async, aggregate, hit_log, hit_log_cap, mono_copies, table_cache, stream
 * assignment or wave scheduling; the XYZ image is a per-pixel function of those sums and of the order of the folds, which is the order of the
 * caller's sessions (a plane value is float32(double(S) * 2^-F)), so a fixed seed and ray_base give the same bytes on every run.  Over several
 * layers this holds together with cont_order = 1.  F is the largest scale <= 32 at which 2^30 rays of the session's largest weight cannot wrap a
 * slot (halo_host_fixed_frac_bits: 29 for weights up to 1); a plane set that has taken 2^30 rays is folded before the next launch, at a launch
 * boundary — beyond that budget the image, not the sums of each fold, depends on chunk.  ACROSS RANKS (halo_set_shard,
 * halo_export_fixed, halo_import_fixed): N shards that export at points P, whose words are summed as integers and imported into one handle that then
 * folds, leave the XYZ bytes and landed weight of one unsharded handle that folds (halo_flush) at the same points P, for sessions of at most 2^30
 * rays between two points; a float reduce of per-rank images (halo_reduce_accumulator, dist.ShardedTracer) stays reproducible per rank only.  REFUSED, by name, at halo_begin (nothing is ever run on
 * a float route in silence): a multi-layer session without cont_order = 1, raypath-colour tables, capture_exits = 1, rehit_strategy = 0, a
 * filter that needs the generic filter kernels.  On the direct route every hit outside the pixel cache is a memory-side 64-bit integer atomic
 * (configs[1]'s step +62 %, a full-sky X/Y/Z session 5 x); launches of 2 Mi rays and more take the hit log's integer twins instead (see "hit_log":
 * +33 % and 1.43 x); not inside a session),
 * scheduling (ABI 6; none of them changes a result): "overlap" (1 [default]: launches of <= 2 Mi rays alternate between two
 * trace streams, closing folds run on an auxiliary stream; 0 = everything on the one stream), "table_cache" (1 [default]: equal
 * sessions reuse their device tables), "small_blocks_per_cu" (default 5: workgroups per CU a small launch spreads over before a
 * workgroup takes a second pass), "defer_fold" (see halo_flush), "gen_ahead" (experiment knob, 0 [default]; 1: the crystal generator of a
 * launch that fills the chip is queued beside the previous launch's trace kernel — measured, gains nothing: both are VALU-bound),
 * "close_direct" (-1 [default]: a hit-log launch that is its whole session — last layer, one crystal entry, one chunk, nothing pending in the
 * planes — on the float route's contiguous-tile scalar path (one plane, one copy, twin present, not a full-sky render) and large enough to fill
 * the chip has its per-tile pass add CMF x sum to the XYZ image itself: bit-equal to plane-then-fold, no closing fold; 0: never; 1: wherever
 * eligible, whatever the launch size; halo_direct_closes counts them), "tile_append" (-1 [default]: a launch that closes directly, fills the chip and
 * runs a trace kernel with a per-tile twin — plain mode, one regular prism, scalar plane, closed gate, a lens that is a template constant — appends
 * its records to per-tile chunks of each workgroup, and the closing pass reads the chunks: no split pass; the same records reach the same integer
 * tile sums; 0: never; 1: wherever eligible, whatever the launch size; halo_tile_appends counts them), "tile_ticket" (-1: a launch
 * that takes the per-tile append by "tile_append"'s auto rule — it fills the chip and runs over generated roots — runs ONE resident round of
 * workgroups whose waves draw their passes of the ray loop, 64 rays each, from a counter: the same rays, ray by ray, traced by whichever wave is
 * free; -2 [default]: as -1, for launches whose static grid is more than one resident round — the others have no rounds to even out and keep the
 * static loop, and with it its landed tally to the last digit; 0: never, the static ray loop; 1: every launch that appends per tile, whatever its
 * size; halo_tile_tickets counts them.  Counts are
 * those of the static loop exactly; the image differs by the order of float adds; which rays a lane traces changes from run to run, so a ticketed
 * launch sums its landed and exit weight in fp64 from the lane on, and two runs of one seed agree in them to rel 1e-12, not to the last
 * bit), "ticket_min" / "ticket_max" / "ticket_div" (experiment knobs, UNSUPPORTED — they may go without notice: the bounds of a ticket in wave-passes and the divisor of the guided
 * rule, halo_host_ticket_size; defaults 4 / 64 / 2), "lean_events" (1 [default]: markers that
 * fall on one point of one stream share one recorded event, and a trace stream does not wait again for a main stream that has been given nothing
 * since it last did; 0: every marker its own record, every launch the wait — the A/B switch; same results either way). */
int halo_set_option(halo_handle_t h, const char* key, int64_t value);
/* Use an external HIP stream (e.g. torch's current stream) for all launches. NULL = own stream. */
int halo_set_stream(halo_handle_t h, void* hip_stream);
/* Bind an externally-owned device accumulator of width*height*3+4 floats (e.g. a torch tensor, so
 * torch.distributed can reduce it in place).  NULL = backend-owned.  Layout: the xyz image, then 4 reserved floats
 * (kept zero; the landed-weight tally is a separate fp64 scalar read with halo_take_landed / halo_readback_xyz64). */
int halo_bind_accumulator(halo_handle_t h, void* device_ptr, uint64_t n_floats);
/* The filter table HaloEntry::filter_id indexes (ConfigManager::filters_, config_manager.cpp:184-215). Copied; stays in
 * force until replaced.  A filter-failing exit is dropped: neither emitted nor continued (CollectData simulator.cpp:725). */
int halo_set_filters(halo_handle_t h, const HaloFilter* filters, int32_t count);

/* --- session ------------------------------------------------------------------------------ */
/* TraceBackend::BeginSession(SessionSpec) — trace_backend.hpp:374-378. scene/render are COPIED.  ray_num (SessionSpec::ray_num)
 * is the number of roots the session is going to trace; it only selects the accumulation layout of illuminant sessions
 * (see "lambda_planes"), results do not depend on it. */
int halo_begin(halo_handle_t h, const HaloScene* scene, const HaloRender* render, const HaloWl* wl, uint64_t ray_num);
/* A SPECTRUM session (additive in ABI 6, no struct changed): one session for a whole list of discrete wavelengths, where the reference — and
 * halo_begin — take one session per wavelength (simulator.cpp:1098-1109).  entries[0 .. count) are discrete HaloWl (illuminant == -1),
 * 1 <= count <= HALO_WL_POOL_MAX; anything else is HALO_FATAL with a message that names the argument, and the handle stays usable.  The session's
 * wavelength pool is what halo_host_wl_pool gives for each entry, one behind the other: {n(lambda_k), weight_k, CMF(round lambda_k)} — n = 1 outside
 * 350-900 nm and CMF 0 outside 360-830 nm, as a discrete session has them.  count == 1 IS the discrete session of entries[0]: same route, same bytes.
 * For count > 1 the session is an illuminant-like pool session wherever layouts are chosen (X/Y/Z or per-entry planes, "lambda_planes", "hit_log",
 * "bin", the deterministic X/Y/Z planes), with the largest |weight_k| as the bound of the fixed-point sums; halo_trace_layer, halo_recombine,
 * halo_end, the readbacks and the consumer are what they are for any session.
 * WHICH RAY TAKES WHICH ENTRY — by index, not by a draw: in layer 0 crystal entry ci gets m_ci roots from the partition, back to back as always; its
 * root r (0-based within ci's range, counted across the launches "chunk" cuts, not within one) takes spectrum entry min(r / per_ci, count - 1) with
 * per_ci = ceil(m_ci / count): blocks of consecutive roots INSIDE each crystal entry's range, so that no crystal is lit by a part of the spectrum
 * only; when count > m_ci the blocks are single roots and entries >= m_ci get none.  Host-injected rays follow the same rule over the injected
 * batch and keep their injected weight.  Layers >= 1 read the entry from the continuation pool, as every pool session does.  No RNG draw is
 * consumed for the pick and the wavelength stream is not touched; every other stream keeps its slots, so root r is the ray a discrete session
 * generates at that counter (with "ray_base" = B, block k of a one-entry scene is entry k's discrete session at ray_base B + k * per).
 * ray_num: as for halo_begin — the roots the session is going to trace; it selects the accumulation layout only. */
int halo_begin_spectrum(halo_handle_t h, const HaloScene* scene, const HaloRender* render, const HaloWl* entries, int32_t count, uint64_t ray_num);
/* TraceBackend::TraceLayer(RootRaySource) — trace_backend.hpp:380-389.  First call of a session:
 * host mode, `count` roots self-generated on device (rays == NULL) or injected (rays != NULL).
 * Later calls: device mode, consumes the continuation produced by halo_recombine (count ignored). */
int halo_trace_layer(halo_handle_t h, uint64_t count, const HaloHostRays* rays, HaloLayerStats* stats);
/* TraceBackend::Recombine(handle, RecombineSpec{shuffle}) — trace_backend.hpp:391-395.  No data moves: the pools swap
 * roles and the next layer reads its roots through a Feistel bijection of the pool positions.  The bijection permutes
 * chunks of 32 consecutive pool entries (32 different parent rays), not single entries like the reference's CUDA
 * shuffle_cont_kernel (cu:1633-1657): same decorrelation of position ranges, coalesced reads. */
int halo_recombine(halo_handle_t h, int shuffle, uint64_t* continuation_count);
/* TraceBackend::DrainExits — trace_backend.hpp:430-448 (only with "capture_exits").  Copies at most `cap` pending records
 * (oldest first) into `out`, *count = records copied; the rest stays pending, so a caller may drain in pieces.
 * out == NULL: *count = number of pending records, nothing is consumed. */
int halo_drain_exits(halo_handle_t h, HaloExitRecord* out, uint64_t cap, uint64_t* count);
/* TraceBackend::EndSession. The accumulator persists (SupportsThirdClockDrain, cu:4801-4808). */
int halo_end(halo_handle_t h);
/* TraceBackend::ReadbackXyzAccum — trace_backend.hpp:461-469, cuda_trace_backend.cu:4800-4846:
 * sync, ADD landed weight into *landed_weight, copy W*H*3 floats, zero the device accumulator. */
int halo_readback_xyz(halo_handle_t h, float* xyz, int width, int height, float* landed_weight);
/* Same, but returns landed weight in double and does not add. */
int halo_readback_xyz64(halo_handle_t h, float* xyz, int width, int height, double* landed_weight);
/* Raypath colour tables: `sets` is referenced by HaloEntry.color_id (1-based), `classes` defines the Y lanes.
 * n_sets = n_classes = 0 switches colour off (the default; the production kernels then carry no mask at all). */
int halo_set_color(halo_handle_t h, const HaloColorSet* sets, int n_sets, const HaloColorClass* classes, int n_classes);
/* TraceBackend::ReadbackClassLanes — trace_backend.hpp:471-493: copies class_count*W*H floats (lane c at
 * lanes[c*W*H + py*W + px]) and zeroes the device lanes.  Call after halo_readback_xyz's sync point or halo_sync. */
int halo_readback_class_lanes(halo_handle_t h, float* lanes, int width, int height, int class_count);
/* TraceBackend::GetLastBatchStochasticCrystalSampleCount / ...OrientationSampleCount (trace_backend.hpp:587,625), for the
 * session traced last (counters reset at halo_begin): crystal instances actually sampled (one per geom_clock rays of every
 * crystal entry that is not IsDeterministic; 0 for fixed shapes) and rays whose orientation was drawn (every ray of an entry
 * whose axis has a non-fixed distribution).  Real counts of what the kernels did, not estimates. */
int halo_last_sample_counts(halo_handle_t h, uint64_t* crystal_samples, uint64_t* orientation_samples);
/* Which kernels served the session traced last (masks reset at halo_begin).  Diagnostics for the parity tests and the bench:
 * a test that means to check the production binned shape-pool kernel asserts that it really ran. */
typedef struct HaloRouteInfo {
  uint32_t launches;     /* trace-kernel launches since halo_begin */
  uint32_t mode_mask;    /* bit m: a launch ran the MODE m instantiation: 0 production; 1 production + emit-gate filter, 4 production + filter and
                            raypath colour (both for max_hits <= 16: path in a register, predicates as host-built member tables); 2 + exit capture
                            (tests); 3 the generic filter / colour kernels (paths to 64 faces, or tables that do not fit the fast form) */
  uint32_t geom_mask;    /* bit g: GEOM g (0 one shape per dispatch, 1 pool of 4.1 KB records, 2 pool of prism records, 3 one shape = regular hexagonal prism) */
  uint32_t accum_mask;   /* bit 0 direct X/Y/Z planes, 1 direct scalar plane(s), 2 binned one level, 3 binned two levels, 4 hit log, 5 hit log of an illuminant session (X, Y, Z made in the per-tile pass), 6 none (a layer whose every exit continues), 7 fixed-point planes (option "deterministic": beside it only bit 4 or 5 — launches that went through the hit log's integer twins, scalar plane or X, Y, Z — and bit 6) */
  uint32_t source_mask;  /* bit 0 generated roots, 1 continuation pool (layer >= 1), 2 host-injected rays */
  uint32_t plane_cnt;    /* accumulation planes of the session (1 discrete, 3 X/Y/Z, M per-entry) */
  uint32_t plane_copies; /* privatised copies of each plane */
  uint32_t shuffle_chunk;/* pool entries that move together through Recombine's shuffle */
  uint32_t spec_mask;    /* specialised instantiations that ran — bit 0: last-layer kernel (no continuation-append code), 1: lens as a compile-time
                            constant, 2: visible range as a constant, 3: closed gate (prob <= 0) as a constant */
  uint32_t generic_launches; /* launches that ran an instantiation with none of those specialisations */
} HaloRouteInfo;
int halo_last_route(halo_handle_t h, HaloRouteInfo* out);
/* Root-generation profiles among the kernels that served the session traced last (reset at halo_begin; additive in ABI 6, no struct changed —
 * HaloRouteInfo keeps its size and its masks their meaning).  Bit 0: a launch ran the last-layer instantiation that has "generated roots, latitude
 * by the LUT, azimuth and roll uniform" as compile-time constants; bit 1: the same orientation over the continuation pool (a last layer >= 1).
 * 0: every launch generated its roots with run-time tests on source, latitude path and distribution kinds (see option "spec_root"). */
int halo_last_root_profile(halo_handle_t h, uint32_t* profile_mask);
/* Launches, since halo_create, that closed their session in their own per-tile pass (option "close_direct"; additive in ABI 6, no struct changed —
 * such a launch still reports accum_mask bit 4).  A cumulative count: take the difference around the sessions of interest. */
int halo_direct_closes(halo_handle_t h, uint64_t* count);
/* Launches, since halo_create, whose trace kernel appended its records per tile (option "tile_append"; additive in ABI 6, no struct changed — such a
 * launch is also counted by halo_direct_closes and still reports accum_mask bit 4).  A cumulative count. */
int halo_tile_appends(halo_handle_t h, uint64_t* count);
/* Launches, since halo_create, whose trace kernel drew its rays by wave tickets (option "tile_ticket"; additive, no struct changed — such a launch is
 * also counted by halo_tile_appends and halo_direct_closes).  A cumulative count. */
int halo_tile_tickets(halo_handle_t h, uint64_t* count);
/* Bring the accumulator up to date WITHOUT a host wait: the closing folds of the ended sessions are queued and the backend's stream is made
 * to wait for them, so that work queued on that stream afterwards (a collective on a bound accumulator, a copy) sees the finished image.
 * Needed with option "defer_fold" = 1 (halo_end then leaves the fold of a caller-bound accumulator pending so that the next session's trace
 * kernels run under it); harmless otherwise.  Not inside a session. */
int halo_flush(halo_handle_t h);
/* Kernel time of the sessions' LAST layers since the previous call (HIP events on the launch's stream, read after a host wait): trace_ms = the
 * trace kernels' own spans, post_ms = the spans of their accumulation passes (split + per-tile sums), launches = dispatches timed.  For
 * bench.py's roofline object, which prices the last layer's trace kernel; HaloLayerStats::kernel_ms is trace + passes of every layer. */
int halo_collect_timing(halo_handle_t h, double* trace_ms, double* post_ms, uint64_t* launches);
int halo_sync(halo_handle_t h);
/* Tallies of every layer traced since the previous call (summed), after waiting for the stream. With option
 * "async" = 1 a final-layer halo_trace_layer only queues its dispatches (its `stats` carry root_count alone) and the
 * exit / pixel-hit / kernel-time tallies are delivered here — the reference's LayerStats are diagnostics
 * (trace_backend.hpp:296-299), nothing on the path waits for them. */
int halo_collect_stats(halo_handle_t h, HaloLayerStats* out);
/* Read AND zero the device landed-weight tally (fp64) without touching the image: used when the image lives in a
 * bound external accumulator that is reduced across ranks in place. */
int halo_take_landed(halo_handle_t h, double* landed_weight);
/* The pending fixed-point planes of deterministic sessions, as the integers they are (additive in ABI 6).  Valid after halo_end, with option
 * "lazy_fold" = 1 and the backend's OWN accumulator, until a reader of the image or a session with other planes folds them: waits for the device and
 * copies plane `plane` (0 for a discrete session; 0, 1, 2 = X, Y, Z for an illuminant one) in PIXEL order — sums[py * width + px], the planes' slot
 * hash undone — n_pix = width * height; *frac_bits = F of those sums (a plane value is sums[p] * 2^-F); *landed = the landed weight of the ended
 * deterministic sessions nobody has taken yet, in units of 2^-*landed_frac_bits.  Every out pointer may be NULL.  Folds, zeroes and takes
 * nothing.  HALO_FATAL when no fixed-point planes are pending. */
int halo_peek_fixed(halo_handle_t h, int32_t plane, uint64_t* sums, uint64_t n_pix, uint32_t* frac_bits, uint64_t* landed, uint32_t* landed_frac_bits);

/* --- shards: N handles (ranks, boxes, or handles on one GPU) trace ONE session's rays between them (additive in ABI 6, no struct changed) --- */
/* Shard `index` of `count`; (0, 1) is the default and the whole of everything.  From then on halo_begin / halo_begin_spectrum / halo_trace_layer take
 * the WHOLE session's ray_num / count: every shard runs the same partition with the same carry, walks the same plan of launches and moves its root,
 * gate and shape counters on by the whole layer, exactly as one rank does — and launches only the part of each planned launch that lies in its
 * slice of the launch's crystal entry (halo_host_shard_slice), with the counter bases, spectrum blocks and HaloExitRecord::root it has in the whole
 * run.  The shards of a session trace exactly the one-rank session's rays, each once.  HaloLayerStats::root_count and halo_last_sample_counts
 * report what the shard traced; a shard whose slices are empty launches nothing and still moves the counters.  With deterministic = 1 the shard's
 * integer planes are a PART of the image: they leave through halo_export_fixed, and whatever would fold them — a readback, halo_flush,
 * halo_take_landed, a halo_begin with other planes — is HALO_FATAL with a message that names halo_export_fixed (the handle stays usable).  With
 * deterministic = 0 (capture_exits included) the shards trace the same rays and each folds its own float image: their sum differs from one rank's by
 * summation order only.  REFUSED, by name, handle usable: inside a session; count == 0 or index >= count; and with count > 1 a multi-layer scene (at
 * halo_begin: the next layer's pool order and shuffle are global over all roots), host-injected rays (at halo_trace_layer), option "rank" != 0,
 * a sampled crystal entry whose launches ("chunk", "stoch_chunk") are not multiples of geom_clock (at halo_trace_layer, before anything is queued),
 * and a launch whose session's weights change F_landed while the shard still holds landed weight of its own (export first: the integer leaves
 * as an integer).  WHERE TO EXCHANGE so that the merged image is one handle's: wherever one handle folds — before a session with other planes
 * (wavelength, spectrum, image size) or other weights, at every reader of the image, and before the LAUNCH with which the pending planes would pass
 * 2^30 rays; a caller that exchanges between sessions must therefore not let a session of several launches straddle that budget. */
int halo_set_shard(halo_handle_t h, uint32_t index, uint32_t count);
/* The slice rule, no device needed: shard `index` of `count` takes rays [*first, *first + *n) of a crystal entry's share of `share` rays, cut in
 * units of `clock` rays (geom_clock for an entry with sampled shapes, 1 for a fixed one): with u = ceil(share / clock),
 * [clock * floor(index * u / count), min(clock * floor((index + 1) * u / count), share)).  Disjoint, in index order, covering the share, starting at
 * clock multiples, sizes within one clock of each other.  HALO_FATAL for clock == 0, count == 0, index >= count or a NULL pointer. */
int halo_host_shard_slice(uint64_t share, uint32_t clock, uint32_t index, uint32_t count, uint64_t* first, uint64_t* n);
/* MOVE the pending fixed-point planes out, to device memory (preconditions of halo_peek_fixed: pending fixed-point planes, the backend's own
 * accumulator, not inside a session): dev_words receives plane_cnt * W * H 64-bit words in pixel order — plane p at [p * W * H, (p + 1) * W * H),
 * the slot hash undone by the kernel — and then ONE word, the landed integer nobody has taken yet; n_words must be plane_cnt * W * H + 1.  The planes
 * are left all zero and no longer pending and the landed integer is taken: nothing is counted twice.  *plane_cnt, *frac_bits (F) and
 * *landed_frac_bits (F_landed) describe the words (each may be NULL).  Waits for the device; the words are complete when it returns.  A shard that
 * ended a session without tracing a ray exports zeros.  Landed weight that was converted to a double when F_landed changed between sessions
 * stays with the handle for its next taker (halo_take_landed, a readback): on a shard that is imported weight only — weight of the whole image, on
 * the handle that folds it — exactly as one handle carries it. */
int halo_export_fixed(halo_handle_t h, void* dev_words, uint64_t n_words, uint32_t* plane_cnt, uint32_t* frac_bits, uint32_t* landed_frac_bits);
/* ADD such words (device memory; e.g. the integer sum of every shard's export) into the planes of the handle's last ended deterministic session,
 * modulo 2^64, in stream order on the backend's stream; the planes become pending at that F, the landed word joins the handle's untaken landed
 * integer, and `rays` — the rays the words stand for — count against the 2^30-ray budget of one unfolded plane set.  halo_flush and the readbacks
 * then fold exactly as after the handle's own session.  REFUSED, by name: a layout that is not the handle's (plane count, image size via n_words,
 * F, F_landed), a budget that would be passed, float planes pending, no deterministic session on the backend's own accumulator before it. */
int halo_import_fixed(halo_handle_t h, const void* dev_words, uint64_t n_words, uint32_t plane_cnt, uint32_t frac_bits, uint32_t landed_frac_bits, uint64_t rays);

/* Multi-GPU drain for a C/C++ host (one process — or one thread — per GPU, one backend per GPU): sum-reduce this rank's XYZ
 * accumulator (width*height*3+4 floats, owned or bound) onto rank `root` with ONE ncclReduce over RCCL/xGMI, queued on the
 * backend's stream behind its trace kernels; every other rank's accumulator is then zeroed (drained) in stream order.
 * `nccl_comm` is the caller's ncclComm_t (rccl.h); `root` its root rank.  The landed-weight scalars stay on their devices: read
 * them with halo_take_landed and add on the host.  RCCL is loaded lazily (dlopen "librccl.so"): the library has no link-time
 * dependency on it, and a host that never calls this never loads it.  HALO_UNAVAILABLE when RCCL cannot be loaded.
 * Reference: the drain point is Simulator::DrainDeviceXyz (simulator.cpp:1409-1477); Lumice itself has no multi-GPU code. */
int halo_reduce_accumulator(halo_handle_t h, void* nccl_comm, int root, int this_rank);

/* --- consumer on device (RenderConsumer::ConsumeDeviceFused / PrepareSnapshot / PostSnapshot, server/render.cpp) -- */
/* HaloDisplay: the RenderConfig fields PostSnapshot reads (render_config.hpp:84-92). ray_color[0] < 0 = real colour. */
typedef struct HaloDisplay {
  float intensity_factor;
  float ray_color[3];
  float background[3];
} HaloDisplay;
/* ConsumeDeviceFused (render.cpp:138-201): fold the device accumulator into the running image with Neumaier-compensated
 * adds (accum_shared.h:70-74), add its landed weight to total_intensity, zero the accumulator.  All on device. */
int halo_consumer_fold(halo_handle_t h);
/* The same fold for a drained image the CALLER holds — RenderConsumer::ConsumeDeviceFused(const SimData&), render.cpp:138-201, as it is
 * written: xyz = SimData::xyz_pixel_data_ (W*H*3 floats, Neumaier-folded into the running image), landed = xyz_landed_weight_ (added to
 * total_intensity), lanes = lane_pixel_data_ (class_count x W x H floats added to the class lanes; NULL / 0 = none).  What another rank,
 * another backend or the legacy path drained becomes part of this consumer; the first call sizes the consumer to width x height. */
int halo_consumer_consume(halo_handle_t h, const float* xyz, int width, int height, float landed, const float* lanes, int class_count);
/* PrepareSnapshot + PostSnapshot (render.cpp:465-578): snapshot = sum + compensation; scale = intensity_factor * 0.08 *
 * N_pix / total_intensity (ExposureScale :96-102); XYZ → gamut clip → linear RGB → sRGB u8 (util/color_space.cpp).
 * rgb_out: W*H*3 bytes (nullable); xyz_out: W*H*3 floats raw snapshot (nullable); total_intensity out (nullable). */
int halo_consumer_snapshot(halo_handle_t h, const HaloDisplay* display, uint8_t* rgb_out, float* xyz_out, double* total_intensity);
int halo_consumer_reset(halo_handle_t h);

/* --- auto exposure: the reference GUI's Adaptive Brightness anchor on the device (gui/gui_ev_auto.hpp, doc/adaptive-brightness.md) --- */
typedef struct HaloAutoEv {
  float p99_y;               /* fine-equivalent P99 (coarse P99 / f^2 on the coarse path) */
  float per_pixel_intensity; /* total_intensity / (0.08 * n_pix) */
  float ev_auto;             /* stops, clamped to [-6, 6]; 0 when there is no data */
  int32_t produced;          /* 0: no positive value or no landed intensity ("auto: no data") */
  uint32_t value_count;      /* positive values the percentile was taken over */
  int32_t coarse_w, coarse_h;/* 0, 0 = fine path */
} HaloAutoEv;
/* ComputeP99Y (gui_ev_auto.hpp:92-138) of the consumer's snapshot Y = sum + compensation (exactly halo_consumer_snapshot's xyz_out), the
 * per-pixel landed intensity of RenderConsumer::GetRawXyzResult (render.cpp:584-593) and ComputeEvAuto of the two, all in fp32 like the
 * reference.  downsample_factor > 1 with W / f > 0 and H / f > 0: Y is box-summed onto the f-times coarser grid (each bin's f x f pixels added
 * one after another, rows outside, columns inside; trailing rows / columns that fill no bin are dropped), the percentile is taken over the bins
 * > 0 and divided by f * f — a coarse grid with no positive bin gives 0, never the fine path.  Otherwise (f <= 1, or the grid collapses) it is
 * taken over the pixels with Y > 0.  The percentile is the exact order statistic at index (size_t)((float)count * 0.99f), clamped to count - 1:
 * a radix select on the device, one 32-byte record read back.  The reference's GUI passes downsample_factor 8 and target_white 135.
 * Applying the result is the caller's multiplication: snapshot with intensity_factor * 2^ev_auto.  Reads the consumer only: image, lanes and
 * total intensity stay as they are.  HALO_FATAL (handle still usable) before any fold / consume, with out == NULL, or with target_white outside (0, 255]. */
int halo_consumer_auto_ev(halo_handle_t h, int32_t downsample_factor, float target_white, HaloAutoEv* out);
/* ComputeEvAuto (gui_ev_auto.hpp:143-155): 0 if either input is <= 0, else clamp(log2f(target_linear / (p99_y / per_pixel_intensity)), -6, 6)
 * with target_linear the sRGB decoding of target_white / 255.  No GPU needed. */
float halo_host_ev_auto(float p99_y, float per_pixel_intensity, float target_white);

/* --- image statistics: exact percentiles and moments of the consumer's image, on the device (the numbers of the reference's
 *     doc/xyz-stats-tool.md / scripts/dump_xyz_stats.py; the stage has no counterpart in the reference's backend seam) --- */
#define HALO_STATS_MAX_PERCENTILES 16
enum { HALO_STATS_PLANE_Y = -1 }; /* >= 0: class lane c of halo_set_color */
typedef struct HaloStatsSpec {
  int32_t plane;            /* HALO_STATS_PLANE_Y or a lane index */
  int32_t percentile_count; /* 0 .. 16 */
  double percentiles[HALO_STATS_MAX_PERCENTILES]; /* each in [0, 100], any order, repeats allowed */
  float norm;               /* > 0: the divisor of the saturation test; <= 0: the per-pixel intensity (HaloAutoEv::per_pixel_intensity) */
  int32_t reserved;
} HaloStatsSpec;
typedef struct HaloImageStats {
  uint64_t pixel_count, positive_count, saturated_count;
  double sum, sum_sq;       /* of the positive values: the exact sums of the floats and of their exact squares, each rounded once */
  float max, norm;          /* norm: the divisor actually used */
  int32_t produced;         /* 0: no positive value, or norm == 0 when asked for the intensity */
  int32_t percentile_count;
  uint64_t rank[HALO_STATS_MAX_PERCENTILES]; /* lower rank, 0-based */
  float lo[HALO_STATS_MAX_PERCENTILES], hi[HALO_STATS_MAX_PERCENTILES];      /* order statistics at rank and min(rank + 1, n - 1): raw values, bit-exact */
  double frac[HALO_STATS_MAX_PERCENTILES], value[HALO_STATS_MAX_PERCENTILES]; /* value = lo + (hi - lo) * frac, evaluated in float64 */
} HaloImageStats;
/* Statistics of the values v > 0 (n = positive_count of them; NaN fails the test, +inf passes and orders above every finite value) of the
 * consumer's snapshot Y = sum + compensation (exactly halo_consumer_snapshot's xyz_out[..., 1] and what halo_consumer_auto_ev's fine path reads)
 * or of class lane `plane` as it lies.  Percentile p is numpy's default ("linear"): vi = (p / 100.0) * (double)(n - 1) — the quotient first,
 * then one float64 product — rank = floor(vi), frac = vi - rank, and the two order statistics at rank and min(rank + 1, n - 1), found by ONE
 * radix select for all ranks with no host wait between its passes.  saturated_count counts v / norm > 1 on the float32 quotient; sum and
 * sum_sq come from integer sums per exponent and do not depend on the order of any add.  The whole result is bit-reproducible.  With no
 * positive value — or norm == 0 when the intensity was asked for — only pixel_count, norm and percentile_count are written (the rest is
 * zero).  Reads the consumer only: image, lanes and total intensity stay as they are.  HALO_FATAL (handle still usable) before any fold /
 * consume (plane Y) or without lanes / with a lane index outside halo_set_color's class count (plane >= 0), on NULL arguments, on a
 * percentile outside [0, 100] or a percentile_count outside 0 .. 16. */
int halo_consumer_stats(halo_handle_t h, const HaloStatsSpec* spec, HaloImageStats* out);
/* The rank rule above, as the device evaluates it.  HALO_FATAL for a percentile outside [0, 100], n == 0 or a NULL pointer.  No GPU needed. */
int halo_host_percentile_rank(double percentile, uint64_t n, uint64_t* rank, double* frac);
/* The exact sum behind HaloImageStats::sum (squares = 0: bins[256], per float exponent field e the sum of the 24-bit significands m, hidden
 * bit included, none at e = 0; a value is m * 2^(max(e, 1) - 150)) or ::sum_sq (squares = 1: bins[512], per e the sum of (m * m) & 0xFFFFFF,
 * then per e the sum of (m * m) >> 24), rounded once to the nearest float64, ties to even; +inf when the bins of e = 255 hold anything.  No
 * GPU needed. */
int halo_host_binned_sum(const uint64_t* bins, int32_t squares, double* out);

/* --- view stage: the consumer's image through any lens, gathered on the device (what the reference's preview and export shaders do with
 *     their one full-sky image: gui/preview_renderer.cpp, gui/export_fbo_renderer.hpp; the stage has no counterpart in the backend seam) --- */
typedef struct HaloViewSpec {
  HaloRender view;      /* the lens, fov, size, lens shift, view az / el / roll, visible range and overlap to look through: a session's meaning */
  int32_t has_source;   /* 0: the image was accumulated under the handle's last session's render; 1: under `source` */
  HaloRender source;    /* the render the consumer's image was accumulated under (its size must be the consumer's) */
  HaloDisplay display;  /* halo_consumer_snapshot's display transform */
} HaloViewSpec;
/* For every pixel (px, py) of `view`, row-major:
 *   dir_out  (3 floats) the world-space exit direction w (the trace kernels' convention: the ray's travel direction, sky position -w) that the
 *            view's lens puts on the pixel's CENTRE — the w for which the trace kernels' projection computes the continuous coordinates (px, py)
 *            before its floor(. + 0.5).  Zeros where the pixel has no direction: outside a fisheye's image circle (its rim cz = 0 is culled as the
 *            projection culls it), outside both discs of a dual lens (a disc reaches to the end of its overlap band; the pixel belongs to the
 *            circle that contains its centre), outside |lon| <= pi, |lat| <= pi/2 of the rectangular lens, past the globe's limb (the unit sphere
 *            from distance 4), or where the view's own visible range would have culled the direction (single-view lenses, as in the projection).
 *   map_out  (int32) the row-major index of the source pixel that direction lands on: the projection's PRIMARY hit under `source` (the overlap
 *            write of a dual source is not read) if it lies inside the source frame, else -1.
 *   xyz_out  (3 floats) that pixel's raw value sum + compensation, exactly halo_consumer_snapshot's xyz_out there: nearest neighbour, a copy.
 *            Zeros at -1.
 *   rgb_out  (3 bytes) halo_consumer_snapshot's display transform of that value: rgb_view[p] == rgb_snapshot[map[p]] byte for byte; at -1 what
 *            the snapshot gives a zero pixel.
 * A gather with no Jacobian, like the reference's shader: from an equal-area source (dual fisheye equal area is the reference's choice and the
 * recommended one) the view shows radiance; from any other source it shows the source pixels' energy as it lies.  No filtering (halo_consumer_view_filtered); the class composite and the class lanes have calls of their own below.
 * Host pointers, any of them NULL to skip that output; runs on the backend's stream with one synchronise; reads the consumer only.
 * HALO_FATAL (handle still usable) before any fold / consume, inside a session, with every output NULL, with a source render whose size is not
 * the consumer's, with has_source = 0 on a handle that has had no session, with an empty view or an unknown lens; HALO_UNAVAILABLE for a view of
 * more than 2^25 pixels. */
int halo_consumer_view(halo_handle_t h, const HaloViewSpec* spec, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out);
/* dir_out of one pixel, by the same code on the host: returns 1 and the direction, or 0 and zeros (no direction, a pixel outside the view, NULL
 * arguments).  No GPU needed. */
int halo_host_view_direction(const HaloRender* view, int32_t px, int32_t py, float dir[3]);

/* --- the filtered view: what the reference's shaders do on top of the gather — GL_LINEAR, clamp to edge (gui/preview_renderer.cpp:554-557), and
 *     the cross-fade of a dual fisheye's overlap band (sampleDualFisheye, :152-180) --- */
enum { HALO_VIEW_NEAREST = 0, HALO_VIEW_BILINEAR = 1 };
typedef struct HaloViewFilter {
  int32_t filter;      /* HALO_VIEW_NEAREST: the copy of the view call above; HALO_VIEW_BILINEAR: four taps around the continuous source position */
  int32_t blend;       /* 1: where a dual-fisheye source holds an overlap write for the direction, cross-fade it in; 0: the primary hit alone */
  int32_t reserved[2]; /* zero */
} HaloViewFilter;
/* The view call above with a filter.  dir_out and map_out are that call's: a pixel has a source iff map_out >= 0.  Per pixel that has one:
 *   tap_out  (5 floats) {fx0, fy0, fx1, fy1, t}: the continuous source coordinates of the projection's primary hit — the projection's own fp32
 *            expressions before its floor(. + 0.5): pixel n's centre is n, and floor(fx0 + 0.5), floor(fy0 + 0.5) is map_out's pixel (the rectangular
 *            lens gives the unwrapped column) — and, where the source is a dual fisheye with overlap > 0 and the sky direction has |sz| < max_abs_dz,
 *            those of its overlap write and the tent weight t = (max_abs_dz - |sz|) / (2 max_abs_dz), in fp32; else fx1 = fy1 = t = 0.  Zeros
 *            where map_out is -1.
 *   xyz_out  (3 floats) the sample at (fx0, fy0).  Bilinear: with x0 = floor(fx), ax = fx - x0 (and so for y), taps v = sum + compensation at
 *            columns x0, x0 + 1 and rows y0, y0 + 1 — clamped to the frame; the columns of a rectangular source wrap modulo its width instead —
 *            top = fma(ax, v10 - v00, v00), bot = fma(ax, v11 - v01, v01), c = fma(ay, bot - top, top): every difference and every fma one fp32
 *            rounding.  Nearest: map_out's pixel, a copy.  With blend = 1 and a second hit, c = fma(t, c2 - c, c) with c2 the same sample at
 *            (fx1, fy1) (nearest: the pixel floor(f + 0.5), clamped to the frame).  No source pixel is masked: what no exit was landed on is zero,
 *            and a disc's rim fades into it as the reference's does.  Zeros at -1.
 *   rgb_out  (3 bytes) the snapshot's display transform of xyz_out: it runs on the filtered value, as the shader's does.
 * filter = nearest, blend = 0 gives the view call's bytes.  blend = 1 on a source without an overlap band changes nothing.  No area filter for
 * minified views, no Jacobian.  Refusals are the view call's (every output NULL counts tap_out), plus HALO_FATAL — the handle
 * stays usable — for a NULL filter, an unknown filter, a blend other than 0 or 1, non-zero reserved words. */
int halo_consumer_view_filtered(halo_handle_t h, const HaloViewSpec* spec, const HaloViewFilter* filter, uint8_t* rgb_out, float* xyz_out, int32_t* map_out,
                                float* dir_out, float* tap_out);
/* tap_out of one direction under `source`, by the same code on the host: returns the hit count (0: the projection culls the direction, or NULL
 * arguments / an unknown lens; pos is zeros then) and pos = {fx0, fy0, fx1, fy1, t}.  The frame is not consulted: a hit outside it is returned
 * as it lies.  No GPU needed. */
int halo_host_view_source_pos(const HaloRender* source, const float dir[3], float pos[5]);

/* --- display-side composite of the raypath-colour class lanes (server/component_compositor.cpp) ------------- */
/* CompositeMode (component_compositor.hpp:21): how the per-class Y lanes become one colour per pixel. */
enum { HALO_COMPOSITE_DOMINANT = 0, HALO_COMPOSITE_ADDITIVE = 1, HALO_COMPOSITE_PAINTER = 2 };
/* The display half of a ColorClass (config/color_class_table.hpp:21-35): colour, visibility, solo, draw order.  Entry c belongs
 * to lane c of halo_set_color's `classes`; z_order re-orders the DRAW, never the lane binding (component_compositor.cpp:34-37). */
typedef struct HaloCompositeClass {
  float color[3];
  int32_t z_order;
  int32_t visible; /* ColorClass::visible_ */
  int32_t solo;    /* ColorClass::solo_: if any class is solo, only solo classes take part */
} HaloCompositeClass;
typedef struct HaloComposite {
  int32_t mode;                 /* HALO_COMPOSITE_* */
  float display_exposure_scale; /* GUI EV multiplier; 1 = none */
  float intensity_factor;       /* RenderConfig::intensity_factor_ (ParticipatingExposureScale, render.cpp:120-135) */
  int32_t class_count;          /* must equal the class count of halo_set_color */
  HaloCompositeClass classes[HALO_COLOR_MAX_CLASSES];
} HaloComposite;
/* CompositeColorClassesLinear + LinearRgbToSrgbU8 (component_compositor.cpp:180-303) on the device lanes, which stay as they are
 * (the consumer's lanes: they accumulate over sessions until halo_readback_class_lanes or halo_consumer_reset).  The participating
 * P99 is the exact order statistic the reference takes with nth_element (index = float(count) * 0.99f of the positive lane values
 * of the participating classes), found by a radix select over the float bit patterns; A = intensity_factor * target_linear / P99.
 * *produced = 0 where the reference returns false: no class bit referenced (outputs untouched), or total intensity / P99 zero (P99
 * written, the linear image zeroed as the reference's assign does, :189).  linear_rgb_out: W*H*3 floats, srgb_out: W*H*3 bytes (either
 * may be NULL).  total intensity = what halo_consumer_fold has summed (or halo_consumer_load_lanes set). */
int halo_consumer_composite(halo_handle_t h, const HaloComposite* spec, float* linear_rgb_out, uint8_t* srgb_out,
                            float* participating_p99_y, int32_t* produced);
/* Replace the device lanes with host values (class_count x W x H floats, lane c at lanes[c*W*H + py*W + px]): lanes summed over
 * ranks on the host, or a saved consumer.  total_intensity >= 0 also replaces the consumer's total intensity.  Needs halo_set_color
 * (the lane count is its class count); allocates the lanes when no session has yet. */
int halo_consumer_load_lanes(halo_handle_t h, const float* lanes, int width, int height, int class_count, double total_intensity);
/* ParseCompositeMode (component_compositor.cpp:118-134): "dominant" / "additive" / "painter"; anything else is painter. */
int halo_host_parse_composite_mode(const char* mode);

/* --- the raypath-colour images through any lens: what the reference's preview shader shows in RGB mode — the composited sRGB bytes as its texture
 *     (gui/preview_renderer.cpp:660-678, GL_RGB8), GL_LINEAR taps and sampleDualFisheye's cross-fade, no xyzToSrgb (:458-464) --- */
/* halo_consumer_view_filtered's gather, of halo_consumer_composite's image instead of the consumer's.  Stage 1 composites the source render's
 * image by halo_consumer_composite's code — active classes, participating P99, exposure scale, the composite kernel — into device memory, where
 * it stays; stage 2 gathers the view from its bytes.  Per pixel of `spec->view`, row-major:
 *   map_out    (int32) and
 *   tap_out    (5 floats) are halo_consumer_view_filtered's for the same spec, bit for bit: a pixel has a source iff map_out >= 0.  They do not
 *              depend on the composite and are written whenever the call returns HALO_OK.
 *   value_out  (3 floats) the sample in BYTE units: a tap is the composite's sRGB byte triple as floats, float(b) — the GL texel times 255, an exact
 *              integer, so a constant image stays that constant to the bit — and the taps, the three lerps (each one subtraction and one fma) and the
 *              blend c = fma(t, c2 - c, c) are halo_consumer_view_filtered's.  Zeros at -1 (the shader's final_color = vec3(0)).
 *   srgb_out   (3 bytes) uint8(floorf(value + 0.5f)), the framebuffer's round to nearest; the value lies in [0, 255].  With filter = nearest and
 *              blend = 0: srgb_view[p] == srgb_composite[map[p]], halo_consumer_composite's byte.
 * filter == NULL is nearest without a blend.  spec->display is ignored (the composite carries its own exposure).  The source render — spec->source,
 * or the handle's last session's with has_source = 0 — must have the LANES' size; the consumer's image is not read and no fold is needed: the lanes
 * exist after a colour session or halo_consumer_load_lanes, and stay as they are.  *produced and *participating_p99_y are halo_consumer_composite's:
 * no class bit referenced — *produced = 0, neither image written; no active class — *produced = 1, both images black, P99 0; total intensity or
 * P99 zero — *produced = 0, P99 written, srgb_out untouched, value_out zeroed.  Host pointers, any output NULL to skip it (participating_p99_y may
 * be NULL, produced may not); runs on the backend's stream, the host waiting where the P99 select does and once at the end.
 * HALO_FATAL (handle still usable) for a NULL spec, composite or produced, inside a session, with every output NULL, without lanes, with a source
 * render whose size is not the lanes', with has_source = 0 on a handle that has had no session, with an empty view, an unknown lens, filter or
 * composite mode, a blend other than 0 or 1, non-zero reserved words, a class_count other than halo_set_color's; HALO_UNAVAILABLE for a view of
 * more than 2^25 pixels. */
int halo_consumer_view_composite(halo_handle_t h, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloComposite* composite,
                                 uint8_t* srgb_out, float* value_out, int32_t* map_out, float* tap_out,
                                 float* participating_p99_y, int32_t* produced);
/* The class lanes themselves through the view: lanes_out is float[class_count][view height][view width] for every class of halo_set_color, per
 * class the same sample of float(lane) — the fp64 device lane narrowed per tap, as halo_readback_class_lanes narrows it — with the same taps, lerps
 * and blend; zeros at -1.  No exposure, no composite: what a host with its own compositor, or a per-class analysis of one view, starts from.
 * map_out, tap_out, filter, source and refusals as above; also HALO_UNAVAILABLE for class_count x view pixels of more than 2^27 floats. */
int halo_consumer_view_lanes(halo_handle_t h, const HaloViewSpec* spec, const HaloViewFilter* filter,
                             float* lanes_out, int32_t* map_out, float* tap_out);

/* --- the auxiliary lines over a view: what the reference's preview draws over its image (gui/preview_renderer.cpp overlayAuxLines) — the horizon,
 *     an altitude / azimuth grid, circles of constant angular distance from the sun, zenith and nadir rings, a sun marker — per view pixel from the
 *     direction the gather has already computed.  No text labels, no background image. --- */
#define HALO_VIEW_MAX_SUN_CIRCLES 16
typedef struct HaloViewOverlay {
  int32_t show_horizon, show_grid, show_sun_circles, show_zenith_nadir, show_sun_marker; /* the five layers, each 0 | non-zero */
  float grid_step_deg;                               /* the grid's spacing in altitude and azimuth, > 0 where the grid is on */
  float sun_dir[3];                                  /* the sun's TRAVEL direction (sky position -sun_dir), a unit vector */
  int32_t sun_circle_count;                          /* 0 .. HALO_VIEW_MAX_SUN_CIRCLES */
  float sun_circle_deg[HALO_VIEW_MAX_SUN_CIRCLES];   /* angular distances from the sun in (0, 180] */
  float horizon_color[3], horizon_alpha;             /* every colour channel and every alpha in [0, 1] */
  float grid_color[3], grid_alpha;
  float sun_circles_color[3], sun_circles_alpha;
  float zenith_nadir_color[3], zenith_nadir_alpha;
  float sun_marker_color[3], sun_marker_alpha;
  float zenith_nadir_radius_px;                      /* the rings' radius in view pixels, >= 0 */
  float sun_marker_radius_px;                        /* the disc's radius in view pixels, >= 0 */
  int32_t reserved[2];                               /* zero */
} HaloViewOverlay;
/* The reference's defaults (gui/preview_renderer.hpp OverlayDecoration) into *out: every switch off; circles at 22 and 46 degrees; horizon
 * (0.8, 0.2, 0.2) at 0.6; grid white at 0.3; circles (1, 0.9, 0.3) at 0.5; rings as the horizon, radius 8; marker (1, 0.9, 0.3) at 0.75, radius 5;
 * the grid step by the view's field of view: 30 / 20 / 10 / 5 / 2 / 1 / 0.5 degrees for fov >= 120 / 60 / 30 / 15 / 6 / 2 / below;
 * sun_dir = (-cos alt cos az, -cos alt sin az, -sin alt) of the sun's altitude and azimuth in degrees (NULL: altitude 90, (0, 0, -1)).
 * Returns sizeof(HaloViewOverlay) (0 for a NULL out), which a binding checks against its own mirror of the struct.  No GPU needed. */
int halo_host_view_overlay_defaults(float view_fov_deg, const float sun_alt_az_deg[2], HaloViewOverlay* out);
/* halo_consumer_view_filtered's image with the lines on it (filter == NULL: nearest without a blend).  dir_out and map_out are that call's, bit for
 * bit.  Per view pixel, with w = dir_out, s = overlay->sun_dir and D = 57.29578f, every operation one fp32 rounding:
 *   sky_out    (6 floats) {alt, az, dist, fw_alt, fw_az, fw_dist} in degrees: alt = atan2f(-wz, sqrtf(wx wx + wy wy)) D, az = atan2f(-wy, -wx) D,
 *              dist = atan2f(|w x s|, w . s) D, and the pixel footprints fw(q) = |q(x ^ 1, y) - q| + |q(x, y ^ 1) - q| — a partner outside the view or
 *              without a direction is replaced by the pixel's other neighbour on that axis (x - 1 for even x, x + 1 for odd x), a term with neither
 *              is 0, the azimuth difference is wrapped once into [-180, 180] — clamped to [1e-4, 2] (fw_az: [1e-4, 5]).  Zeros without a direction.
 *   value_out  (3 floats) the colour after the last layer, in byte units: c = float(byte) of the filtered view, then per layer
 *              c = fma(colour * 255, k, c * (1 - k)) — grid, sun circles in list order, horizon, zenith ring, nadir ring, sun marker — with
 *              smoothstep(e0, e1, x) = t t (3 - 2 t), t = clamp((x - e0) / (e1 - e0), 0, 1), cover(d, fw) = 1 - smoothstep(0, 1.5 fw, d),
 *              mod(x, g) = x - g floorf(x / g), h = step / 2 and
 *                grid     k = max(cover(|mod(|alt| + h, step) - h|, fw_alt), cover(|mod(az + 180 + h, step) - h|, fw_az) where |alt| < 85) grid_alpha
 *                circles  k = cover(|dist - angle_i|, fw_dist) sun_circles_alpha
 *                horizon  k = cover(|alt|, fw_alt) horizon_alpha
 *                rings    k = (1 - smoothstep(0, 1.5, |r - radius|)) alpha, r the distance from the pixel's centre to the mark, in pixels
 *                marker   k = (1 - smoothstep(radius - 1.5, radius + 1.5, r)) alpha.
 *              A pixel without a direction keeps float(byte).
 *   rgb_out    (3 bytes) uint8(floorf(clamp(value, 0, 255) + 0.5f)).  With every switch off, or every alpha 0, the filtered view's bytes.
 *   marks_out  (9 floats, not per pixel) {x, y, present} of the zenith (0, 0, -1), the nadir (0, 0, 1) and the sun: halo_host_view_source_pos's
 *              primary hit of that direction under spec->view (pixel n's centre at n); present = 0 and zeros where the projection culls it.
 * The lines are drawn wherever the view has a direction, whether or not the source covers it (map_out = -1).  Host pointers, any output NULL to skip
 * it.  Refusals are halo_consumer_view_filtered's (every output NULL counts all six per-pixel and marks_out), plus HALO_FATAL — the handle stays
 * usable — for a NULL overlay, a colour or alpha outside [0, 1], grid_step_deg <= 0 with the grid on, a circle count outside 0 .. 16, a circle
 * angle outside (0, 180], a negative radius, a sun_dir more than 1e-3 from unit length while circles or marker are on, non-zero reserved words. */
int halo_consumer_view_overlay(halo_handle_t h, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloViewOverlay* overlay, uint8_t* rgb_out,
                               float* value_out, float* sky_out, float* marks_out, int32_t* map_out, float* dir_out);
/* The same pass over halo_consumer_view_composite's srgb: srgb_out, value_out (the colour after the last layer), sky_out, marks_out as above, map_out
 * / tap_out / participating_p99_y / produced that call's, dir_out the view call's.  Where that call writes no composite or a constant one
 * (*produced = 0; no active class) nothing is drawn: the images are that call's.  Refusals: that call's and the overlay's above. */
int halo_consumer_view_composite_overlay(halo_handle_t h, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloComposite* composite,
                                         const HaloViewOverlay* overlay, uint8_t* srgb_out, float* value_out, float* sky_out, float* marks_out,
                                         int32_t* map_out, float* tap_out, float* dir_out, float* participating_p99_y, int32_t* produced);
/* sky_out[0:3] of one direction, and value_out of one pixel that has a direction — base_rgb its 3 bytes, sky6 its sky_out, pixel_xy its integer
 * coordinates as floats, marks9 the call's marks_out — by the same code on the host.  They return 1, or 0 (outputs zeroed) for a NULL argument or a circle count outside 0 .. 16.
 * The record is taken as it is: the refusals above are the calls'.  No GPU needed. */
int halo_host_view_sky(const float dir[3], const float sun_dir[3], float sky3[3]);
int halo_host_view_overlay_pixel(const uint8_t base_rgb[3], const float sky6[6], const float pixel_xy[2], const float marks9[9], const HaloViewOverlay* overlay,
                                 float value3[3]);

/* --- host-side pieces of the path, exported for parity tests (no GPU needed) ---------------- */
/* Geometry tables the kernels consume (reference: Crystal::PopulateFromCfGeom crystal.cpp:304-347,
 * detail::BuildEntrySubTris simulator.cpp:90-129). */
typedef struct HaloGeomTables {
  int32_t face_cnt;                 /* compact present faces */
  float face_n[HALO_MAX_FACES * 3];
  float face_d[HALO_MAX_FACES];
  int32_t face_number[HALO_MAX_FACES];
  int32_t tri_cnt;
  float tri_v[HALO_MAX_TRIS * 9];
  float tri_n[HALO_MAX_TRIS * 3];
  float tri_area[HALO_MAX_TRIS];
  int32_t tri_face[HALO_MAX_TRIS];
} HaloGeomTables;
/* Crystal::CreatePrism(h, dist) — crystal.cpp:349-377. Returns HALO_OK; face_cnt==0 = empty crystal. */
int halo_host_prism_geometry(float h, const float dist[6], HaloGeomTables* out);
/* Crystal::CreatePyramid(wedge_u, wedge_l, h1, h2, h3, dist) — crystal.cpp:379-426. */
int halo_host_pyramid_geometry(float wedge_upper_deg, float wedge_lower_deg, float h1, float h2, float h3,
                               const float dist[6], HaloGeomTables* out);
/* The nine shape scalars [h0, h1, h2, d0..d5] of crystal instance `shape_index` (SyncGroupSampler, simulator.cpp:361-393, over the PCG
 * shape stream): via_plan = 0 walks the draw sequence as the host builder does, 1 draws each scalar from the per-dispatch draw plan the
 * device generators use (one lane per scalar).  The two must agree bit for bit.  Parity-test hook, no device needed. */
int halo_host_shape_scalars(const HaloCrystal* crystal, uint32_t seed, uint64_t shape_index, int via_plan, float out9[9]);
/* Sample crystal instances [first_index, first_index + n) of `crystal` from the backend's shape-scalar stream
 * (MakeCrystal simulator.cpp:448 + SyncGroupSampler :361-393 + closed-form geometry) into `out[n]`:
 * on_device = 1 runs the device generator of the general (4.1 KB) records, 2 — prisms only — the generator of the prism pools' 1360-byte
 * records (one team of 8 lanes per crystal: what a stochastic-prism trace really runs), 0 the host builder.
 * All of them are the same geometry (csrc/halo_geom.h); the tables are bit-equal whenever the draws involve no libm call
 * (fixed / uniform distributions) and equal to float rounding otherwise.  Parity-test hook. */
int halo_generate_shapes(halo_handle_t h, const HaloCrystal* crystal, uint64_t first_index, uint32_t n, int on_device,
                         HaloGeomTables* out);
/* BuildLatLut — lat_lut.cpp:74-204. theta/cdf/flip are HALO_LUT_NODES floats each. */
int halo_host_build_lat_lut(const HaloDist* latitude, float* theta, float* cdf, float* flip);
/* BuildProjParams — lens_proj_build.hpp:79-137 → 19 x 4 bytes laid out as lm_proj::ProjParams. */
int halo_host_build_proj_params(const HaloRender* render, void* proj_params_76_bytes);
/* PartitionCrystalRayNum — simulator.cpp:519-582. carry has n entries and persists across calls. */
int halo_host_partition(const float* proportions, int n, uint64_t ray_num, double* carry, uint64_t* out_counts);
/* Crystal::ReduceRaypath(rp, symmetry, sigma_a, d_applicable) — crystal.cpp:536-600 (hexagonal families, fn_period 6). */
int halo_host_reduce_raypath(const uint8_t* rp, int32_t n, int32_t symmetry, int32_t sigma_a, int32_t d_applicable, uint8_t* out);
/* The emit-gate filter predicate as the production filter kernels evaluate it — DeviceFilterCheck, shared/filter_shared.h:308-315, on the
 * host-built member tables (csrc/halo_device.h FastTables; max_hits <= 16): filter `f` for a crystal with orientation `axis`, asked about an
 * exit with face-number path `path[0..n)` (n <= 16), world direction `dir` and crystal id `crystal_id`.  Writes 1 / 0 to *pass.  HALO_FATAL
 * when the filter does not fit the fast form (the backend then runs the generic kernels).  A host-side test hook: the tests compare it with
 * the reduction-based predicate (halo_host_reduce_raypath) over every short face sequence. */
int halo_host_filter_fast_check(const HaloFilter* f, const HaloAxis* axis, const uint8_t* path, int32_t n, const float dir[3], int32_t crystal_id, int32_t* pass);
/* The raypath-colour pass of the production colour kernels on the host — ApplyLayerColorBits, cuda_trace_backend.cu:498-527; CPU:
 * the colour loop of CollectData, simulator.cpp:689-716 (FilterSpec::CheckSummandMask per predicate): every predicate of `colors`
 * (with its OWN symmetry, evaluated for a crystal with orientation `axis`) that matches the exit ORs its bit into `carried`.
 * Same member tables as halo_host_filter_fast_check (n <= 16).  A host-side test hook for the reference's component-gate vectors. */
int halo_host_color_fast_mask(const HaloColorSet* colors, const HaloAxis* axis, const uint8_t* path, int32_t n, const float dir[3], int32_t crystal_id,
                              uint64_t carried, uint64_t* mask);
/* The scale of a 64-bit fixed-point sum that takes up to `hits` addends of at most `max_w` each: the largest F <= 32 with
 * 4 * max(max_w, 1e-30) * max(hits, 1) * 2^F < 2^62 (the factor 4: a ray's exits never outweigh the ray; x 2 for the second hit of a dual lens, x 2
 * for the CMF rows).  The per-tile passes of the hit log use it with the rays of one launch, option "deterministic" with 2^30 for the planes
 * and 2^32 for the landed integer. */
uint32_t halo_host_fixed_frac_bits(double max_w, uint64_t hits);
/* The size, in wave-passes of 64 rays, of the ticket a wave of a ticketed launch (option "tile_ticket") asks for: the launch has `total` passes, the
 * wave has just read the counter at `seen`, and the rule is clamp((total - seen) / waves, lo, hi) with lo >= 1 — the kernel
 * passes waves = ticket_div x the waves of its grid.  The same function the kernel runs. */
uint32_t halo_host_ticket_size(uint32_t total, uint32_t seen, uint32_t waves, uint32_t lo, uint32_t hi);
/* The launch's `all` wave-passes are cut into halo_host_ticket_groups() ranges with a counter each: range g is passes [*first, *first + *n).  A wave
 * whose home range is `home` (its workgroup's index; taken modulo the number of ranges) and which found the ranges of mask `open` (bit g: range g
 * has passes left) unfinished turns to range halo_host_ticket_next(open, home): the first at or after home, wrapping round; the number of
 * ranges when open is 0.  The same functions the kernel runs. */
uint32_t halo_host_ticket_groups(void);
void halo_host_ticket_range(uint32_t all, uint32_t g, uint32_t* first, uint32_t* n);
uint32_t halo_host_ticket_next(uint64_t open, uint32_t home);
/* IceRefractiveIndex::Get — optics.cpp:180-197. */
double halo_host_refractive_index(double wavelength_nm);
/* GetIlluminantSpd(type, wavelength) — util/illuminant.cpp:113-134 (HALO_ILLUM_*; 0 outside the tabulated range). */
float halo_host_illuminant_spd(int illuminant, float wavelength_nm);
/* ComputeWlPool — core/backend/wl_pool.hpp:67-91: the session's wavelength entries as the kernels read them, 5 floats each
 * {refractive index, SPD weight, cmf_x, cmf_y, cmf_z}; a discrete HaloWl gives one entry.  Returns the entry count (<= cap
 * entries are written), 0 on error. */
int halo_host_wl_pool(const HaloWl* wl, float* entries5, int cap);
/* The spectrum entry of root r among the m roots of one crystal entry's share in a spectrum session of `count` entries (halo_begin_spectrum):
 * min(r / ceil(m / count), count - 1), evaluated by the function the kernels call, with the per-launch constants the host hands them — for two
 * different cuts of the share into launches, which must agree (0xFFFFFFFF if they did not).  Parity-test hook, no device needed. */
uint32_t halo_host_spectrum_entry(uint64_t m, uint32_t count, uint64_t r);
int halo_abi_version(void);
/* sizeof() of boundary structs as compiled (0 scene, 1 render, 2 wl, 3 exit record, 4 geom tables, 5 layer stats, 6 entry, 7 colour set, 8 colour class, 9 filter, 10 route info, 11 composite, 12 auto ev, 13 stats spec, 14 image stats, 15 view spec). */
uint64_t halo_abi_sizeof(int which);

#ifdef __cplusplus
}
#endif

/* Layout pins of every struct that crosses the boundary (LP64, natural alignment).  A field added, removed or re-typed on
 * either side of the ABI — here, in a binding (ice_halo_sim_amd/abi.py checks the same numbers through halo_abi_sizeof), or
 * in the reference-side glue (integration/hip_backend_glue.hpp) — fails to compile instead of shifting what the kernels read. */
#if defined(__cplusplus)
#define HALO_STATIC_ASSERT(c, m) static_assert(c, m)
#elif defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define HALO_STATIC_ASSERT(c, m) _Static_assert(c, m)
#else
#define HALO_STATIC_ASSERT(c, m)
#endif
HALO_STATIC_ASSERT(sizeof(HaloDist) == 12, "HaloDist");
HALO_STATIC_ASSERT(sizeof(HaloAxis) == 36, "HaloAxis");
HALO_STATIC_ASSERT(sizeof(HaloCrystal) == 4 + 9 * 12 + 9 * 4 + 8, "HaloCrystal");
HALO_STATIC_ASSERT(sizeof(HaloEntry) == sizeof(HaloCrystal) + sizeof(HaloAxis) + 16, "HaloEntry");
HALO_STATIC_ASSERT(sizeof(HaloFilterTerm) == 8 + HALO_MAX_HITS + 16 + 8 + 12 + 4, "HaloFilterTerm");
HALO_STATIC_ASSERT(sizeof(HaloFilter) == 16 + 4 * HALO_FILTER_MAX_OR + HALO_FILTER_MAX_TERMS * sizeof(HaloFilterTerm), "HaloFilter");
HALO_STATIC_ASSERT(sizeof(HaloColorTerm) == sizeof(HaloFilterTerm) + 8, "HaloColorTerm");
HALO_STATIC_ASSERT(sizeof(HaloColorSet) == 8 + HALO_COLOR_MAX_TERMS * sizeof(HaloColorTerm), "HaloColorSet");
HALO_STATIC_ASSERT(sizeof(HaloColorClass) == 16, "HaloColorClass");
HALO_STATIC_ASSERT(sizeof(HaloLayer) == 8 + HALO_MAX_ENTRIES * sizeof(HaloEntry), "HaloLayer");
HALO_STATIC_ASSERT(sizeof(HaloScene) == 20 + HALO_MAX_LAYERS * sizeof(HaloLayer), "HaloScene");
HALO_STATIC_ASSERT(sizeof(HaloRender) == 44, "HaloRender");
HALO_STATIC_ASSERT(sizeof(HaloWl) == 16, "HaloWl");
HALO_STATIC_ASSERT(sizeof(HaloHostRays) == 5 * sizeof(void*), "HaloHostRays");
HALO_STATIC_ASSERT(sizeof(HaloLayerStats) == 56, "HaloLayerStats");
HALO_STATIC_ASSERT(sizeof(HaloExitRecord) == 40 + HALO_PATH_CAP, "HaloExitRecord");
HALO_STATIC_ASSERT(sizeof(HaloRouteInfo) == 40, "HaloRouteInfo");
HALO_STATIC_ASSERT(sizeof(HaloDisplay) == 28, "HaloDisplay");
HALO_STATIC_ASSERT(sizeof(HaloAutoEv) == 28, "HaloAutoEv");
HALO_STATIC_ASSERT(sizeof(HaloStatsSpec) == 16 + 8 * HALO_STATS_MAX_PERCENTILES, "HaloStatsSpec");
HALO_STATIC_ASSERT(sizeof(HaloImageStats) == 56 + 32 * HALO_STATS_MAX_PERCENTILES, "HaloImageStats");
HALO_STATIC_ASSERT(sizeof(HaloViewSpec) == 44 + 4 + 44 + 28, "HaloViewSpec");
HALO_STATIC_ASSERT(sizeof(HaloViewFilter) == 16, "HaloViewFilter");
HALO_STATIC_ASSERT(sizeof(HaloViewOverlay) == 20 + 4 + 12 + 4 + 4 * HALO_VIEW_MAX_SUN_CIRCLES + 5 * 16 + 8 + 8, "HaloViewOverlay");
HALO_STATIC_ASSERT(sizeof(HaloCompositeClass) == 24, "HaloCompositeClass");
HALO_STATIC_ASSERT(sizeof(HaloComposite) == 16 + HALO_COLOR_MAX_CLASSES * 24, "HaloComposite");
HALO_STATIC_ASSERT(sizeof(HaloGeomTables) == 4 + HALO_MAX_FACES * 20 + 4 + HALO_MAX_TRIS * (36 + 12 + 4 + 4), "HaloGeomTables");
#endif /* HALO_TRACE_H_ */
