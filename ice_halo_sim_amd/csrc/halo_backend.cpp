// halo_backend.cpp — the C ABI of include/halo_trace.h: session state machine, per-(layer, entry) dispatch, device memory, streams/events, the
// fixed-point import / export and the shards.  Host C++ only; kernels live in halo_trace.inl (+ halo_trace_m*.hip) and halo_kernels.hip.
// Its neighbours: halo_state.h (the state and the helpers the units share), halo_options.h (the option table halo_set_option asks),
// halo_order.h (the streams and everything that orders them: b->ord),
// halo_consumer.cpp (the consumer stages), halo_host_abi.cpp (every export that takes no handle).
//
// State machine (reference trace_backend.hpp:91-116):
//   halo_begin → (halo_trace_layer → halo_recombine)* → halo_trace_layer → halo_end ; halo_readback_xyz any time.
// There is no CPU fallback in this library: every entry point that computes needs a gfx950 device and fails
// with HALO_UNAVAILABLE otherwise.
#include <cstdlib>
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "halo_state.h"

#ifndef HALO_XYZ_LOG_MIN_PIX
#define HALO_XYZ_LOG_MIN_PIX (1u << 19)   // illuminant sessions on images ABOVE this many pixels take the X/Y/Z hit log (below: one scalar plane per pool entry)
#endif

using namespace halo;

// ---- the helpers every unit calls (declared in halo_state.h) ----
namespace halo {

int fail(HaloBackend* b, int code, const std::string& msg) {
  if (b) b->error = msg;
  return code;
}
int hip_fail(HaloBackend* b, hipError_t e, const char* what) {
  return fail(b, (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorOutOfMemory) ? HALO_UNAVAILABLE : HALO_FATAL,
              std::string(what) + ": " + hipGetErrorString(e));
}
void drop_table_cache(HaloBackend* b) {
  for (auto& layer : b->tcache)
    for (auto& e : layer) e.valid = false;
}
}  // namespace halo

namespace {

// The plane set the open / pending session adds to (HaloBackend::mono_two).
inline float* planes_of(HaloBackend* b) { return b->mono.ptr + (b->mono_two ? static_cast<size_t>(b->mono_set) * b->mono_half : 0u); }
// Smallest launch the hit log takes by itself (option hit_log = -1).  Direct atomics retire memory-side at ~21 G/s whatever they hit; the log's
// passes cost a fixed ~75 us per launch plus ~10 ps per record, and on a small launch they run beside the next session's trace kernel.  A
// full-sky render lands every exit (5-6 per root: 0.8 M roots = 4.4 M atomics = 210 us against 102 us of logged trace kernel, bench.py --config 4d),
// a lens that sees part of the sky 1-2 per root.
inline uint64_t log_min_rays(int visible) { return visible == HALO_VISIBLE_FULL ? (1ull << 19) : (2ull << 20); }
// The cumulative landed tally up to here belongs to the OWNED image that is being left (re-sized: its light is discarded with it): whoever
// reads the new image must not be handed weight that landed in the old one and was never taken.
int forget_landed(HaloBackend* b) {
  if (!b->tally.ptr) return HALO_OK;
  if (int rc = join_aux(b)) return rc;
  double unused = 0.0;
  return take_landed_delta(b, &unused);
}

int ensure_accumulator(HaloBackend* b, int w, int h) {
  const uint64_t need = static_cast<uint64_t>(w) * h * 3 + 4;
  if (b->acc && b->acc != b->acc_own.ptr) {  // external binding
    if (b->acc_floats < need) return fail(b, HALO_FATAL, "bound accumulator smaller than width*height*3+4 floats");
    b->acc_w = w;
    b->acc_h = h;
    return HALO_OK;
  }
  // own_w/own_h describe the OWNED buffer's image (acc_w/acc_h are also written by the external-binding path above, so they
  // cannot decide whether the owned buffer fits); capacity is checked on its own
  if (!b->acc_own.ptr || b->acc_own.cap < need || b->own_w != w || b->own_h != h) {
    if (int rc = reserve_idle(b, b->acc_own, need)) return rc;
    if (int rc = join_aux(b)) return rc;   // (a fold of the old image may still be queued there)
    if (b->own_w != 0 || b->own_h != 0)
      if (int rc = forget_landed(b)) return rc;   // the old image goes, and its landed weight with it
    HIPCHK(b, hipMemsetAsync(b->acc_own.ptr, 0, need * sizeof(float), main_q(b)));
    b->own_w = w;
    b->own_h = h;
  }
  b->acc_w = w;
  b->acc_h = h;
  b->acc = b->acc_own.ptr;
  b->acc_floats = need;
  return HALO_OK;
}

// take the timing of one finished ring slot (the tallies are cumulative device counters: pull_tally)
void harvest_slot(HaloBackend* b, Order::RingSlot& r) {
  if (!r.busy) return;
  (void)hipEventSynchronize(r.fin);
  float ms = 0.0f, ms2 = 0.0f;
  (void)hipEventElapsedTime(&ms, r.ev0, r.ev1);
  if (r.posts) (void)hipEventElapsedTime(&ms2, r.t2, r.ev3);   // the passes' own span
  static const bool debug_timing = std::getenv("HALO_DEBUG_TIMING") != nullptr;
  if (debug_timing) std::fprintf(stderr, "[halo timing] slot %d final %d posts %d trace %.4f ms passes %.4f ms\n", int(&r - b->ord.ring), int(r.final), int(r.posts), ms, ms2);
  // An event pair that reads backwards (seen once: two twelve-launch runs of one bench process summed to -10 ms; the rocprofv3 trace of the same
  // command had every kernel in order) is a measurement that did not happen: it is left out of the timing sums and of their launch count.
  const bool timed = ms >= 0.0f && ms2 >= 0.0f;
  if (timed) b->layer_acc.kernel_ms += ms + ms2;
  if (r.final && timed) {
    b->time_trace_ms += ms;
    b->time_post_ms += ms2;
    b->time_launches += 1;
  }
  b->layer_acc.launches += 1;
  r.busy = false;
}
// Snapshot of the cumulative tallies (one 1 KB D2H copy + a stream sync): the sum over the lines, per tally.
int read_tally(HaloBackend* b, double out[kSumNum], unsigned long long* fix_landed = nullptr) {
  HIPCHK(b, hipMemcpyAsync(b->tally_host.ptr, b->tally.ptr, kTallyLines * kTallyStride * sizeof(double), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  if (fix_landed) {   // the lines' integer slot (deterministic sessions), summed modulo 2^64
    *fix_landed = 0ull;
    for (uint32_t l = 0; l < kTallyLines; l++) {
      unsigned long long v;
      std::memcpy(&v, &b->tally_host.ptr[l * kTallyStride + kSumFixLanded], sizeof(v));
      *fix_landed += v;
    }
  }
  for (int t = 0; t < kSumNum; t++) {
    double v = 0.0;
    for (uint32_t l = 0; l < kTallyLines; l++) v += b->tally_host.ptr[l * kTallyStride + static_cast<uint32_t>(t)];
    out[t] = v;
  }
  return HALO_OK;
}
// What the kernels have tallied since the statistics were last pulled goes to layer_acc (exit weight, exit count, pixel hits).
int pull_tally(HaloBackend* b) {
  if (!b->tally_unread) return HALO_OK;
  double now[kSumNum];
  int rc = read_tally(b, now);
  if (rc != HALO_OK) return rc;
  b->layer_acc.exit_w_sum += now[kSumExitW] - b->tally_seen[kSumExitW];
  b->layer_acc.exit_count += static_cast<uint64_t>(now[kSumExitN] - b->tally_seen[kSumExitN] + 0.5);
  b->layer_acc.pixel_hits += static_cast<uint64_t>(now[kSumPixN] - b->tally_seen[kSumPixN] + 0.5);
  for (int t : {kSumExitW, kSumExitN, kSumPixN}) b->tally_seen[t] = now[t];
  b->tally_unread = false;
  return HALO_OK;
}
}  // namespace

namespace halo {
// The landed weight since the last taker (readback, take_landed, consumer fold).
int take_landed_delta(HaloBackend* b, double* landed) {
  double now[kSumNum];
  unsigned long long fix_now = 0ull;
  int rc = read_tally(b, now, &fix_now);
  if (rc != HALO_OK) return rc;
  // (deterministic sessions land as an integer in units of 2^-F_L: exact in the integer, one conversion here)
  *landed = now[kSumLanded] - b->tally_seen[kSumLanded] + std::ldexp(static_cast<double>(fix_now - b->fix_landed_seen), -static_cast<int>(b->fix_frac_landed)) + b->landed_carry;
  b->tally_seen[kSumLanded] = now[kSumLanded];
  b->fix_landed_seen = fix_now;
  b->landed_carry = 0.0;
  return HALO_OK;
}
}  // namespace halo

namespace {

void harvest_all(HaloBackend* b) {
  for (Order::RingSlot& r : b->ord.ring) harvest_slot(b, r);
}
void add_stats(HaloLayerStats& dst, const HaloLayerStats& src) {
  dst.root_count += src.root_count;
  dst.exit_count += src.exit_count;
  dst.continuation_count += src.continuation_count;
  dst.exit_w_sum += src.exit_w_sum;
  dst.kernel_ms += src.kernel_ms;
  dst.pixel_hits += src.pixel_hits;
  dst.launches += src.launches;
}
const host::LatLut& cached_lut(HaloBackend* b, const HaloDist& d) {
  for (const auto& e : b->lut_cache)
    if (e.type == d.type && e.center == d.center && e.spread == d.spread) return e.lut;
  if (b->lut_cache.size() >= 64) b->lut_cache.clear();
  b->lut_cache.push_back({d.type, d.center, d.spread, host::BuildLatLut(d)});
  return b->lut_cache.back().lut;
}

}  // namespace

static int fold_queue(HaloBackend* b);

extern "C" {

int halo_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int halo_create(int device_ordinal, uint32_t seed, halo_handle_t* out) {
  if (!out) return HALO_FATAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n) return HALO_UNAVAILABLE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_ordinal) != hipSuccess) return HALO_UNAVAILABLE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HALO_UNAVAILABLE;  // this library carries gfx950 code only
  auto* b = new HaloBackend();
  b->device = device_ordinal;
  b->seed = seed ? seed : 1u;
  b->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  // (whatever exists when a step fails goes in halo_destroy: the streams and the events with b->ord, the ring and the pinned mirrors with the handle)
  if (hipSetDevice(device_ordinal) != hipSuccess || b->ord.create() != hipSuccess || b->slots_dev.reserve(Order::kRing) != hipSuccess ||
      b->slots_host.alloc(Order::kRing) != hipSuccess || b->tally_host.alloc(kTallyLines * kTallyStride) != hipSuccess ||
      b->tally.reserve(kTallyLines * kTallyStride) != hipSuccess || b->counters.reserve(kCntNum) != hipSuccess) {
    halo_destroy(b);
    return HALO_UNAVAILABLE;
  }
  (void)hipMemsetAsync(b->tally.ptr, 0, kTallyLines * kTallyStride * sizeof(double), main_q(b));
  (void)hipMemsetAsync(b->counters.ptr, 0, kCntNum * sizeof(uint32_t), main_q(b));
  *out = b;
  return HALO_OK;
}

int halo_destroy(halo_handle_t b) {
  if (!b) return HALO_OK;
  (void)hipSetDevice(b->device);
  b->ord.destroy();   // the streams are synchronised, then the events go, then the streams
  delete b;   // every buffer frees itself (DevBuf, PinnedBuf): the streams were synchronised above
  return HALO_OK;
}

const char* halo_last_error(halo_handle_t b) { return b ? b->error.c_str() : "null handle"; }

// The rules — keys, value rules, refusals, what counts as a change — are halo_options.h set_option's, which needs no device; here its verdict is
// carried out: the effects first, and only then the value.  A refused set leaves nothing behind.
int halo_set_option(halo_handle_t b, const char* key, int64_t v) {
  if (!b || !key) return HALO_FATAL;
  // (the kernels' grid-stride index is 32-bit: n_rays + one stride of workgroups must stay below 2^32)
  const uint64_t chunk_top = (1ull << 32) - (static_cast<uint64_t>(b->cu_count) * 64ull * kBlock) - kBlock;
  const OptionSet set = set_option(b->opt, b->in_session, b->shard_count, chunk_top, key, v);
  if (set.status == OptionSet::kRefused) return fail(b, HALO_FATAL, set.message);
  if (set.effects & kFxFoldPlanes)
    if (int rc = fold_if_dirty(b)) return rc;   // planes of ended sessions may still wait for their fold (lazy_fold)
  if (set.effects & kFxSync)
    if (int rc = sync_all(b)) return rc;        // (nothing may still be reading what is freed, or be queued by the other overlap rule)
  if (set.effects & kFxReleasePlanes) b->mono.release();
  if (set.effects & kFxDropCache) drop_table_cache(b);
  if (set.effects & kFxCounters) b->gen_count = b->gate_count = b->transit_count = b->shape_count = set.counter_base;
  if (set.effects & kFxSeed) b->seed = static_cast<uint32_t>(set.value);
  set.commit(b->opt);
  return HALO_OK;
}

int halo_set_stream(halo_handle_t b, void* s) {
  if (!b) return HALO_FATAL;
  b->ord.set_main(static_cast<hipStream_t>(s));   // (host waits for all streams first; no stream: the handle's own again)
  return HALO_OK;
}

int halo_bind_accumulator(halo_handle_t b, void* device_ptr, uint64_t n_floats) {
  if (!b) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "bind_accumulator inside a session");
  if (int rc = fold_if_dirty(b)) return rc;   // planes of ended sessions belong to the accumulator they were traced for
  // (The landed tally is NOT touched: it belongs to the sessions traced, and goes to whoever takes it — halo_take_landed, a readback — whichever
  //  tensor holds their light.  A caller that alternates two bound tensors, dist.ShardedTracer's drain, rebinds with nothing waiting on the host.)
  if (!device_ptr) {
    b->acc = b->acc_own.ptr;
    b->acc_floats = b->acc_own.cap;
    return HALO_OK;
  }
  b->acc = static_cast<float*>(device_ptr);
  b->acc_floats = n_floats;
  return HALO_OK;
}

int halo_set_filters(halo_handle_t b, const HaloFilter* filters, int32_t count) {
  if (!b || count < 0 || (count > 0 && !filters)) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "set_filters inside a session");
  for (int32_t i = 0; i < count; i++) {
    const HaloFilter& f = filters[i];
    int terms = f.is_complex ? 0 : 1;
    if (f.is_complex) {
      if (f.or_count < 0 || f.or_count > HALO_FILTER_MAX_OR) return fail(b, HALO_FATAL, "complex filter: too many OR-clauses");
      for (int o = 0; o < f.or_count; o++) terms += f.and_counts[o];
      if (terms > HALO_FILTER_MAX_TERMS) return fail(b, HALO_FATAL, "complex filter: too many terms");
    }
  }
  // (the Lumice glue hands the filter table over at every BeginSession: equal tables keep the table cache — ADVICE r5)
  const bool same = static_cast<size_t>(count) == b->filters.size() && (count == 0 || std::memcmp(b->filters.data(), filters, sizeof(HaloFilter) * static_cast<size_t>(count)) == 0);
  if (same) return HALO_OK;
  b->filters.assign(filters, filters + count);
  drop_table_cache(b);
  return HALO_OK;
}


// BeginSession for both entry points.  spec_n >= 2: a spectrum session over the discrete entries spec[0 .. spec_n) (halo_begin_spectrum; `wl` is then
// spec[0], kept for the members that describe "the session's wavelength"); spec_n == 0: halo_begin's session of `wl`.
static int begin_session(halo_handle_t b, const HaloScene* scene, const HaloRender* render, const HaloWl* wl, const HaloWl* spec, int32_t spec_n, uint64_t ray_num) {
  if (!b || !scene || !render || !wl) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "BeginSession inside a session");
  if (scene->layer_count < 1 || scene->layer_count > HALO_MAX_LAYERS) return fail(b, HALO_FATAL, "layer_count out of range");
  if (scene->max_hits < 1 || scene->max_hits > HALO_MAX_HITS) return fail(b, HALO_FATAL, "max_hits out of range");
  if (render->width <= 0 || render->height <= 0) return fail(b, HALO_FATAL, "bad resolution");
  bool plain_scene = !b->opt.capture;   // no filter, raypath colour or capture anywhere: every launch runs the production kernels
  for (int l = 0; l < scene->layer_count; l++) {
    if (scene->layers[l].entry_count < 1 || scene->layers[l].entry_count > HALO_MAX_ENTRIES)
      return fail(b, HALO_FATAL, "entry_count out of range");
    for (int e = 0; e < scene->layers[l].entry_count; e++) {
      const int fid = scene->layers[l].entries[e].filter_id;
      if (fid < 0 || fid > static_cast<int>(b->filters.size())) return fail(b, HALO_FATAL, "entry refers to a filter_id outside the table");
      const int cid = scene->layers[l].entries[e].color_id;
      if (cid < 0 || cid > static_cast<int>(b->color_sets.size())) return fail(b, HALO_FATAL, "entry refers to a color_id outside the table");
      if (fid > 0 || cid > 0) plain_scene = false;
      const int kind = scene->layers[l].entries[e].crystal.kind;
      if (kind != HALO_CRYSTAL_PRISM && kind != HALO_CRYSTAL_PYRAMID) return fail(b, HALO_FATAL, "unknown crystal kind");
    }
  }
  if (b->shard_count > 1 && scene->layer_count > 1)
    return fail(b, HALO_FATAL, "halo_set_shard count > 1: a multi-layer scene is not supported (the next layer's pool order and shuffle are global over all roots; shards do not exchange continuation pools)");
  const bool det = b->opt.deterministic != 0;
  if (det) {
    // A deterministic session runs the kAccFixed kernels or nothing: what they do not cover is refused here, by name, before any state changes —
    // never run on a float route in silence.
    if (scene->layer_count > 1 && !b->opt.cont_order)
      return fail(b, HALO_FATAL, "deterministic = 1: a multi-layer session needs cont_order = 1 (the continuation pool's append order decides which rays the next layer traces)");
    if (!b->color_classes.empty() || !b->color_sets.empty()) return fail(b, HALO_FATAL, "deterministic = 1: raypath-colour tables are set (the class lanes are fp64 atomics)");
    if (b->opt.capture) return fail(b, HALO_FATAL, "deterministic = 1: capture_exits = 1 is not supported (the capture kernels have no fixed-point route)");
    if (b->opt.rehit_strategy == 0) return fail(b, HALO_FATAL, "deterministic = 1: rehit_strategy = 0 is not supported (the legacy strategy lives in the generic kernels)");
    for (int l = 0; l < scene->layer_count; l++)
      for (int e = 0; e < scene->layers[l].entry_count; e++) {
        const HaloEntry& E = scene->layers[l].entries[e];
        if (E.filter_id <= 0) continue;
        const FilterDev fd = host::BuildFilter(b->filters[static_cast<size_t>(E.filter_id - 1)], E.axis);
        if (!(fd.is_complex || fd.terms[0].type != HALO_FILTER_NONE || fd.action != 0)) continue;   // a filter that passes everything: the plain kernels
        std::unique_ptr<FastTables> ft(new FastTables());
        std::memset(ft.get(), 0, sizeof(FastTables));
        if (!b->opt.filter_fast || scene->max_hits > 16 ||
            !host::BuildFastTables(&b->filters[static_cast<size_t>(E.filter_id - 1)], nullptr, E.axis, static_cast<uint32_t>(E.crystal_config_id), *ft))
          return fail(b, HALO_FATAL, "deterministic = 1: a filter of this scene needs the generic filter kernels (filter_fast = 0, max_hits > 16, or tables that do not fit the fast form)");
      }
  }
  HIPCHK(b, hipSetDevice(b->device));
  // (the cached slots hold the session's wavelength pool: a spectrum session's key is its whole entry table)
  const bool same_spec = b->tcache_spec.size() == static_cast<size_t>(spec_n) &&
                         (spec_n == 0 || std::memcmp(b->tcache_spec.data(), spec, sizeof(HaloWl) * static_cast<size_t>(spec_n)) == 0);
  if (std::memcmp(&b->tcache_scene, scene, sizeof(HaloScene)) != 0 || std::memcmp(&b->tcache_wl, wl, sizeof(HaloWl)) != 0 || !same_spec) {
    drop_table_cache(b);   // another scene, wavelength or spectrum: the cached tables are not this session's
    b->tcache_scene = *scene;
    b->tcache_wl = *wl;
    b->tcache_spec.assign(spec, spec + spec_n);
  }
  b->scene = *scene;
  b->render = *render;
  b->had_session = true;
  b->wl = *wl;
  b->proj = host::BuildProj(*render);
  std::vector<WlEntryDev> pool = host::BuildWlPool(*wl);
  for (int32_t k = 1; k < spec_n; k++) {   // a spectrum session's pool: what each entry's own discrete session would read, one behind the other
    const std::vector<WlEntryDev> one = host::BuildWlPool(spec[k]);
    pool.insert(pool.end(), one.begin(), one.end());
  }
  b->spec_count = static_cast<uint32_t>(spec_n);
  b->wl_pool_size = static_cast<uint32_t>(pool.size());
  if (pool.empty() || pool.size() > HALO_WL_POOL_MAX) return fail(b, HALO_FATAL, "wavelength pool size out of range");
  b->wl_pool_host = pool;  // travels to the device inside each dispatch slot
  b->sess_max_w = 0.0;     // no ray of this session weighs more (continuations only lose weight): bounds the per-tile fixed-point sums
  for (const WlEntryDev& e : pool) b->sess_max_w = std::max(b->sess_max_w, static_cast<double>(std::fabs(e.spd_weight)));
  // Accumulation planes of this session (kernels never touch the XYZ image; halo_fold_kernel closes the session):
  //  * discrete wavelength: ONE scalar plane, coefficient = CMF(lambda)            (1 atomic per hit)
  //  * illuminant, batch >= 8 Mi rays: one scalar plane per pool entry, coefficient = its CMF (1 atomic per hit, fold reads M planes)
  //  * illuminant, small batch or "mono" = 0: X, Y, Z planes, unit coefficients        (3 atomics per hit, cheap fold)
  const size_t npix = static_cast<size_t>(render->width) * render->height;
  // 2^25 pixels (an 8192x4096 panorama) is what the workgroup cache's 32-bit key names on its own; with a plane index beside the pixel the
  // key keeps 23 bits for the pixel, so sessions above 2^23 pixels take the layouts without per-entry planes (below: mono_by_wl)
  if (npix > (1u << 25)) return fail(b, HALO_UNAVAILABLE, "more than 2^25 pixels");   // recoverable: the caller falls back (INTEGRATION.md limits table)
  // (a spectrum session is a pool session wherever layouts are chosen: per-ray entries, X/Y/Z or per-entry planes)
  const bool discrete = wl->illuminant < 0 && spec_n == 0;
  //  * illuminant, batch >= 2 Mi rays, hit log on (the default): X, Y, Z planes too, but the launches log {slot, pool entry, w} and
  //    the per-tile pass applies the CMF (halo_log_accumulate_kernel<3>): no plane per entry, no two-level split, a 3-plane fold
  //    (images above 512 Ki pixels: on small ones most hits land in the pixel cache, and the X/Y/Z cache pays three fp32 LDS adds — the
  //    slow kind on gfx950 — per hit where a scalar plane pays one: the reference's 512x256 D65 scene runs 2.8 vs 8.0 G rays/s)
  uint32_t s_log2 = 6;  // columns per plane row: at least one fold tile
  while ((static_cast<size_t>(kMonoRows) << s_log2) < npix) s_log2++;
  // the log's tile layout has limits (plan_route: log_layout_ok): X/Y/Z records keep the slot in 23 bits of which the per-tile pass
  // takes <= 4 Ki-slot tiles x 512, scalar planes 16 Ki-slot tiles x 256.  A session the log cannot serve keeps the routes it had before
  // (one plane per pool entry + binned lists; privatised copies for the direct atomics).
  const bool log_xyz_fits = s_log2 <= 11u, log_mono_fits = s_log2 <= 12u;
  // (the layout is worked out in locals first: whether the planes of earlier sessions must be folded before this one starts depends on it)
  const bool xyz_log_n = !det && b->opt.mono_enabled && !discrete && b->opt.lambda_planes < 0 && b->opt.hit_log != 0 && ray_num >= (2ull << 20) && npix > HALO_XYZ_LOG_MIN_PIX && log_xyz_fits;
  const bool mono_by_wl_n = !det && b->opt.mono_enabled && !discrete && !xyz_log_n && npix <= (1u << 23) && (b->opt.lambda_planes < 0 ? ray_num >= (8ull << 20) : b->opt.lambda_planes != 0);
  const bool mono_session_n = b->opt.mono_enabled && (discrete || mono_by_wl_n);
  const uint32_t plane_cnt_n = mono_by_wl_n ? static_cast<uint32_t>(pool.size()) : (mono_session_n ? 1u : 3u);
  // privatised copies spread the direct atomics of hot pixels; per-entry planes spread them already, and a session whose
  // launches all go through the hit log (copy 0 only) would just make the closing fold read seven empty copies
  // ("all" cannot be known here: a layer's rays are dealt out to its crystal entries, and an entry's launch under 2 Mi rays adds directly.
  // So the copies go only when every layer has ONE entry — a layer is then launches of the whole batch, and what may still fall under the
  // threshold, a last chunk or a thin continuation layer, is little work by definition)
  bool one_entry_layers = true;
  for (int l = 0; l < scene->layer_count; l++) one_entry_layers = one_entry_layers && scene->layers[l].entry_count == 1;
  const bool fast_scene = b->opt.rehit_strategy != 0 && (plain_scene || (!b->opt.capture && b->opt.filter_fast && scene->max_hits <= 16));   // (a dispatch whose tables do not fit the fast form still adds directly: copy 0 only, correct, slower)
  const bool all_logged = !det && fast_scene && one_entry_layers && b->opt.hit_log < 0 && b->opt.aggregate == 1 && ray_num >= (discrete ? log_min_rays(render->visible) : (2ull << 20)) &&
                          (discrete ? log_mono_fits : xyz_log_n) && (mono_session_n || xyz_log_n);
  // (a deterministic session: one scalar plane or X, Y, Z, one copy — integer atomics onto HaloBackend::fix; hit_log, bin, lambda_planes and mono_copies do not apply)
  const uint32_t plane_copies_n = (mono_by_wl_n || all_logged || det) ? 1u : static_cast<uint32_t>(b->opt.mono_copies);
  const bool two_sets_n = all_logged && discrete && mono_session_n && !mono_by_wl_n && b->opt.overlap != 0;   // (see HaloBackend::mono_two)
  std::vector<std::array<float, 3>> coef_n;
  for (uint32_t m = 0; m < plane_cnt_n; m++) {
    if (mono_session_n) coef_n.push_back({pool[m].cmf_x, pool[m].cmf_y, pool[m].cmf_z});
    else coef_n.push_back({m == 0 ? 1.0f : 0.0f, m == 1 ? 1.0f : 0.0f, m == 2 ? 1.0f : 0.0f});
  }
  {
    // Planes that earlier sessions left unfolded (lazy_fold: halo_end of a session on the backend's own accumulator does not fold) stay as
    // they are when this session adds to the SAME planes with the SAME coefficients — a server that sends one wavelength's rays as many small
    // sessions (Lumice's CUDA-route dispatch is 2^18 rays, server.cpp:151) then pays one fold per readback instead of one per session (22 us
    // of a 0.15 ms session at 1920x1080 x 8 copies).  Anything else — another wavelength, image size, plane count or copy count — is folded
    // now, with the members still describing the old planes.
    const bool same_planes = b->mono_dirty && b->opt.lazy_fold && b->acc != nullptr && b->acc == b->acc_own.ptr && b->acc_w == render->width &&
                             b->acc_h == render->height && b->mono_s_log2 == s_log2 && b->plane_cnt == plane_cnt_n && b->plane_copies == plane_copies_n &&
                             b->mono_two == two_sets_n && b->plane_coef == coef_n && b->fix_planes == det;
    if (!same_planes) {
      // (queued on the auxiliary stream; the HOST does not wait.  This session's launches whose trace kernel adds to the planes, and its logged
      // launches that fill the chip, are queued behind it (next_trace_stream); a SMALL logged launch starts under it and only its passes wait — for
      // this fold, or with two plane sets for the one that last zeroed theirs (LaunchPlan::under_fold).  The twin's two halves keep the fold and the open session apart)
      int rc = fold_queue(b);  // also: a session that was never ended still owes its plane to the accumulator (old layout)
      if (rc != HALO_OK) return rc;
      const bool caller_reads = b->acc != nullptr && b->acc != b->acc_own.ptr && !b->opt.defer_fold;   // the caller's memory, read in stream order: the fold must be in that order too
      const bool layout_changes = b->mono_s_log2 != s_log2 || b->plane_cnt != plane_cnt_n || b->plane_copies != plane_copies_n || b->mono_two != two_sets_n;   // the twin's halves (and the plane sets) move
      if (caller_reads || layout_changes) {
        rc = join_aux(b);
        if (rc != HALO_OK) return rc;
      }
    }
    int rc = ensure_accumulator(b, render->width, render->height);
    if (rc != HALO_OK) return rc;
  }
  b->xyz_log = xyz_log_n;
  b->mono_by_wl = mono_by_wl_n;
  b->mono_session = mono_session_n;
  b->plane_cnt = plane_cnt_n;
  b->plane_copies = plane_copies_n;
  b->plane_coef = coef_n;
  b->det_session = det;
  if (det) {   // the fixed-point planes, made here with the session's other buffers and all-zero between folds
    const size_t need = (static_cast<size_t>(kMonoRows) << s_log2) * b->plane_cnt;
    b->mono_two = false;
    b->mono_set = 0;
    if (b->fix.cap < need) {
      if (int rc = reserve_idle(b, b->fix, need)) return rc;
      HIPCHK(b, hipMemsetAsync(b->fix.ptr, 0, b->fix.cap * sizeof(unsigned long long), main_q(b)));
    }
    b->mono_s_log2 = s_log2;
  } else {
    const size_t one = (static_cast<size_t>(kMonoRows) << s_log2) * b->plane_copies * b->plane_cnt;
    b->mono_two = two_sets_n;
    b->mono_half = one;
    if (!b->mono_two) b->mono_set = 0;
    const size_t need = one * (b->mono_two ? 2u : 1u);
    if (b->mono.cap < need) {
      if (int rc = reserve_idle(b, b->mono, need)) return rc;
      HIPCHK(b, hipMemsetAsync(b->mono.ptr, 0, b->mono.cap * sizeof(float), main_q(b)));
    }
    b->mono_s_log2 = s_log2;  // planes are all-zero whenever the layout changes (folded above), so it may change freely
    // the twin: one double per float of every plane's copy 0 (2.1 MB x planes at configs[1]'s image; a 64-plane session on 2048x1024 takes
    // 1 GB), kept all-zero between sessions like the planes; sessions whose twin would pass 4 GB go without (their overflow stays on the fp32
    // plane), and so does a session whose twin cannot be allocated
    // (two halves: a session's overflows go to one while the fold of the session before may still be reading the other, `twin_set`)
    const size_t twin_need = (static_cast<size_t>(kMonoRows) << s_log2) * b->plane_cnt;
    if (b->ovf.cap < 2u * twin_need && twin_need <= (512ull << 20)) {
      hipError_t oe = hipSuccess;
      if (int rc = reserve_idle(b, b->ovf, 2u * twin_need, &oe)) return rc;
      bool ok = oe == hipSuccess;
      if (ok && !b->ovf_flag.ptr) ok = b->ovf_flag.reserve(2) == hipSuccess && hipMemsetAsync(b->ovf_flag.ptr, 0, 2 * sizeof(uint32_t), main_q(b)) == hipSuccess;
      if (ok) {
        HIPCHK(b, hipMemsetAsync(b->ovf.ptr, 0, b->ovf.cap * sizeof(double), main_q(b)));
      } else {
        (void)hipGetLastError();   // out of memory is not this session's failure: the launches run without a twin
        b->ovf.release();
        b->ovf_flag.release();
      }
    }
  }
  if (!b->color_classes.empty()) {  // Y lanes persist like the accumulator, until halo_readback_class_lanes
    const size_t need = b->color_classes.size() * npix;
    if (b->lanes.cap < need || b->lanes_w != render->width || b->lanes_h != render->height) {
      if (int rc = reserve_idle(b, b->lanes, need)) return rc;
      if (int rc = join_aux(b)) return rc;
      HIPCHK(b, hipMemsetAsync(b->lanes.ptr, 0, b->lanes.cap * sizeof(double), main_q(b)));
      b->lanes_w = render->width;
      b->lanes_h = render->height;
    }
  }
  b->sess_crystal_samples = b->sess_orient_samples = 0;
  b->route = HaloRouteInfo{};
  b->route_root = 0u;
  b->route.plane_cnt = b->plane_cnt;
  b->route.plane_copies = b->plane_copies;
  b->route.shuffle_chunk = 1u << b->opt.shuffle_chunk_log2;
  b->in_session = true;
  b->layer_idx = 0;
  b->cont_in_n = 0;
  b->cont_out_slot = 0;
  return HALO_OK;
}

int halo_begin(halo_handle_t b, const HaloScene* scene, const HaloRender* render, const HaloWl* wl, uint64_t ray_num) {
  return begin_session(b, scene, render, wl, nullptr, 0, ray_num);
}

int halo_begin_spectrum(halo_handle_t b, const HaloScene* scene, const HaloRender* render, const HaloWl* entries, int32_t count, uint64_t ray_num) {
  if (!b) return HALO_FATAL;
  if (!scene) return fail(b, HALO_FATAL, "halo_begin_spectrum: scene is NULL");
  if (!render) return fail(b, HALO_FATAL, "halo_begin_spectrum: render is NULL");
  if (!entries) return fail(b, HALO_FATAL, "halo_begin_spectrum: entries is NULL");
  if (count < 1 || count > HALO_WL_POOL_MAX) return fail(b, HALO_FATAL, "halo_begin_spectrum: count " + std::to_string(count) + " outside 1..HALO_WL_POOL_MAX (255)");
  for (int32_t k = 0; k < count; k++)
    if (entries[k].illuminant >= 0)
      return fail(b, HALO_FATAL, "halo_begin_spectrum: entries[" + std::to_string(k) + "] is an illuminant (illuminant >= 0); a spectrum is made of discrete wavelengths");
  // one entry: the discrete session of that wavelength, by the same route
  if (count == 1) return begin_session(b, scene, render, entries, nullptr, 0, ray_num);
  return begin_session(b, scene, render, entries, entries, count, ray_num);
}

}  // extern "C"

// The twin half a session of the current layout uses: valid only when the buffer holds two halves of this layout.
static double* twin_of(HaloBackend* b, int set) {
  const size_t half = (static_cast<size_t>(kMonoRows) << b->mono_s_log2) * b->plane_cnt;
  if (!b->ovf.ptr || !b->ovf_flag.ptr || b->ovf.cap < 2u * half) return nullptr;
  return b->ovf.ptr + static_cast<size_t>(set) * half;
}

// Queue the closing fold of the pending planes on the post stream (behind everything both streams hold); the main stream does NOT wait.
static int fold_queue(HaloBackend* b) {
  if (!b->mono_dirty) return HALO_OK;
  // a shard's own integer planes are a part of the image: they leave through halo_export_fixed, never through a fold
  if (b->fix_planes && b->shard_count > 1 && !b->fix_imported)
    return fail(b, HALO_FATAL, "shard " + std::to_string(b->shard_index) + " of " + std::to_string(b->shard_count) +
                                   ": the pending fixed-point planes hold a part of the image; move them out with halo_export_fixed (and fold what halo_import_fixed brings in)");
  HIPCHK(b, hipSetDevice(b->device));
  HIPCHK(b, b->ord.fork_aux());
  hipStream_t ps = b->ord.post_stream();
  const uint32_t npix = static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h);
  if (b->fix_planes) {   // a deterministic session's planes: integers in, float32(double(S) * 2^-F) out, then the same chain (no copies, no twin)
    FoldCoef coef{};
    for (uint32_t m = 0; m < b->plane_cnt; m++)
      for (int a = 0; a < 3; a++) coef.c[m][a] = b->plane_coef[m][static_cast<size_t>(a)];
    hipError_t e = launch_fold_fixed(b->acc, b->fix.ptr, npix, b->mono_s_log2, b->plane_cnt, coef, b->fix_frac, ps);
    if (e != hipSuccess) return hip_fail(b, e, "halo_fold_fixed_kernel launch");
    b->fix_hits = 0;
    b->fix_planes = false;
    b->fix_imported = false;
    b->mono_dirty = false;
    return HALO_OK;
  }
  const size_t plane = (static_cast<size_t>(kMonoRows) << b->mono_s_log2) * b->plane_copies;
  const size_t twin_plane = static_cast<size_t>(kMonoRows) << b->mono_s_log2;
  double* twin = twin_of(b, b->twin_set);
  uint32_t* flag = twin ? b->ovf_flag.ptr + b->twin_set : nullptr;
  for (uint32_t first = 0; first < b->plane_cnt; first += kFoldGroup) {
    const uint32_t n = std::min<uint32_t>(kFoldGroup, b->plane_cnt - first);
    FoldCoef coef{};
    for (uint32_t m = 0; m < n; m++)
      for (int a = 0; a < 3; a++) coef.c[m][a] = b->plane_coef[first + m][static_cast<size_t>(a)];
    hipError_t e = launch_fold(b->acc, planes_of(b) + first * plane, npix, b->mono_s_log2, b->plane_copies, n, coef, twin ? twin + first * twin_plane : nullptr, flag, ps);
    if (e != hipSuccess) return hip_fail(b, e, "halo_fold_kernel launch");
  }
  if (flag) HIPCHK(b, hipMemsetAsync(flag, 0, sizeof(uint32_t), ps));   // every group has seen it; the fold zeroed what it took
  b->twin_set ^= 1;   // what traces from here on overflows into the other half
  if (b->mono_two) {    // ... and adds to the other plane set, once the fold that last zeroed THAT one is through (set_folded)
    HIPCHK(b, b->ord.set_folded[b->mono_set].mark(ps));
    b->mono_set ^= 1;
  }
  b->mono_dirty = false;
  return HALO_OK;
}
// ... and with the main stream waiting for it: for readers of the image and for whoever hands the image to somebody else.
int halo::fold_if_dirty(HaloBackend* b) {
  if (int rc = fold_queue(b)) return rc;
  return join_aux(b);
}

extern "C" {

int halo_end(halo_handle_t b) {
  if (!b) return HALO_FATAL;
  // a session closes by folding its planes into the XYZ image (a discrete wavelength's CMF applied to the scalar plane) — at once when the image
  // is the caller's memory (halo_bind_accumulator: the caller reads it without asking), otherwise when somebody reads it (every reader folds
  // first) or a session with other planes begins
  int rc = HALO_OK;
  const bool own = b->acc != nullptr && b->acc == b->acc_own.ptr;
  if (!((b->opt.lazy_fold && own) || (b->opt.defer_fold && !own))) rc = fold_if_dirty(b);
  b->in_session = false;
  return rc;
}

// the canonical order's error word (kContErr*) as a session failure
static int cont_order_fail(HaloBackend* b, uint32_t err) {
  return fail(b, HALO_FATAL, (err & kContErrSum) ? "cont_order = 1: the roots' masks do not add up to the continuation pool (an exit seq continued twice, or a record lost)"
                                                 : "cont_order = 1: a continuation record's key lies outside its layer or pool");
}
}  // extern "C"

// ---- The steps of halo_trace_layer: plan (no HIP call) -> entry tables -> parameters -> route buffers -> launch + passes -> route record -> close ----
namespace {


// What the launches of one halo_trace_layer call share.
struct LayerCtx {
  int layer = 0, out_slot = 0;
  uint32_t source = kSrcGen, out_cap = 0;
  uint64_t n = 0;
  uint64_t traced = 0;   // the roots this handle launched: n, or its slices of them (halo_set_shard)
  const HaloHostRays* rays = nullptr;
  // host_crystal — HostRayBatch::crystal (trace_backend.hpp:230-239): injected rays may bring the crystal they were sampled on; it is traced as it
  // is — one shape for the whole batch, no draw from the shape stream, no stochastic sample counted (test_cpu_trace_backend.cpp:737-777)
  bool final_layer = false, canon_check = false, host_crystal = false;
};
// Everything that is DECIDED about one launch before any HIP call is made: plan_launch fills the chunking part for the whole layer up front (the
// continuation pool is sized from the same plans the launch loop walks), plan_route the accumulation route once the entry's kernel mode is known.
struct LaunchPlan {
  int ci = 0;
  uint64_t m = 0, off = 0, first = 0;   // rays; offset within the entry's share; index of the first ray within the layer
  uint64_t share = 0;                   // the entry's whole share of the layer's rays (off + left when the launch was planned)
  bool deterministic = false, host_pool = false, alternate = false;
  int geom = 0, blocks = 0;             // geom: 0 = one shape per dispatch, 1 = pool of ShapeDev records, 2 = pool of ShapePrism records (device-generated prisms)
  uint32_t shape_cnt = 1;
  bool use_bin = false, two_level = false, use_log = false, use_log_xyz = false, canon = false, no_land = false;
  bool only = false;                    // the layer's only launch, on the session's last layer (halo_trace_layer)
  bool close = false;                   // ... that closes its session in its per-tile pass (close_direct_ok): nothing is left in the planes
  bool tile = false;                    // ... and whose trace kernel appends per tile (bind_tile_append): the closing pass reads chunks, no split pass
  bool ticket = false;                  // ... in its ticketed form: `blocks` is then one resident round at the most (bind_tile_append)
  bool fixed = false;                   // a deterministic session's launch: the kAccFixed kernels, with use_log their logging twins (or, where every exit continues, kAccNone)
  uint32_t fan_log2 = 0, lists1 = 0, bin_tiles = 0, log_t_log2 = 0, log_planes = 1, log_tiles = 0;
  uint64_t cap1 = 0, cap2 = 0;          // records per region / coarse list and per tile list, as REQUESTED: reserve_log_buffers clamps the log's against free memory
  // (Round 6: a LOGGED trace kernel writes records, its region counts and the twin's other half — nothing the closing fold of the session
  //  before reads or zeroes — so on a SMALL launch it starts under that fold, and only its passes, which add to the planes, wait for it.  A
  //  discrete spectrum of many short sessions (bench.py --config 4d: 31 x 0.8 M rays) was one serial chain of generator, trace, split, sums
  //  and fold, 325 us per session; the trace kernel and generator of session k + 1 now run beside the passes and the fold of session k.
  //  Launches that fill the chip keep the old order: measured in round 5, nothing to gain there and the kernel's own span stretches.)
  // (A deterministic logged launch flushes its integer cache onto the planes from the trace kernel itself: it waits for the fold, as a direct one does.)
  // (A directly closing launch writes the image and the twin's half in its passes: it is queued behind the auxiliary stream like a launch that fills the chip.)
  bool under_fold() const { return use_log && alternate && !fixed && !close; }
  bool sums_plain() const { return (use_log && !fixed) || (use_bin && two_level); }   // the per-tile sums end in plain read-modify-writes of the planes (Order: plane ownership)
};
// What a launch was given when it was queued: its dispatch-ring slot, log buffer set, shape pool and the first index of its shape stream.
struct LaunchSlots { int k = 0, ls = 0, shape_set = 0; uint64_t first_shape = 0; };
// The dispatch-constant tables of one crystal entry (prepare_entry_tables) and where a launch finds them (upload_tables).
struct EntryTables {
  int mode = 0;
  bool fast_mode = true;    // production-shaped kernels: exit queue, hit log, regular-prism search
  bool use_filter = false, use_color = false, cached = false;
  bool entry_fast = false, hex_regular = false, has_fast = false;   // what the slot the launch reads holds
  FilterDev fd{};
  ColorDev cd{};
  FastTables* fast_host = nullptr;
  HaloBackend::TableCacheEntry* ce = nullptr;
  DispatchSlot* ce_dev = nullptr;   // the entry's two slots
};
// launch plan: chunking bounds the host-built shape pool for stochastic geometry and keeps n_rays < 2^32
uint64_t chunk_of(const HaloBackend& b, uint64_t left, const HaloCrystal& crystal, bool host_crystal) {
  uint64_t m = std::min<uint64_t>(left, b.opt.chunk);
  if (b.det_session) m = std::min<uint64_t>(m, kFixBudgetHits);   // a launch fits the budget of one fixed-point plane set
  // stochastic geometry: one pool record per geom_clock rays.  Device-generated prisms are 1360 B records (2.9 GB per
  // 64 Mi rays), other device-generated shapes 4.1 KB (2 GB per 16 Mi rays); host-built pools (pageable staging + H2D)
  // stay at 4 Mi rays
  if (!host::IsDeterministic(crystal) && !host_crystal) {
    const uint64_t dev = b.opt.stoch_chunk ? b.opt.stoch_chunk : (1ull << 26);   // records: 2.9 GB (prism) / 8.6 GB (general) per 64 Mi rays
    m = std::min<uint64_t>(m, b.opt.host_shapes ? (1ull << 22) : dev);
  }
  return m;
}
int blocks_of(const HaloBackend& b, uint64_t m, bool pool) {
  // per-workgroup fixed costs (table staging, pixel-cache zero + flush) are paid per launch, a long tail is paid per
  // round of resident workgroups: aim at >= 32 passes of the ray loop per workgroup, between 4 and blocks_per_cu per CU
  // (measured: 1 M rays 0.27 -> 0.20 ms at 4/CU; 50 M rays 4.02 -> 3.67 ms at 24/CU instead of 8/CU)
  // (Measured again on the per-tile-append kernel, six resident workgroups per CU, where every workgroup also leaves a chunk and a count per tile
  //  for the closing pass: the trace kernel of configs[1] at 6 / 8 / 12 / 16 / 24 / 32 / 48 per CU 1.74 / 1.71 / 1.60 / 1.55 / 1.53 / 1.51 / 1.51 ms
  //  (32 and 48 are capped by `want` like 24) — ONE round of resident workgroups ends with its slowest, 0.2 ms behind several rounds that even the
  //  tail out — and that is four times what the closing pass gains from the longer chunks of the smaller grid (0.20 -> 0.14 ms at 6 per CU, 0.16
  //  at 12): 24 stays, for the static loop of these launches too.  profiles/resident_grid_ab.txt.  With wave tickets — option tile_ticket,
  //  bind_tile_append — such a launch runs ONE resident round whose waves draw their passes from counters: the round's tail is one short ticket
  //  long: five rounds against the parent, medians, trace kernel 1.513 -> 1.484 ms AND closing pass 0.179 -> 0.150.  profiles/wave_tickets_ab.txt.)
  // Small launches — a Lumice server that keeps a GPU route's small dispatch (2^15 .. 2^18 rays per session, server.cpp:140-151) sends nothing
  // else — are latency: one pass of the ray loop is ~11 us on a wave that has its SIMD to itself, so they spread over as many workgroups as
  // a CU holds (five) before a workgroup takes a second pass.  (Round 4 had found the opposite — one per CU best — while every WAVE ended
  // with four same-line fp64 atomics; with those gone, tools/dispatch_probe.cpp, us per session at 1 / 2 / 3 / 4 / 5 / 8 per CU:
  // 2^18 rays 67 / 50 / 45 / 44 / 43 / 44, 2^20 188 / 133 / 122 / 115 / 110 / 111, 2^22 326 / 326 / 276 / 261 / 250 / 259.)
  const uint64_t want = m / (static_cast<uint64_t>(kBlock) * 32u);
  // (shape-pool kernels hold four workgroups a CU, not six, and every workgroup of a logged launch is a region for the split pass: three per CU
  //  there — bench.py --config 4d, 0.8 M rays per session, ms per step at 1 / 2 / 3 / 4 / 5 / 6 / 8 per CU: 7.26 / 5.99 / 5.73 / 5.77 / 5.86 / 6.14 / 6.39)
  const int small_k = b.opt.small_blocks_per_cu > 0 ? b.opt.small_blocks_per_cu : pool ? 3 : 5;
  const uint64_t lo_cap = static_cast<uint64_t>(b.cu_count) * static_cast<uint64_t>(std::min(b.opt.blocks_per_cu, small_k));
  const uint64_t cap = std::min<uint64_t>(static_cast<uint64_t>(b.cu_count * b.opt.blocks_per_cu), std::max<uint64_t>(lo_cap, want));
  uint64_t nb = std::min<uint64_t>((m + kBlock - 1) / kBlock, cap);
  if (b.opt.blocks_cap > 0) nb = std::min<uint64_t>(nb, static_cast<uint64_t>(b.opt.blocks_cap));
  return static_cast<int>(nb);
}
// The chunking part of a launch's plan: the next launch of entry `ci`, `left` of whose rays are still to be traced (`first_ci` = the entry's first ray).
LaunchPlan plan_launch(const HaloBackend& b, const LayerCtx& c, int ci, uint64_t first_ci, uint64_t off, uint64_t left) {
  const HaloCrystal& crystal = b.scene.layers[c.layer].entries[ci].crystal;
  LaunchPlan p;
  p.ci = ci, p.off = off, p.first = first_ci + off, p.share = off + left;
  p.m = chunk_of(b, left, crystal, c.host_crystal);
  p.deterministic = c.host_crystal || host::IsDeterministic(crystal);
  p.shape_cnt = p.deterministic ? 1u : static_cast<uint32_t>((p.m + b.opt.geom_clock - 1) / b.opt.geom_clock);
  p.host_pool = !p.deterministic && b.opt.host_shapes;
  p.geom = p.deterministic ? 0 : ((crystal.kind == HALO_CRYSTAL_PRISM && !p.host_pool) ? 2 : 1);
  p.blocks = blocks_of(b, p.m, !p.deterministic);
  // Launches of <= 2^21 rays alternate between the two trace streams (next_trace_stream); only those can meet a neighbour that still reads
  // or writes a buffer set, so only those take the sets in turn — a launch that fills the chip keeps stream 0 and set 0 (a second set
  // allocated in the middle of a run is a host sync and a multi-gigabyte hipMalloc: 1.2 s in configs[4]'s first timed step)
  p.alternate = p.m <= (1ull << b.opt.alt_log2);
  return p;
}
// The accumulation route of a planned launch (direct / binned one- or two-level / hit log scalar / hit log X/Y/Z / none) and the buffer sizes it asks for.
void plan_route(const HaloBackend& b, const LayerCtx& c, bool fast_mode, LaunchPlan& p) {
  const HaloLayer& L = b.scene.layers[c.layer];
  const uint64_t m = p.m, blocks = static_cast<uint64_t>(p.blocks);
  const uint32_t s_log2 = b.mono_s_log2;
  const bool full_sky = b.render.visible == HALO_VISIBLE_FULL;
  // binned accumulation for big one-plane launches (see halo_trace.inl: HitBuffer)
  // 16384-slot tiles over the session's planes taken as one array (1 plane, or the per-entry planes of a small image)
  const uint64_t bin_slots = (static_cast<uint64_t>(kMonoRows) << s_log2) * (b.mono_by_wl ? b.plane_cnt : 1u);
  p.bin_tiles = static_cast<uint32_t>(bin_slots >> 14);
  const bool bin_geom_ok = p.deterministic || L.entries[p.ci].crystal.kind == HALO_CRYSTAL_PRISM;
  // up to 512 tiles: one level (interleaved tiles).  More (per-wavelength planes of a large image): two levels — the
  // trace kernel fills coarse lists of `fan` consecutive tiles each, a split pass deals them out to the tiles.
  p.fan_log2 = 0u;
  while (((p.bin_tiles + (1u << p.fan_log2) - 1u) >> p.fan_log2) > b.opt.bin_l1) p.fan_log2++;
  p.two_level = p.bin_tiles > 512u;
  const bool bin_shape_ok = p.two_level ? (p.fan_log2 <= 8u && (bin_slots & 16383ull) == 0ull)
                                        : (p.bin_tiles >= 8u && (p.bin_tiles & (p.bin_tiles - 1u)) == 0u);
  // The hit log over the scalar planes of a per-entry-plane session (small images: the reference's 512x256 D65 scenes): every plane gets
  // 2^t interleaved tiles of <= 16 Ki slots, and the split pass feeds at most 512 lists — 64 planes up to 128 Ki pixels, 32 up to 256 Ki.
  const uint32_t wl_t_log2 = s_log2 >= 4u ? s_log2 - 4u : 0u;
  const bool log_planes_ok = b.mono_by_wl && (static_cast<uint64_t>(b.plane_cnt) << wl_t_log2) <= 512ull &&
                             (static_cast<uint64_t>(b.plane_cnt) << (s_log2 + 10u)) <= (1ull << 31) && b.opt.hit_log != 0 && b.opt.bin <= 0;
  // (a layer before the last under canonical continuation order takes direct accumulation: only those kernels have CANON twins)
  p.canon = b.opt.cont_order && !c.final_layer;
  p.fixed = b.det_session;   // every accumulating launch of a deterministic session adds integers: directly, or through the hit log's integer twins — never lists
  const bool fixed_xyz = p.fixed && !b.mono_session;   // ... on X, Y, Z planes (a deterministic session has no plane per pool entry)
  p.use_bin = !p.fixed && !p.canon && b.mono_session && b.opt.aggregate == 1 && !b.opt.capture && bin_shape_ok && bin_slots <= (1ull << 31) &&
              // own choice: only where the hit log cannot go (one plane per pool entry on a larger image) — the log beats the binned route
              // on every launch measured (tools/bin_vs_log_probe.py: dual fisheye 50 M rays 5.13 -> 4.42 ms)
              (b.opt.bin < 0 ? (b.mono_by_wl && !log_planes_ok && bin_geom_ok && full_sky && m >= (2ull << 20)) : b.opt.bin != 0);
  p.lists1 = p.two_level ? ((p.bin_tiles + (1u << p.fan_log2) - 1u) >> p.fan_log2) : p.bin_tiles;
  // Hit log (halo_trace.inl log_hit): global fp32 atomics retire memory-side at 21 G/s on this part, which bounded every big
  // launch once its trace was fast enough (configs[1]: 2.4 ms of trace, 2.8 ms of atomics).  A production-mode launch on one
  // scalar plane, or on the X/Y/Z planes of an illuminant session, appends its cache misses to one log region per workgroup
  // instead; a split pass and a per-tile pass add them to the plane(s) afterwards.
  // Tiles: as many as the split pass feeds whatever the image size — the per-tile pass has one workgroup per tile — of at least
  // 256 and at most 16 Ki slots (X/Y/Z: 4 Ki) of ONE plane: 512 for X/Y/Z; for a scalar plane 128 where that keeps them within
  // 16 Ki slots (longer runs in the split pass: 0.23 vs 0.25 ms at configs[1]).
  // (a small launch takes 256 tiles: its per-tile pass is one workgroup per tile, and 128 of them leave half the chip idle — config 4d 2.85 -> 3.18 G rays/s; big launches keep 128 for the split's longer runs)
  const uint32_t asked_t_log2 = static_cast<uint32_t>(m < (4ull << 20) ? std::max(b.opt.log_tiles_log2, 8) : b.opt.log_tiles_log2);
  const uint32_t scalar_t_log2 = std::max<uint32_t>(wl_t_log2, std::min<uint32_t>(asked_t_log2, s_log2 + 2u));   // tiles of 256 .. 16 Ki slots
  p.log_t_log2 = log_planes_ok ? wl_t_log2 : (b.xyz_log || fixed_xyz) ? std::min<uint32_t>(9u, s_log2 + 2u) : scalar_t_log2;
  p.log_planes = log_planes_ok ? b.plane_cnt : 1u;
  p.log_tiles = p.log_planes << p.log_t_log2;   // lists the split pass feeds
  const bool log_layout_ok = (b.xyz_log || fixed_xyz) ? (s_log2 <= 11u) : (b.mono_session && (log_planes_ok || (!b.mono_by_wl && s_log2 <= 12u)));
  // (aggregate = 0 under a forced log — every hit a record — exists in deterministic sessions only, where the cache is a run-time branch of accumulate_fixed)
  const bool log_agg_ok = b.opt.aggregate == 1 || (p.fixed && b.opt.aggregate == 0 && b.opt.hit_log > 0);
  p.use_log = !p.canon && !p.use_bin && log_layout_ok && log_agg_ok && fast_mode &&
              (L.prob < 1.0f || c.final_layer) &&   // a layer whose every exit continues puts nothing on the image
              // (own choice in a deterministic session: from 2 Mi rays on either plane layout and whatever the visible range — the float route's
              //  512 Ki for full-sky scalar sessions buys nothing there: the integer log neither starts under the previous fold nor has two plane
              //  sets, and bench.py --config 4d measured 10.96 ms per step logged against 10.79 direct)
              (b.opt.hit_log < 0 ? m >= (p.fixed ? (2ull << 20) : (b.mono_session && !b.mono_by_wl) ? log_min_rays(b.render.visible) : (2ull << 20)) : b.opt.hit_log != 0);
  p.use_log_xyz = p.use_log && (b.xyz_log || fixed_xyz);
  p.no_land = L.prob >= 1.0f && !c.final_layer && fast_mode && b.opt.aggregate == 1;
  if (p.use_log) {
    // a region takes 4 records per ray of its workgroup (configs[1]: 1.2 logged per ray), 8 for full-sky renders (5-6 per ray),
    // and a tile list twice its even share of that; what runs over falls back to direct atomics
    const uint64_t per_wg = (m + blocks - 1u) / blocks;
    p.cap1 = std::min<uint64_t>(std::max<uint64_t>(4ull * per_wg, 4096ull), (6ull << 30) / (8ull * blocks));
    if (p.use_log_xyz || full_sky) p.cap1 = std::min<uint64_t>(std::max<uint64_t>(8ull * per_wg, 4096ull), (8ull << 30) / (8ull * blocks));
    // (per-launch cost of the slack, measured: configs[1] split 234 / 238 / 241 us at 2x / 4x / 8x; configs[4]'s 512 X/Y/Z lists 554 / 574 / 635 us —
    // so 8x for scalar planes, where a hot pixel meets near-constant addends, 4x for X/Y/Z, whose addends vary with the wavelength)
    const uint64_t kListSlack = p.use_log_xyz ? 4ull : 8ull;
    // (8x the even share, within the 8 GB below: what runs over a tile list is added with fp32 atomics, and on a pixel that holds 4e5 the
    // rounding of a near-constant addend is a bias, not noise — tools/route_fuzz.py seed 969: the sun's tile of a 1024 x 512 render took five
    // even shares and its pixel read 5.6e-4 high with 2x)
    p.cap2 = std::max<uint64_t>(kListSlack * ((p.use_log_xyz || full_sky) ? 8ull : 4ull) * m / p.log_tiles, 1ull << 14);
    p.cap2 = std::min<uint64_t>(p.cap2, (8ull << 30) / (8ull * p.log_tiles));
    if (b.opt.hit_log_cap) {   // tests: run both overflow fallbacks
      p.cap1 = b.opt.hit_log_cap;
      p.cap2 = std::max<uint64_t>(p.cap1 * blocks / (2ull * p.log_tiles), 64ull);
    }
  } else if (p.use_bin) {
    // lists sized for ~6 hits per ray spread 4x unevenly; an overflowing list falls back to direct atomics
    // (the coarse and tile lists of the two-level route are slot ranges interleaved over the image — rows p % 1024 — and
    // stay balanced whatever the image shows: 2x there)
    const uint64_t slack = p.two_level ? 2ull : 4ull;
    p.cap1 = std::min<uint64_t>(std::max<uint64_t>(slack * 6ull * m / p.lists1, 1ull << 16), (8ull << 30) / (8ull * p.lists1));
    if (p.two_level) p.cap2 = std::min<uint64_t>(std::max<uint64_t>(slack * 6ull * m / p.bin_tiles, 1ull << 12), (8ull << 30) / (8ull * p.bin_tiles));
  }
}
// The second stage of a logged launch's plan, the one that asks the device: the caps give way to free memory and both log sets are reserved.
// p.cap1 / p.cap2 leave as what the buffers hold; a reserve that fails takes the launch off the log (p.use_log).
int reserve_log_buffers(HaloBackend* b, LaunchPlan& p, int ls) {
  const uint64_t blocks = static_cast<uint64_t>(p.blocks);
  // The log's capacity is a speed matter only (what runs over is added directly), so it gives way to the memory there is: the
  // regions and lists still to be allocated take at most half of what is free (the continuation and shape pools of later layers
  // want theirs), and a reserve that fails all the same sends this launch down the direct route instead of failing the trace.
  size_t free_b = 0, total_b = 0;
  const uint64_t have = (b->bin_list_s[ls].cap + b->bin_list2_s[ls].cap) * sizeof(HitRec);
  const uint64_t need = (p.cap1 * blocks + p.cap2 * p.log_tiles) * sizeof(HitRec);
  if (need > have && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need - have > free_b / 2u) {
    const double shrink = static_cast<double>(have + free_b / 2u) / static_cast<double>(need);
    p.cap1 = std::max<uint64_t>(static_cast<uint64_t>(static_cast<double>(p.cap1) * shrink), 1024ull);
    p.cap2 = std::max<uint64_t>(static_cast<uint64_t>(static_cast<double>(p.cap2) * shrink), 1024ull);
  }
  hipError_t e1 = hipSuccess, e2 = hipSuccess;
  if (int rc = reserve_idle(b, b->bin_list_s[ls], p.cap1 * blocks, &e1)) return rc;
  if (e1 == hipSuccess)
    if (int rc = reserve_idle(b, b->bin_list2_s[ls], p.cap2 * p.log_tiles, &e2)) return rc;
  if (b->opt.overlap && p.alternate && e1 == hipSuccess && e2 == hipSuccess) {
    // the other set with it: the next launch would otherwise stop the queue (a host sync and a multi-gigabyte hipMalloc) for it.  A speed
    // matter only — if there is no room, the launch that finds the set short shrinks its log as above.
    hipError_t e3 = hipSuccess, e4 = hipSuccess;
    if (int rc = reserve_idle(b, b->bin_list_s[ls ^ 1], p.cap1 * blocks, &e3)) return rc;
    if (e3 == hipSuccess)
      if (int rc = reserve_idle(b, b->bin_list2_s[ls ^ 1], p.cap2 * p.log_tiles, &e4)) return rc;
    if (e3 != hipSuccess || e4 != hipSuccess) (void)hipGetLastError();
  }
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipGetLastError();   // out of memory: not this launch's route
    p.use_log = p.use_log_xyz = false;
  }
  return HALO_OK;
}
// The filter / colour / fast tables of entry `ci`, the kernel mode they ask for, and the entry's table-cache slot if it has one.
void prepare_entry_tables(HaloBackend* b, const LayerCtx& c, int ci, EntryTables& T) {
  const HaloEntry& E = b->scene.layers[c.layer].entries[ci];
  const bool deterministic = c.host_crystal || host::IsDeterministic(E.crystal);
  T = EntryTables{};
  // the entry's tables may still be on the device from an earlier dispatch (table cache, see HaloBackend::TableCacheEntry)
  T.ce = (b->opt.table_cache && deterministic && !c.host_crystal && c.source != kSrcTransit) ? &b->tcache[c.layer][ci] : nullptr;
  if (T.ce && !b->tcache_dev.ptr) {
    if (b->tcache_dev.reserve(static_cast<size_t>(HALO_MAX_LAYERS) * HALO_MAX_ENTRIES * 2u) != hipSuccess) {
      (void)hipGetLastError();
      T.ce = nullptr;   // no room for the cache: every dispatch uploads its tables
    }
  }
  T.ce_dev = T.ce ? b->tcache_dev.ptr + (static_cast<size_t>(c.layer) * HALO_MAX_ENTRIES + static_cast<size_t>(ci)) * 2u : nullptr;
  T.cached = T.ce && T.ce->valid;
  if (T.cached) T.use_filter = T.ce->use_filter;
  else if (E.filter_id > 0) {
    T.fd = host::BuildFilter(b->filters[static_cast<size_t>(E.filter_id - 1)], E.axis);
    T.use_filter = T.fd.is_complex || T.fd.terms[0].type != HALO_FILTER_NONE || T.fd.action != 0;
  }

  // raypath colour: this entry's predicates (canonicalised like filter terms, each with its own symmetry) + the classes
  ColorDev& cd = T.cd;
  T.use_color = !b->color_classes.empty();
  if (T.use_color && !T.cached) {
    cd.class_cnt = static_cast<uint32_t>(b->color_classes.size());
    for (uint32_t k = 0; k < cd.class_cnt; k++) {
      cd.class_bits[k] = b->color_classes[k].bits;
      cd.class_all[k] = b->color_classes[k].combine_all ? 1 : 0;
    }
    if (E.color_id > 0) {
      const HaloColorSet& cs = b->color_sets[static_cast<size_t>(E.color_id - 1)];
      cd.term_cnt = static_cast<uint32_t>(std::min(cs.term_count, HALO_COLOR_MAX_TERMS));
      for (uint32_t k = 0; k < cd.term_cnt; k++) {
        HaloFilter one{};
        one.symmetry = cs.terms[k].symmetry;
        one.terms[0] = cs.terms[k].predicate;
        const FilterDev f1 = host::BuildFilter(one, E.axis);
        cd.terms[k].t = f1.terms[0];
        cd.terms[k].symmetry = f1.symmetry;
        cd.terms[k].d_applicable = f1.d_applicable;
        cd.terms[k].sigma_a = f1.sigma_a;
        cd.terms[k].bit = static_cast<uint8_t>(cs.terms[k].bit & 0xFF);
      }
    }
  }

  // Which kernels: capture (tests) > filter / colour in their fast form (paths <= 16 faces, tables fit) > the generic filter kernels > plain
  if (T.cached) T.mode = T.ce->mode;
  else if (b->opt.capture) T.mode = 2;
  else if (b->opt.rehit_strategy == 0) T.mode = 3;   // the legacy next-face strategy lives in the generic kernels only
  else if (T.use_filter || T.use_color) {
    T.mode = 3;
    if (b->opt.filter_fast && b->scene.max_hits <= 16) {
      b->fast_scratch.reset(new FastTables());
      std::memset(b->fast_scratch.get(), 0, sizeof(FastTables));
      const HaloColorSet* cs = (T.use_color && E.color_id > 0) ? &b->color_sets[static_cast<size_t>(E.color_id - 1)] : nullptr;
      if (host::BuildFastTables(T.use_filter ? &b->filters[static_cast<size_t>(E.filter_id - 1)] : nullptr, cs, E.axis, static_cast<uint32_t>(E.crystal_config_id), *b->fast_scratch)) {
        T.fast_host = b->fast_scratch.get();
        T.fast_host->class_cnt = T.use_color ? cd.class_cnt : 0u;
        for (uint32_t k = 0; k < T.fast_host->class_cnt; k++) {
          T.fast_host->class_bits[k] = cd.class_bits[k];
          T.fast_host->class_all[k] = cd.class_all[k];
        }
        T.mode = T.use_color ? 4 : 1;
      }
    }
  }
  T.fast_mode = T.mode == 0 || T.mode == 1 || T.mode == 4;
  T.has_fast = T.cached ? T.ce->has_fast : T.fast_host != nullptr;
  if (T.cached) T.entry_fast = T.ce->entry_fast, T.hex_regular = T.ce->hex_regular;
}
// The dispatch slot a launch reads its tables from: the entry's cache slot if it is valid, else tables + zeroed tallies go up in one copy from
// ring slot k's pinned mirror (`shape`: the one shape of a deterministic entry).
int upload_tables(HaloBackend* b, const LayerCtx& c, const LaunchPlan& p, const HaloEntry& E, uint32_t lat_path, const ShapeDev* shape, int k, EntryTables& T,
                  DispatchSlot** out) {
  HaloBackend::TableCacheEntry* ce = T.ce;
  DispatchSlot& hs = b->slots_host.ptr[k];
  if (ce && !T.cached) ce->cur ^= 1;   // an upload takes the entry's other slot
  DispatchSlot* ds = *out = ce ? T.ce_dev + ce->cur : b->slots_dev.ptr + k;
  if (T.cached) return HALO_OK;   // (T describes the slot already: from the cache entry, or from this entry's previous upload)
  if (lat_path == kLatLut) {
    const host::LatLut& lut = cached_lut(b, E.axis.latitude);
    std::copy(lut.theta.begin(), lut.theta.end(), hs.lut);
    std::copy(lut.cdf.begin(), lut.cdf.end(), hs.lut + kLutNodes);
    std::copy(lut.flip.begin(), lut.flip.end(), hs.lut + 2 * kLutNodes);
  }
  std::copy(b->wl_pool_host.begin(), b->wl_pool_host.end(), hs.wl);
  if (p.deterministic) {
    hs.shape = *shape;
    T.entry_fast = b->opt.entry_fast && host::BuildEntryFast(*shape, hs.efast);
    T.hex_regular = T.entry_fast && hs.efast.hex_regular;
  }
  if (T.use_filter) hs.filter = T.fd;
  if (T.use_color) hs.color = T.cd;
  if (T.fast_host) std::memcpy(&hs.fast, T.fast_host, sizeof(FastTables));
  if (c.source == kSrcTransit) std::copy(b->cont_seg, b->cont_seg + kContShards + 1, hs.seg);
  // (the fast filter tables are the slot's last member and travel only with the dispatches that use them; the pinned mirror is this
  // ring slot's, so it stays as it is until the copy has run — harvest_slot in trace_launch)
  // A cache slot is a fixed device address: a kernel of an earlier, queued session (async: nobody harvested it) may still be staging its
  // tables out of it on a trace stream.  The upload goes behind the last launch that read this slot (no host wait; ring slots are
  // protected by harvest_slot).  Without this the earlier kernel's late workgroups could pick up THIS session's wavelength pool or
  // shape (tests/test_gpu_production_routes.py::test_async_sessions_alternating_wavelengths).
  if (ce && ce->read_ring[ce->cur] >= 0) HIPCHK(b, b->ord.behind_reader(ce->read_ring[ce->cur], ce->read_use[ce->cur]));
  HIPCHK(b, hipMemcpyAsync(ds, &hs, T.fast_host ? sizeof(DispatchSlot) : offsetof(DispatchSlot, fast), hipMemcpyHostToDevice, main_q(b)));
  if (ce) {   // the next dispatch of this entry — the layer's next chunk, the next equal session — finds the tables in place
    ce->valid = true, ce->mode = T.mode, ce->use_filter = T.use_filter, ce->use_color = T.use_color;
    ce->entry_fast = T.entry_fast, ce->hex_regular = T.hex_regular, ce->has_fast = T.has_fast;
    T.cached = true;
  }
  return HALO_OK;
}
// The root profile a dispatch record matches exactly (halo_trace.inl kRoot*: LUT latitude, uniform azimuth and roll, generated roots or the
// continuation pool); anything else keeps the generic root generation.  Whether an instantiation with that profile exists for the launch's
// kernel is the selector's business (halo_select.h with_root).
uint32_t root_profile_of(const DispatchParams& P) {
  if (P.lat_path != kLatLut || P.az_type != HALO_DIST_UNIFORM || P.roll_type != HALO_DIST_UNIFORM) return kRootProfileNone;
  return P.source == kSrcGen ? kRootProfileGen : P.source == kSrcTransit ? kRootProfileTransit : kRootProfileNone;
}
// The fields of DispatchParams that every launch of entry `ci` shares.  The accumulation route's (bin_*, log_*, mono_copy_mask, mono_by_wl,
// no_land) are written by bind_route alone, the tables', shapes' and counters' by trace_launch.
DispatchParams fill_params(HaloBackend* b, const LayerCtx& c, int ci) {
  const HaloLayer& L = b->scene.layers[c.layer];
  const HaloEntry& E = L.entries[ci];
  DispatchParams P{};
  P.source = c.source;
  P.layer = static_cast<uint32_t>(c.layer);
  P.final_layer = c.final_layer ? 1u : 0u;
  P.max_hits = static_cast<uint32_t>(b->scene.max_hits);
  P.prob = L.prob;
  P.crystal_id = static_cast<uint32_t>(E.crystal_config_id);
  P.capture = static_cast<uint32_t>(b->opt.capture);
  P.gen_seed = b->seed ^ kNonceGen;
  P.gate_seed = b->seed ^ kNonceGate;
  P.transit_seed = b->seed ^ kNonceTransit;
  P.shuffle = static_cast<uint32_t>(b->cont_shuffle);
  P.shuffle_seed = (b->seed ^ kNonceShuffle) ^ static_cast<uint32_t>(c.layer);  // cuda_trace_backend.cu:4541
  P.shuffle_chunk_log2 = b->opt.shuffle_chunk_log2;
  // orientation wire params (BuildTransitGpParams cuda_trace_backend.cu:342-383)
  P.lat_path = host::SelectLatPath(E.axis);
  P.lat_mean_rad = E.axis.latitude.center * host::kDegToRad;
  P.lat_std_rad = E.axis.latitude.spread * host::kDegToRad;
  P.az_type = static_cast<uint32_t>(E.axis.azimuth.type);
  P.az_mean_rad = E.axis.azimuth.center * host::kDegToRad;
  P.az_std_rad = E.axis.azimuth.spread * host::kDegToRad;
  P.roll_type = static_cast<uint32_t>(E.axis.roll.type);
  P.roll_mean_rad = E.axis.roll.center * host::kDegToRad;
  P.roll_std_rad = E.axis.roll.spread * host::kDegToRad;
  // BuildGenGpParams cuda_trace_backend.cu:391-399, trig evaluated once on the host
  const float sun_lon = (b->scene.sun_azimuth + 180.0f) * host::kDegToRad;
  const float sun_lat = -b->scene.sun_altitude * host::kDegToRad;
  const float half = (b->scene.sun_diameter * 0.5f) * host::kDegToRad;
  P.c_cap = std::cos(half);
  P.c_lon = std::cos(sun_lon);
  P.s_lon = std::sin(sun_lon);
  P.c_lat = std::cos(sun_lat);
  P.s_lat = std::sin(sun_lat);
  P.wl_pool_size = b->wl_pool_size;
  P.proj = b->proj;
  P.proj_pre[0] = static_cast<float>(b->proj.img_w) / 2.0f, P.proj_pre[1] = static_cast<float>(b->proj.img_h) / 2.0f;   // the pixel formulas' conversions, once per dispatch
  P.proj_pre[2] = static_cast<float>(b->proj.lens_shift_x), P.proj_pre[3] = static_cast<float>(b->proj.lens_shift_y);
  P.cont_in = b->cont[c.out_slot ^ 1].ptr;
  P.cont_in_n = static_cast<uint32_t>(b->cont_in_n);
  P.cont_in_stride = b->cont_stride[c.out_slot ^ 1];
  P.cont_out = b->cont[c.out_slot].ptr;
  P.cont_out_stride = b->cont_stride[c.out_slot];
  P.cont_out_cap = c.out_cap;
  P.cont_in_region = b->cont_region[c.out_slot ^ 1];
  P.cont_cnt = b->cont_cnt.ptr;
  P.cont_mask = (b->opt.cont_order && !c.final_layer) ? b->cont_mask.ptr : nullptr;
  P.cont_err = c.canon_check ? b->cont_err.ptr : nullptr;
  P.counters = b->counters.ptr;
  P.mono = planes_of(b);
  P.mono_s_log2 = b->mono_s_log2;
  P.ovf = twin_of(b, b->twin_set);
  P.ovf_copies_log2 = static_cast<uint32_t>(__builtin_ctz(b->plane_copies));
  P.ovf_flag = P.ovf ? b->ovf_flag.ptr + b->twin_set : nullptr;
  P.pool_entry_fast = b->opt.pool_entry_fast ? 1u : 0u;
  P.rehit_legacy = b->opt.rehit_strategy == 0 ? 1u : 0u;
  P.tally = b->tally.ptr;
  P.exits = b->exits.ptr;
  P.exit_cap = static_cast<uint32_t>(std::min<uint64_t>(b->exits.cap, 0xFFFFFFFFull));
  P.aggregate = static_cast<uint32_t>(b->opt.aggregate);
  P.geom_clock = b->opt.geom_clock;
  P.lanes = b->lanes.ptr;
  P.lane_stride = static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h);
  P.root_profile = (b->opt.spec_root && b->spec_count == 0u) ? root_profile_of(P) : kRootProfileNone;   // (a spectrum session picks its entry in the generic root generation)
  P.fix = b->det_session ? b->fix.ptr : nullptr;   // (fix_frac, fix_frac_landed: trace_launch, once fix_prepare has settled them)
  return P;
}
// The route branch: reserves and resets the buffers of the launch's accumulation route (log set `ls`) and writes the route's fields of P — their
// only writer.  (A direct launch leaves the list fields as the entry's previous launch set them: the kernels read them only behind bin_list.)
int bind_route(HaloBackend* b, LaunchPlan& p, int ls, DispatchParams& P) {
  if (p.use_log)
    if (int rc = reserve_log_buffers(b, p, ls)) return rc;
  DevBuf<HitRec>&bin_list = b->bin_list_s[ls], &bin_list2 = b->bin_list2_s[ls];
  DevBuf<uint32_t>&bin_cnt = b->bin_cnt_s[ls], &bin_cnt2 = b->bin_cnt2_s[ls];
  if (p.use_bin)   // the staged-list route shares one buffer set and resets its counters on the main stream: one launch at a time
    if (int rc = join_aux(b)) return rc;
  if (p.use_log) {
    if (int rc = reserve_idle(b, bin_cnt, std::max<size_t>(static_cast<size_t>(p.blocks), static_cast<size_t>(512) * 16u))) return rc;
    if (int rc = reserve_idle(b, bin_cnt2, static_cast<size_t>(512) * 16u)) return rc;
    HIPCHK(b, b->ord.set_free[ls].wait_on(main_q(b)));   // the passes of the launch that last wrote this set
  } else if (p.use_bin) {
    if (int rc = reserve_idle(b, bin_cnt, static_cast<size_t>(512) * 16u)) return rc;
    HIPCHK(b, hipMemsetAsync(bin_cnt.ptr, 0, static_cast<size_t>(p.two_level ? 512u : p.bin_tiles) * 16u * sizeof(uint32_t), main_q(b)));
    if (int rc = reserve_idle(b, bin_list, p.cap1 * p.lists1)) return rc;
    if (p.two_level) {
      if (int rc = reserve_idle(b, bin_cnt2, static_cast<size_t>(p.bin_tiles) * 16u)) return rc;
      HIPCHK(b, hipMemsetAsync(bin_cnt2.ptr, 0, static_cast<size_t>(p.bin_tiles) * 16u * sizeof(uint32_t), main_q(b)));
      b->cnt2_clean[ls] = false;
      if (int rc = reserve_idle(b, bin_list2, p.cap2 * p.bin_tiles)) return rc;
    }
  }
  const bool lists = p.use_log || p.use_bin;
  P.bin_list = lists ? bin_list.ptr : nullptr;
  P.bin_log = p.use_log ? 1u : 0u;
  P.log_xyz = p.use_log_xyz ? 1u : 0u;
  P.mono_by_wl = b->mono_by_wl ? 1u : 0u;
  P.mono_copy_mask = lists ? 0u : b->plane_copies - 1u;   // logged / staged hits and their fallbacks address copy 0
  if (lists) {
    P.bin_cap = static_cast<uint32_t>(p.cap1);
    P.bin_tiles = p.use_log ? p.log_tiles : p.two_level ? b->opt.bin_l1 : p.bin_tiles;
    P.bin_shift = (p.use_bin && p.two_level) ? 14u + p.fan_log2 : 0u;
    P.bin_cnt = bin_cnt.ptr;   // (log: one fill count per region, written by the trace kernel)
  }
  if (p.use_log) P.log_plane_stride = static_cast<uint32_t>((static_cast<uint64_t>(kMonoRows) << b->mono_s_log2) * b->plane_copies);
  P.no_land = p.no_land ? 1u : 0u;
  return HALO_OK;
}
// Whether a planned, bound launch closes its session in its per-tile pass (Options::close_direct).  What is checked: it is the only launch of
// its halo_trace_layer call (one crystal entry, one chunk), on the last layer, with nothing pending in the planes — an earlier layer that put light
// on them, or an unfolded session under lazy_fold, has left mono_dirty set — on the float hit log's contiguous-tile scalar route, one plane in one
// copy, with the twin to overflow to.  (halo_begin's ray count is not consulted: a caller that traces a last layer in several calls gets a direct
// close per call, each adding its own sums to the image — the planes stay clean in between, so that is the same image.)
bool close_direct_ok(const HaloBackend& b, const LaunchPlan& p, const DispatchParams& P) {
  if (b.opt.close_direct == 0 || !p.only || p.fixed || !p.use_log || p.use_log_xyz || p.log_planes != 1u || b.mono_by_wl) return false;
  if (b.plane_cnt != 1u || b.plane_copies != 1u || b.render.visible == HALO_VISIBLE_FULL) return false;   // (full sky: interleaved tiles)
  if ((1u << p.log_t_log2) > 256u || b.mono_s_log2 + 10u - p.log_t_log2 > kBinTileLog2) return false;
  if (P.ovf == nullptr || P.ovf_flag == nullptr || b.mono_dirty || b.acc == nullptr) return false;
  return b.opt.close_direct > 0 || !p.alternate;   // auto: the hit log's own threshold chose the log; launches that fill the chip only
}
// a one-shape dispatch of a regular hexagonal prism takes the literal-normal instantiation (kGeomOneHex = 3)
int launch_geom_of(const HaloBackend& b, const LaunchPlan& p, const EntryTables& T) { return (p.geom == 0 && T.entry_fast && b.opt.hex_fast && T.hex_regular) ? kGeomOneHex : p.geom; }
// The per-tile append of a launch that closes directly (Options::tile_append): taken where the launch's kernel has a kAccTileFinal twin — the
// selector is asked (halo_select.h: plain mode, one regular prism, scalar plane, last layer with a closed gate, one of the lenses that are
// template constants, the upper sky) — and the chunk buffers of log set `ls` can be reserved.  Tiles: the close's own contiguous ones, at most
// kTileAppendMax (a small launch's 256 become 128: the kernel holds one LDS counter per tile).  A chunk holds kListSlack (8) x its even share of the
// 4 records per ray the log's regions are sized for, all chunks together within the lists' 8 GB (2^30 records: the kernel's 32-bit index) and half of
// free memory; what a chunk cannot hold goes to the twin.  A reserve that fails leaves the launch on the split route.  Writes the tile fields of P.
int bind_tile_append(HaloBackend* b, LaunchPlan& p, const EntryTables& T, int ls, DispatchParams& P) {
  P.tile_chunk = nullptr, P.tile_cnt = nullptr, P.tile_cap = P.tile_log2 = P.tile_tiles = 0u;
  P.ticket = nullptr, P.ticket_waves = P.ticket_min = P.ticket_max = 0u;
  p.tile = p.ticket = false;
  // auto: launches that fill the chip, over generated roots.  (A last layer over the continuation pool — configs[2]: five times the records per
  // launch, hot tiles past their chunks — measured slower with the append, profiles/tile_append_ab.txt: 1 takes it, auto does not.)
  if (!p.close || b->opt.tile_append == 0 || (b->opt.tile_append < 0 && (p.alternate || P.source != kSrcGen))) return HALO_OK;
  const KernelRequest req = make_request(P, T.mode, launch_geom_of(*b, p, T), b->mono_session);
  if (select_kernel(tile_request(req, false)).err != 0) return HALO_OK;   // this launch's kernel has no kAccTileFinal twin
  const uint32_t t_log2 = std::min<uint32_t>(p.log_t_log2, static_cast<uint32_t>(__builtin_ctz(kTileAppendMax)));
  if (b->mono_s_log2 + 10u < t_log2 || b->mono_s_log2 + 10u - t_log2 > kBinTileLog2) return HALO_OK;
  // Wave tickets: auto follows tile_append's auto rule (a launch that fills the chip, over generated roots), whatever tile_append itself is set to.
  // The grid is the workgroups that are resident at once — chunks and counts below are sized from it.  A wave may trace more than its even share
  // now; the chunk's cap stays 8 x the even share, and what runs over goes to the twin as before.
  // (Only where the twin has a ticketed form: halo_select.h kernel_exists.)
  // The default (-2) asks for more: a static grid of more than one resident round — a launch that fits into one round has no rounds to even out,
  // and its landed tally stays the static loop's to the last digit (tests/test_gpu_tile_append_sessions.py compares it at 1e-12).
  const int round = (b->opt.tile_ticket != 0 && select_kernel(tile_request(req, true)).err == 0) ? tile_ticket_resident_per_cu() * b->cu_count : 0;
  const bool want_ticket = round > 0 && (b->opt.tile_ticket > 0 || (!p.alternate && P.source == kSrcGen && (b->opt.tile_ticket == -1 || p.blocks > round)));
  const int resident = want_ticket ? round : 0;
  uint32_t* ticket = nullptr;
  if (resident > 0) {
    if (!b->ticket_zeroed) {   // (counters that were reserved but never seen zeroed are not used: a kernel that finds them past its passes traces nothing)
      hipError_t e0 = hipSuccess;
      if (int rc = reserve_idle(b, b->ticket_cnt, 2u * kTicketGroups * kTicketStride, &e0)) return rc;
      if (e0 == hipSuccess) {
        HIPCHK(b, hipMemsetAsync(b->ticket_cnt.ptr, 0, 2u * kTicketGroups * kTicketStride * sizeof(uint32_t), main_q(b)));
        HIPCHK(b, hipStreamSynchronize(main_q(b)));   // (once per handle: the trace streams are not ordered behind the main stream's memset)
        b->ticket_zeroed = true;
      } else (void)hipGetLastError();
    }
    if (b->ticket_zeroed && b->ticket_cnt.ptr != nullptr) ticket = b->ticket_cnt.ptr + static_cast<size_t>(ls) * kTicketGroups * kTicketStride;
  }
  const int blocks_was = p.blocks;
  if (ticket != nullptr) p.blocks = std::min(p.blocks, resident);
  const uint64_t tiles = 1ull << t_log2, blocks = static_cast<uint64_t>(p.blocks), chunks = tiles * blocks;
  const uint64_t per_wg = (p.m + blocks - 1u) / blocks;
  uint64_t cap = std::max<uint64_t>(8ull * 4ull * per_wg / tiles, 16ull);
  cap = std::min<uint64_t>(cap, (1ull << 30) / chunks);
  if (b->opt.hit_log_cap) cap = std::max<uint64_t>(b->opt.hit_log_cap / tiles, 2ull);   // tests: chunks that overflow
  size_t free_b = 0, total_b = 0;
  const uint64_t have = b->tile_chunk_s[ls].cap * sizeof(HitRec), need = cap * chunks * sizeof(HitRec);
  if (need > have && hipMemGetInfo(&free_b, &total_b) == hipSuccess && need - have > free_b / 2u)
    cap = (have + free_b / 2u) / (chunks * sizeof(HitRec));
  cap &= ~1ull;   // a chunk starts on 16 bytes
  if (cap < 2u) {
    p.blocks = blocks_was;
    return HALO_OK;
  }
  hipError_t e1 = hipSuccess, e2 = hipSuccess;
  if (int rc = reserve_idle(b, b->tile_chunk_s[ls], cap * chunks, &e1)) return rc;
  if (e1 == hipSuccess)
    if (int rc = reserve_idle(b, b->tile_cnt_s[ls], chunks, &e2)) return rc;
  if (e1 != hipSuccess || e2 != hipSuccess) {
    (void)hipGetLastError();   // out of memory: not this launch's route
    p.blocks = blocks_was;
    return HALO_OK;
  }
  if (b->opt.overlap && p.alternate) {   // the other set with it, as reserve_log_buffers does (a speed matter only)
    hipError_t e3 = hipSuccess, e4 = hipSuccess;
    if (int rc = reserve_idle(b, b->tile_chunk_s[ls ^ 1], cap * chunks, &e3)) return rc;
    if (e3 == hipSuccess)
      if (int rc = reserve_idle(b, b->tile_cnt_s[ls ^ 1], chunks, &e4)) return rc;
    if (e3 != hipSuccess || e4 != hipSuccess) (void)hipGetLastError();
  }
  p.tile = true;
  p.ticket = ticket != nullptr;
  P.ticket = ticket;
  P.ticket_waves = std::max<uint32_t>(static_cast<uint32_t>(p.blocks) * static_cast<uint32_t>(kBlock / 64) * b->opt.ticket_div / kTicketGroups, 1u);
  P.ticket_min = b->opt.ticket_min, P.ticket_max = b->opt.ticket_max;
  P.tile_chunk = b->tile_chunk_s[ls].ptr, P.tile_cnt = b->tile_cnt_s[ls].ptr;
  P.tile_cap = static_cast<uint32_t>(cap), P.tile_tiles = static_cast<uint32_t>(tiles), P.tile_log2 = b->mono_s_log2 + 10u - t_log2;
  return HALO_OK;
}
// HaloRouteInfo (halo_last_route: what the GPU tests assert routes with).  The masks name the instantiation that was launched — `k`, the
// selection launch_trace made (halo_select.h) — not the request; what the passes behind the kernel do has no counterpart in the id and comes
// from the plan: one- or two-level lists, the scalar or the X/Y/Z log.
void record_route(HaloBackend* b, const LaunchPlan& p, const DispatchParams& P, const KernelId& k) {
  b->route.launches++;
  b->route.mode_mask |= 1u << k.mode;
  b->route.geom_mask |= 1u << k.geom;
  const uint32_t log_bit = p.use_log ? (p.use_log_xyz ? 32u : 16u) : 0u;
  b->route.accum_mask |= k.acc == kAccNone                            ? 64u
                         : (k.acc == kAccFixed || k.acc == kAccFixedLog) ? (128u | log_bit)
                         : p.use_log                                      ? log_bit
                                                                          : (p.use_bin ? (p.two_level ? 8u : 4u) : (b->mono_session ? 2u : 1u));
  // specialisations: bit 0 last-layer kernel (no continuation code), 1 lens as a constant, 2 visible range as a constant, 3 closed gate as a constant
  const uint32_t spec = ((k.acc == kAccLogFinal || k.acc == kAccTileFinal) ? 1u : 0u) | (k.lens >= 0 ? 2u : 0u) | (k.vis >= 0 ? 4u : 0u) | (k.nogate ? 8u : 0u);
  b->route.spec_mask |= spec;
  if (spec == 0u) b->route.generic_launches++;
  static_assert(kRootProfileGen - 1u == kRootGenLutUniform && kRootProfileTransit - 1u == kRootTransitLutUniform, "route_root: bit kRootProfile* - 1");
  if (root_form(k.root) != kRootAny) b->route_root |= 1u << root_form(k.root);
  b->route.source_mask |= 1u << P.source;
}
// The accumulation passes of a launch, behind its trace kernel on trace stream `ts` (index ts_i), and the ring slot's closing events.
int queue_passes(HaloBackend* b, const LaunchPlan& p, const DispatchParams& P, const LaunchSlots& S, hipStream_t ts, int ts_i, hipEvent_t before_sums) {
  Order& ord = b->ord;
  Order::RingSlot& r = ord.ring[S.k];
  DevBuf<HitRec>&bin_list = b->bin_list_s[S.ls], &bin_list2 = b->bin_list2_s[S.ls];
  DevBuf<uint32_t>&bin_cnt = b->bin_cnt_s[S.ls], &bin_cnt2 = b->bin_cnt2_s[S.ls];
  // fixed-point scale of the per-tile sums (halo_kernels.hip FixQ): no slot of this launch can sum to more than 4 x max weight x rays
  const uint32_t frac_bits = fix_frac_bits(b->sess_max_w, p.m);
  const uint32_t cap2 = static_cast<uint32_t>(p.cap2 & ~15ull);   // whole 128-byte lines per tile list
  if (!p.use_log) {
    if (p.use_bin) {
      hipError_t be = p.two_level ? launch_bin_two_level(P.mono, bin_list.ptr, P.bin_cap, bin_cnt.ptr, p.lists1, bin_list2.ptr, cap2, bin_cnt2.ptr,
                                                         p.bin_tiles, p.fan_log2, frac_bits, P.ovf, P.ovf_flag, ts, before_sums)
                                  : launch_bin_accumulate(P.mono, bin_list.ptr, P.bin_cap, bin_cnt.ptr, p.bin_tiles, frac_bits, ts);
      if (be != hipSuccess) return hip_fail(b, be, "halo_bin_accumulate_kernel launch");
      HIPCHK(b, ord.sums_queued(ts, ts_i, p.sums_plain()));
    }
    HIPCHK(b, hipEventRecord(r.ev1, ts));
    r.posts = false;
    HIPCHK(b, ord.slot_done(r, ts));
    return HALO_OK;
  }
  // the accumulation passes of this launch: behind the trace kernel on its stream.  (Round 5 tried them on the auxiliary stream, under the
  // next launch's trace kernel: configs[1] + 1.2 %, the trace kernel itself 5 % slower for the CUs the 134 KB split workgroups take, the
  // passes' spans stretched sevenfold — profiles that no longer say what a kernel costs, for one percent.  Not kept.)
  HIPCHK(b, hipEventRecord(r.ev1, ts));          // the trace kernel alone: ev0 .. ev1
  hipStream_t ps = ts;
  if (p.under_fold()) {   // the passes add to the planes: behind the fold that last touched THEIR planes
    if (b->mono_two) {   // two plane sets: that is the fold of two sessions ago (it zeroed this set), not the one the trace kernel started under
      HIPCHK(b, ord.set_folded[b->mono_set].wait_on(ps));
    } else HIPCHK(b, ord.wait_for_aux(ts_i));
  }
  // (nothing between ev1 and here unless the passes wait for a fold: one record serves as both, the spans stay the trace kernel's and the passes')
  HIPCHK(b, ord.passes_begin(r, ps, !p.under_fold()));
  if (p.close && p.tile) {
    // the closing pass over the chunks the trace kernel filled: no split, no list counters; the twin's flag is cleared behind the pass as below
    const float coef[3] = {b->plane_coef[0][0], b->plane_coef[0][1], b->plane_coef[0][2]};
    hipError_t ce = launch_tile_route_close(b->acc, static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h), coef, P.tile_chunk, P.tile_cap, P.tile_cnt,
                                            static_cast<uint32_t>(p.blocks), P.tile_tiles, b->mono_s_log2, frac_bits, P.ovf, P.ovf_flag, ps, before_sums, P.ticket);
    if (ce != hipSuccess) return hip_fail(b, ce, "halo_tile_close_kernel launch");
    b->direct_closes++;
    b->tile_appends++;
    if (p.ticket) b->tile_tickets++;
    static const bool debug_counts = std::getenv("HALO_DEBUG_TILE_COUNTS") != nullptr;
    if (debug_counts) {   // (a host sync per launch: what the chunks of this launch hold, for profiles/ — never on a timed path)
      std::vector<uint32_t> cnt(static_cast<size_t>(P.tile_tiles) * static_cast<size_t>(p.blocks));
      HIPCHK(b, hipStreamSynchronize(ps));
      HIPCHK(b, hipMemcpy(cnt.data(), P.tile_cnt, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
      uint64_t met = 0, over = 0, most = 0, empty = 0;
      for (uint32_t c : cnt) met += c, over += c > P.tile_cap ? 1u : 0u, most = std::max<uint64_t>(most, c), empty += c == 0u ? 1u : 0u;
      std::fprintf(stderr, "[halo tile counts] workgroups %d tiles %u cap %u chunks %zu records %llu per chunk %.1f longest %llu empty %llu over cap %llu\n", p.blocks, P.tile_tiles,
                   P.tile_cap, cnt.size(), static_cast<unsigned long long>(met), static_cast<double>(met) / static_cast<double>(cnt.size()), static_cast<unsigned long long>(most),
                   static_cast<unsigned long long>(empty), static_cast<unsigned long long>(over));
    }
    HIPCHK(b, ord.close_marks(r, ps, ts_i, S.ls));   // (the close, the passes' span, the log set free, the slot done: Order::close_marks)
    if (b->opt.overlap && p.alternate) b->log_set ^= 1;
    r.posts = true;
    return HALO_OK;
  }
  if (p.close) {
    // the split and the closing per-tile pass, which leaves nothing behind: counters zeroed by the workgroups that consumed them (the memset in front
    // of the split goes: 4-7 us per launch, profiles/direct_close_ab.txt), the twin's flag cleared behind the pass, the planes untouched (mono_dirty stays false: no fold follows)
    if (!b->cnt2_clean[S.ls]) HIPCHK(b, hipMemsetAsync(bin_cnt2.ptr, 0, static_cast<size_t>(p.log_tiles) * 16u * sizeof(uint32_t), ps));
    const float coef[3] = {b->plane_coef[0][0], b->plane_coef[0][1], b->plane_coef[0][2]};
    hipError_t ce = launch_log_route_close(b->acc, static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h), coef, bin_list.ptr, P.bin_cap, bin_cnt.ptr,
                                           static_cast<uint32_t>(p.blocks), bin_list2.ptr, cap2, bin_cnt2.ptr, 1u << p.log_t_log2, b->mono_s_log2, frac_bits, P.ovf, P.ovf_flag,
                                           ps, before_sums);
    if (ce != hipSuccess) return hip_fail(b, ce, "halo_split_kernel launch (direct close)");
    b->cnt2_clean[S.ls] = true;
    b->direct_closes++;
    HIPCHK(b, ord.close_marks(r, ps, ts_i, S.ls));   // (the close, the passes' span, the log set free, the slot done: Order::close_marks)
    if (b->opt.overlap && p.alternate) b->log_set ^= 1;
    r.posts = true;
    return HALO_OK;
  }
  HIPCHK(b, hipMemsetAsync(bin_cnt2.ptr, 0, static_cast<size_t>(p.log_tiles) * 16u * sizeof(uint32_t), ps));
  b->cnt2_clean[S.ls] = false;
  // (a deterministic launch: the integer twins of the passes, onto the integer planes with the pending plane set's F.  Every writer of those planes
  //  adds with an integer atomic, so the passes take no `before_sums` and leave no rmw marker: nothing has to be ordered against them but the fold.)
  hipError_t be = p.fixed ? (p.use_log_xyz ? launch_log_route_xyz_fixed(P.fix, P.log_plane_stride, bin_list.ptr, P.bin_cap, bin_cnt.ptr, static_cast<uint32_t>(p.blocks), bin_list2.ptr, cap2,
                                                                        bin_cnt2.ptr, p.log_tiles, b->mono_s_log2, P.wl_pool, P.wl_pool_size, b->fix_frac, ps)
                                           : launch_log_route_fixed(P.fix, bin_list.ptr, P.bin_cap, bin_cnt.ptr, static_cast<uint32_t>(p.blocks), bin_list2.ptr, cap2, bin_cnt2.ptr,
                                                                    1u << p.log_t_log2, b->mono_s_log2, b->render.visible == HALO_VISIBLE_FULL, b->fix_frac, ps))
                  : p.use_log_xyz ? launch_log_route_xyz(P.mono, P.log_plane_stride, bin_list.ptr, P.bin_cap, bin_cnt.ptr, static_cast<uint32_t>(p.blocks),
                                                       bin_list2.ptr, cap2, bin_cnt2.ptr, p.log_tiles, b->mono_s_log2, P.wl_pool, P.wl_pool_size, frac_bits, P.ovf, P.ovf_flag, P.ovf_copies_log2, ps, before_sums)
                                : launch_log_route(P.mono, bin_list.ptr, P.bin_cap, bin_cnt.ptr, static_cast<uint32_t>(p.blocks), bin_list2.ptr, cap2,
                                                   bin_cnt2.ptr, 1u << p.log_t_log2, p.log_planes, b->mono_s_log2, b->render.visible == HALO_VISIBLE_FULL, frac_bits,
                                                   P.ovf, P.ovf_flag, P.ovf_copies_log2, ps, before_sums);
  if (be != hipSuccess) return hip_fail(b, be, "halo_split_kernel launch");
  HIPCHK(b, ord.sums_queued(ps, ts_i, p.sums_plain()));
  HIPCHK(b, hipEventRecord(r.ev3, ps));
  HIPCHK(b, ord.set_free[S.ls].mark(ps));
  if (b->opt.overlap && p.alternate) b->log_set ^= 1;
  r.posts = true;
  HIPCHK(b, ord.slot_done(r, ps));
  return HALO_OK;
}
// Stream choice, plane gates, generator, trace kernel, route record and passes of one launch whose tables, shapes and buffers are in place.
int queue_launch(HaloBackend* b, const LaunchPlan& p, const HaloEntry& E, EntryTables& T, const DispatchParams& P, const LaunchSlots& S) {
  Order& ord = b->ord;
  Order::RingSlot& r = ord.ring[S.k];
  // The launch's trace stream (alternating for small launches), behind whatever the auxiliary stream still does to the planes (a closing
  // fold): the launch adds to them — from the trace kernel itself (direct atomics, staged lists) or in its passes, which follow it on
  // the same stream.  (A small logged launch starts under that fold: LaunchPlan::under_fold.)
  hipStream_t ts = nullptr;
  int ts_i = 0;
  HIPCHK(b, ord.next_trace_stream(!p.under_fold(), p.alternate, &ts, &ts_i));
  HIPCHK(b, ord.behind_other_close(ts, ts_i));   // a direct close on the other trace stream: it writes the image and the twin's half plainly
  hipEvent_t before_sums = nullptr;   // rule (1), for the routes whose sums write the planes plainly
#ifndef HALO_NO_PLANE_GATES   // (defined only to see tests/test_gpu_production_routes.py's two-stream test fail without the gates)
  if (!p.use_log) HIPCHK(b, ord.behind_other_sums(ts, ts_i));   // this trace kernel adds to the planes itself: behind the other stream's sums
  if (p.sums_plain()) HIPCHK(b, ord.gate_sums(ts_i, &before_sums));
#endif
  if (!p.deterministic && !p.host_pool) {
    // Device generator: one team per sampled crystal, in front of the trace kernel on its stream.  Option "gen_ahead" puts the one of a
    // launch that fills the chip on trace stream 1 instead, beside the previous launch's trace kernel and passes (it needs nothing of
    // them, only its pool back from the launch before that one).  Measured (25 M rays per launch): prism pools 4.43 -> 4.55 ms per launch,
    // pyramid pools 7.78 -> 7.70: both kernels are VALU-bound, so sharing the chip conserves the work.  Off by default.
    const bool ahead = b->opt.overlap && b->opt.gen_ahead && !p.alternate;
    hipStream_t gs = ahead ? ord.gen_ahead_stream() : ts;
    HIPCHK(b, ord.shapes_free[S.shape_set].wait_on(gs));
    hipError_t ge = launch_shapegen(const_cast<ShapeDev*>(P.shapes), p.geom == 2, p.shape_cnt, b->seed, host::MakeRecipe(E.crystal), S.first_shape, gs, b->opt.gen_serial != 0);
    if (ge != hipSuccess) return hip_fail(b, ge, "halo_shapegen_kernel launch");
    if (ahead) HIPCHK(b, ord.behind_generator(ts));
  }
  HIPCHK(b, hipEventRecord(r.ev0, ts));  // HIP events on the launch stream bracket the kernel alone
  r.final = P.final_layer != 0u;
  const int launch_geom = launch_geom_of(*b, p, T);
  KernelId launched;
  hipError_t le = launch_trace(P, p.blocks, ts, T.mode, launch_geom, b->mono_session, &launched);
  if (T.ce) {   // the slot's last reader (see TableCacheEntry): this launch, whose slot-done event is recorded below
    T.ce->read_ring[T.ce->cur] = S.k;
    T.ce->read_use[T.ce->cur] = r.use;
  }
  // (a launch that closes its session itself leaves the planes as it found them; so does one of the no-accumulation kernels — no_land on one shape,
  // halo_select.h select_kernel: kAccNone has no cache, no exit queue and no code that touches a plane, the log or the twin.  The latter holds for
  // EVERY such launch, eligible for a direct close or not: a session of such launches alone queues no fold of planes nobody wrote.)
  if (!p.close && !(p.no_land && p.geom == 0)) b->mono_dirty = true;
  b->fix_planes = b->det_session;
  if (le != hipSuccess) return hip_fail(b, le, "halo_trace_kernel launch");   // (nothing ran: no route to record)
  record_route(b, p, P, launched);
  if (!p.deterministic) HIPCHK(b, ord.shapes_free[S.shape_set].mark(ts));
  if (int rc = queue_passes(b, p, P, S, ts, ts_i, before_sums)) return rc;
  b->tally_unread = true;
  r.busy = true;
  return HALO_OK;
}
// Before a deterministic launch of `m` rays: the scales it adds with.  All adds into one unfolded plane set share one F, so the pending planes are
// folded first when F has to change (a session of other weights under lazy_fold, host rays heavier than the pool's) or the set's budget is
// spent; the landed integer is taken to the host before ITS scale changes.
int fix_prepare(HaloBackend* b, uint64_t m) {
  const uint32_t f = fix_frac_bits(b->sess_max_w, kFixBudgetHits), fl = fix_frac_bits(b->sess_max_w, kFixLandedHits);
  if (b->mono_dirty && b->fix_planes && (f != b->fix_frac || b->fix_hits + m > kFixBudgetHits))
    if (int rc = fold_queue(b)) return rc;   // (on the auxiliary stream; the launch is queued behind it: next_trace_stream)
  if (!(b->mono_dirty && b->fix_planes)) {
    b->fix_frac = f;
    b->fix_hits = 0;
  }
  b->fix_hits += m;
  if (fl != b->fix_frac_landed) {
    // (a shard's own landed integer is a part of the whole and leaves as the integer it is: converted here it would stay behind on this handle.
    //  What halo_import_fixed brought in is whole, and goes to landed_carry exactly as one handle's own integer does)
    if (b->shard_count > 1 && b->landed_own)
      return fail(b, HALO_FATAL, "shard " + std::to_string(b->shard_index) + " of " + std::to_string(b->shard_count) +
                                     ": this session's weights change the scale of the landed integer (F_landed) while the shard still holds landed weight of its own; move it out with halo_export_fixed first");
    if (int rc = join_aux(b)) return rc;
    double now[kSumNum];
    unsigned long long fix_now = 0ull;
    if (int rc = read_tally(b, now, &fix_now)) return rc;
    b->landed_carry += std::ldexp(static_cast<double>(fix_now - b->fix_landed_seen), -static_cast<int>(b->fix_frac_landed));
    b->fix_landed_seen = fix_now;
    b->fix_frac_landed = fl;
  }
  return HALO_OK;
}
// One planned launch from end to end: shape pool, ring slot, tables, the per-launch fields of P, route buffers, then queue_launch.
int trace_launch(HaloBackend* b, const LayerCtx& c, LaunchPlan& p, EntryTables& T, DispatchParams& P) {
  const HaloEntry& E = b->scene.layers[c.layer].entries[p.ci];
  const uint64_t m = p.m;
  LaunchSlots S;
  std::vector<ShapeDev> pool((p.deterministic && !T.cached) || p.host_pool ? p.shape_cnt : 0u);
  for (uint32_t k = 0; k < static_cast<uint32_t>(pool.size()); k++) {
    if (c.host_crystal) host::ToShapeDev(*c.rays->crystal, pool[k]);
    else host::MakeShapeDev(b->seed, E.crystal, p.deterministic ? 0 : (b->shape_count + k), pool[k]);
  }
  S.first_shape = b->shape_count;
  if (!p.deterministic) {
    b->shape_count += p.shape_cnt;
    b->sess_crystal_samples += p.shape_cnt;
  }
  if (c.rays == nullptr && (E.axis.azimuth.type != HALO_DIST_NONE || E.axis.latitude.type != HALO_DIST_NONE || E.axis.roll.type != HALO_DIST_NONE))
    b->sess_orient_samples += m;   // AxisDistribution::IsAxisDeterministic is false: one orientation per ray
  bool wrapped = false;
  S.k = b->ord.take(&wrapped);
  if (wrapped) harvest_slot(b, b->ord.ring[S.k]);  // blocks only if the ring has wrapped onto a dispatch still in flight
  DispatchSlot* ds = nullptr;
  if (int rc = upload_tables(b, c, p, E, P.lat_path, pool.empty() ? nullptr : pool.data(), S.k, T, &ds)) return rc;
  P.lut = ds->lut;
  P.wl_pool = ds->wl;
  P.filter = T.use_filter ? &ds->filter : nullptr;
  P.color = T.use_color ? &ds->color : nullptr;
  P.fast = T.has_fast ? &ds->fast : nullptr;
  P.cont_in_seg = ds->seg;
  P.entry_fast = T.entry_fast ? &ds->efast : nullptr;
  if (p.deterministic) {
    P.shapes = &ds->shape;
  } else {
    // Two pools, taken in turn by the launches that may run beside a neighbour: the records of launch k+1 are written while launch k still
    // traces out of the other one.
    const bool turn = b->opt.overlap && (p.alternate || b->opt.gen_ahead);   // (a launch that fills the chip runs alone on stream 0: pool 0)
    S.shape_set = turn ? b->shapes_next : 0;
    if (turn) b->shapes_next ^= 1;
    DevBuf<ShapeDev>& shapes = b->shapes_s[S.shape_set];
    if (int rc = reserve_idle(b, shapes, p.shape_cnt)) return rc;   // sized for ShapeDev records; prism pools use the front third
    if (turn)   // (its twin with it, for the same reason as the log's second buffer set)
      if (int rc = reserve_idle(b, b->shapes_s[S.shape_set ^ 1], p.shape_cnt)) return rc;
    if (p.host_pool) {
      HIPCHK(b, b->ord.shapes_free[S.shape_set].wait_on(main_q(b)));
      HIPCHK(b, hipMemcpyAsync(shapes.ptr, pool.data(), pool.size() * sizeof(ShapeDev), hipMemcpyHostToDevice, main_q(b)));
    }
    // (device generator: queued by queue_launch on the launch's trace stream, in front of the trace kernel)
    P.shapes = shapes.ptr;
  }
  P.shape_cnt = p.shape_cnt;
  P.n_rays = static_cast<uint32_t>(m);
  P.ci_start = static_cast<uint32_t>(p.first);
  P.spec_per = P.spec_k0 = P.spec_rem = P.spec_last = 0u;
  if (b->spec_count != 0u && c.layer == 0) {   // the blocks lie within this crystal entry's share (p.share rays), whatever the launches cut out of it
    const SpectrumChunkDev sc = SpectrumChunk(p.share, b->spec_count, p.off);
    P.spec_per = sc.per, P.spec_k0 = sc.k0, P.spec_rem = sc.rem, P.spec_last = sc.last;
  }
  auto split = [](uint64_t v, uint32_t& lo, uint32_t& hi) { lo = static_cast<uint32_t>(v & 0xFFFFFFFFull), hi = static_cast<uint32_t>(v >> 32); };  // SplitPcgRayBase trace_backend.hpp:184-190
  split(b->gen_count, P.gen_lo, P.gen_hi);
  split(b->gate_count, P.gate_lo, P.gate_hi);
  split(b->transit_count, P.transit_lo, P.transit_hi);
  if (c.rays) {
    P.host_d = b->host_f.ptr + p.off * 3;
    P.host_p = b->host_f.ptr + c.n * 3 + p.off * 3;
    P.host_w = b->host_f.ptr + c.n * 6 + p.off;
    P.host_tf = b->host_u.ptr + p.off;
  }
  plan_route(*b, c, T.fast_mode, p);
  if (p.fixed) {
    if (T.mode != 0 && T.mode != 1) return fail(b, HALO_FATAL, "deterministic = 1: this entry needs kernels without a fixed-point route");   // (halo_begin refuses these scenes: never a float route)
    if (int rc = fix_prepare(b, m)) return rc;
    P.fix_frac = b->fix_frac;
    P.fix_frac_landed = b->fix_frac_landed;
  }
  S.ls = (b->opt.overlap && p.alternate) ? b->log_set : 0;   // the buffer set of this launch
  if (int rc = bind_route(b, p, S.ls, P)) return rc;
  p.close = close_direct_ok(*b, p, P);
  if (int rc = bind_tile_append(b, p, T, S.ls, P)) return rc;
  if (int rc = queue_launch(b, p, E, T, P, S)) return rc;
  if (p.host_pool) HIPCHK(b, hipStreamSynchronize(main_q(b)));  // the pageable shape pool must outlive its copy (the copy is on the main stream)
  if (P.source == kSrcGen) b->gen_count += m;
  if (P.source == kSrcTransit) b->transit_count += m;
  b->gate_count += m;
  return HALO_OK;
}
// The launch loop of a shard (halo_set_shard count > 1; one layer, generated roots): the whole layer's plan is walked and the counters — root, gate
// and shape streams — move on by every planned launch as they do on one rank, but only the part of a launch inside this shard's slice of its crystal
// entry is queued, as a launch of its own that keeps the bases it has in the whole run: stream counters at its first ray, the shape stream at its
// first shape, `off` and `share` of the entry (the spectrum blocks), `first` within the layer (HaloExitRecord::root).  A trace kernel reads shape
// tid / geom_clock of ITS launch, so a part must start on a shape of its planned launch: slices start at clock multiples within the entry, planned
// launches start at multiples of the chunk — a sampled entry whose launches do not start on shapes is refused, before anything is queued.
int trace_shard(HaloBackend* b, LayerCtx& c, std::vector<LaunchPlan>& plans, const std::vector<uint64_t>& per_ci) {
  for (const LaunchPlan& p : plans)
    if (!p.deterministic && p.off % b->opt.geom_clock != 0u)
      return fail(b, HALO_FATAL, "halo_set_shard count > 1: a sampled crystal entry is cut into launches (chunk, stoch_chunk) that are not multiples of geom_clock; a shard cannot start inside a sampled shape");
  // (checked here, before a counter has moved; fix_prepare holds the same line for every launch)
  if (b->det_session && b->landed_own && fix_frac_bits(b->sess_max_w, kFixLandedHits) != b->fix_frac_landed)
    return fail(b, HALO_FATAL, "shard " + std::to_string(b->shard_index) + " of " + std::to_string(b->shard_count) +
                                   ": this session's weights change the scale of the landed integer (F_landed) while the shard still holds landed weight of its own; move it out with halo_export_fixed first");
  EntryTables T;
  DispatchParams P{};
  int cur = -1;
  c.traced = 0;
  for (const LaunchPlan& whole : plans) {
    uint64_t s0 = 0, sn = 0;
    shard_slice(per_ci[static_cast<size_t>(whole.ci)], whole.deterministic ? 1u : b->opt.geom_clock, b->shard_index, b->shard_count, &s0, &sn);
    const uint64_t lo = std::max(whole.off, s0), hi = std::min(whole.off + whole.m, s0 + sn);
    const uint64_t gen0 = b->gen_count, gate0 = b->gate_count, shape0 = b->shape_count;
    if (lo < hi) {
      LaunchPlan p = plan_launch(*b, c, whole.ci, whole.first - whole.off, lo, hi - lo);   // (hi - lo <= whole.m: one launch)
      p.share = whole.share;
      b->gen_count = gen0 + (lo - whole.off);
      b->gate_count = gate0 + (lo - whole.off);
      if (!whole.deterministic) b->shape_count = shape0 + (lo - whole.off) / b->opt.geom_clock;
      if (p.ci != cur) {
        cur = p.ci;
        prepare_entry_tables(b, c, cur, T);
        P = fill_params(b, c, cur);
      }
      // (trace_launch may first fold pending planes whose budget or scale is spent — fix_prepare: imported ones, which are whole, fold; the
      //  shard's own are refused)
      if (int rc = trace_launch(b, c, p, T, P)) return rc;
      b->fix_imported = false;   // what is pending from here on is, at least in part, this shard's own
      b->landed_own = b->det_session;
      c.traced += p.m;
    }
    b->gen_count = gen0 + whole.m;
    b->gate_count = gate0 + whole.m;
    if (!whole.deterministic) b->shape_count = shape0 + whole.shape_cnt;
  }
  if (b->det_session && !(b->mono_dirty && b->fix_planes)) {
    // nothing of this shard's is in the planes (empty slices): they are pending all the same — all zero, at the session's scales — so that the shard
    // exports like every other
    if (int rc = fix_prepare(b, 0)) return rc;
    b->mono_dirty = true;
    b->fix_planes = true;
    b->fix_imported = false;
  }
  return HALO_OK;
}
// The end of a layer: counters, shard fill counts and the error word come back, the next layer's segment table and the statistics are made.
int close_layer(HaloBackend* b, const LayerCtx& c, bool defer, HaloLayerStats* stats) {
  const uint64_t n = c.n;
  if (defer) {  // queued, not waited for: the tallies arrive through halo_collect_stats
    b->layer_acc.root_count += c.traced;
    if (stats) {
      std::memset(stats, 0, sizeof(*stats));
      stats->root_count = c.traced;
    }
    b->cont_in_n = 0;
    return HALO_OK;
  }
  if (int rc = join_aux(b)) return rc;   // the copies below (and the caller) want this layer's kernels done: the main stream waits for the trace streams
  uint32_t cnt[kCntNum] = {0, 0, 0, 0};
  std::vector<uint32_t> fill(c.final_layer ? 0 : kContShards * kContCntStride);
  HIPCHK(b, hipMemcpyAsync(cnt, b->counters.ptr, sizeof(cnt), hipMemcpyDeviceToHost, main_q(b)));
  if (!c.final_layer) HIPCHK(b, hipMemcpyAsync(fill.data(), b->cont_cnt.ptr, fill.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, main_q(b)));
  uint32_t cont_err = 0;
  if (c.canon_check) HIPCHK(b, hipMemcpyAsync(&cont_err, b->cont_err.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, main_q(b)));
  if (b->tally_unread) {
    if (int rc = pull_tally(b)) return rc;   // (one more small copy and THE stream sync of this call: the two copies above are complete behind it)
  } else {
    HIPCHK(b, hipStreamSynchronize(main_q(b)));
  }
  harvest_all(b);
  if (cont_err != 0u)   // never a pool handed on (or traced) out of canonical order in silence
    return cont_order_fail(b, cont_err);
  uint64_t n_cont = 0;
  if (!c.final_layer) {  // the next layer addresses the pool through the prefix of the shard fill counts
    b->cont_fill_max = 0;
    for (int sI = 0; sI < kContShards; sI++) {
      const uint32_t cs = fill[static_cast<size_t>(sI) * kContCntStride];
      // (canonical order included: a pool that lost records would be handed on with holes in its order — never, the session fails)
      if (cs > c.out_cap) return fail(b, HALO_FATAL, b->opt.cont_order ? "continuation pool overflow (cont_order = 1: the canonical pool would be incomplete)" : "continuation pool overflow");
      b->cont_seg[sI] = static_cast<uint32_t>(n_cont);
      n_cont += cs;
      b->cont_fill_max = std::max(b->cont_fill_max, cs);
    }
    b->cont_seg[kContShards] = static_cast<uint32_t>(n_cont);
    b->cont_roots = n;
  }
  b->exits_pending = std::min<uint64_t>(cnt[kCntExit], b->exits.cap);
  b->layer_acc.root_count = c.traced;
  b->layer_acc.continuation_count = n_cont;
  if (stats) *stats = b->layer_acc;
  add_stats(b->pending, b->layer_acc);
  b->layer_acc = HaloLayerStats{};
  b->cont_in_n = n_cont;  // becomes the next layer's input at Recombine
  return HALO_OK;
}
}  // namespace

extern "C" {
int halo_trace_layer(halo_handle_t b, uint64_t count, const HaloHostRays* rays, HaloLayerStats* stats) {
  if (!b) return HALO_FATAL;
  if (!b->in_session) return fail(b, HALO_FATAL, "TraceLayer outside a session");
  LayerCtx c;
  const int layer = c.layer = b->layer_idx;
  if (layer >= b->scene.layer_count) return fail(b, HALO_FATAL, "TraceLayer past the last layer");
  HIPCHK(b, hipSetDevice(b->device));
  const HaloLayer& L = b->scene.layers[layer];
  const uint64_t n = c.n = c.traced = (layer == 0) ? count : b->cont_in_n;
  c.final_layer = (layer == b->scene.layer_count - 1);
  if (n > 0xFFFFFFF0ull) return fail(b, HALO_FATAL, "more than 2^32 rays in one layer dispatch; split the batch");
  if (layer > 0 && rays) return fail(b, HALO_FATAL, "host rays are first-layer only");
  if (rays && b->shard_count > 1) return fail(b, HALO_FATAL, "halo_set_shard count > 1: host-injected rays are not supported (a shard generates its slice of the session's roots)");
  if (rays && rays->crystal) {   // an injected crystal is copied into fixed-size device tables: its counts and indices are the caller's, check them
    const HaloGeomTables& g = *rays->crystal;
    if (g.face_cnt < 0 || g.face_cnt > HALO_MAX_FACES || g.tri_cnt < 0 || g.tri_cnt > HALO_MAX_TRIS)   // (0 faces = the empty crystal: its rays carry no weight)
      return fail(b, HALO_FATAL, "host crystal: face_cnt / tri_cnt outside 0..HALO_MAX_FACES / 0..HALO_MAX_TRIS");
    for (int t = 0; t < g.tri_cnt; t++)
      if (g.tri_face[t] < 0 || g.tri_face[t] >= g.face_cnt) return fail(b, HALO_FATAL, "host crystal: tri_face refers to a face outside the table");
  }
  c.rays = rays;
  c.source = rays ? kSrcHost : (layer == 0 ? kSrcGen : kSrcTransit);
  c.host_crystal = rays != nullptr && rays->crystal != nullptr && layer == 0;
  c.out_slot = b->cont_out_slot;
  // canonical order over several layers: every layer ends with the error-word check (the appends of this layer, the reorder in front of it)
  c.canon_check = b->opt.cont_order && b->scene.layer_count > 1;
  float props[HALO_MAX_ENTRIES];
  for (int ci = 0; ci < L.entry_count; ci++) props[ci] = L.entries[ci].proportion;
  std::vector<uint64_t> per_ci = host::Partition(props, L.entry_count, n, b->carry[layer]);
  if (rays && layer == 0) {  // host ingest is a single population (cpu_trace_backend.cpp:121-127)
    std::fill(per_ci.begin(), per_ci.end(), 0);
    per_ci[0] = n;
  }
  // chunked launches, planned once: the continuation pool below is sized from the plans the launch loop walks
  std::vector<LaunchPlan> plans;
  uint64_t ci_start = 0;
  for (int ci = 0; ci < L.entry_count; ci_start += per_ci[ci], ci++)
    for (uint64_t off = 0; off < per_ci[ci]; off += plans.back().m) plans.push_back(plan_launch(*b, c, ci, ci_start, off, per_ci[ci] - off));
  // continuation output pool: kContShards regions; a region must hold everything its blocks can emit over the layer's
  // dispatches (every root emits at most max_hits candidates)
  if (!c.final_layer) {
    uint64_t region = 0;
    for (const LaunchPlan& p : plans) {
      const uint64_t nb = static_cast<uint64_t>(p.blocks);
      const uint64_t per_block = (p.m + nb * kBlock - 1) / (nb * kBlock) * kBlock;   // grid-stride share, rounded up
      region += (nb + kContShards - 1) / kContShards * per_block * static_cast<uint64_t>(b->scene.max_hits);
    }
    region = (region + 63) & ~63ull;
    const uint64_t stride = region * kContShards;
    if (stride > 0xFFFFFFF0ull) return fail(b, HALO_FATAL, "continuation pool would exceed 2^32 rays; split the batch");
    // + mask lo/hi planes with raypath colour; canonical order: + root and interaction planes (kContPlaneRoot, kContPlaneBit)
    const uint64_t planes = b->opt.cont_order ? kContPlanesCanonical : (b->color_classes.empty() ? 5 : 7);
    if (b->opt.cont_order && stride * planes > 0xFFFFFFFFull) return fail(b, HALO_FATAL, "canonical continuation pool planes would exceed 2^32 floats; split the batch");
    if (int rc = reserve_idle(b, b->cont[c.out_slot], stride * planes)) return rc;
    b->cont_stride[c.out_slot] = static_cast<uint32_t>(stride);
    b->cont_region[c.out_slot] = static_cast<uint32_t>(region);
    c.out_cap = static_cast<uint32_t>(region);
    HIPCHK(b, b->cont_cnt.reserve(kContShards * kContCntStride));
    HIPCHK(b, hipMemsetAsync(b->cont_cnt.ptr, 0, kContShards * kContCntStride * sizeof(uint32_t), main_q(b)));
    if (b->opt.cont_order) {   // the roots' masks start empty: queued on the stream, behind the scatter that read the previous layer's
      if (b->opt.rehit_strategy == 0) return fail(b, HALO_FATAL, "cont_order = 1 needs rehit_strategy = 1 (the legacy strategy can emit twice at one interaction)");
      if (int rc = reserve_idle(b, b->cont_mask, kContMaskWords * std::max<uint64_t>(c.n, 1))) return rc;
      HIPCHK(b, hipMemsetAsync(b->cont_mask.ptr, 0, kContMaskWords * c.n * sizeof(uint32_t), main_q(b)));
      if (c.layer == 0) {   // a session starts with a clean error word (a session that set one was refused)
        if (int rc = reserve_idle(b, b->cont_err, 16)) return rc;
        HIPCHK(b, hipMemsetAsync(b->cont_err.ptr, 0, sizeof(uint32_t), main_q(b)));
      }
    }
  }
  const bool defer = b->opt.async && c.final_layer && !b->opt.capture && !c.canon_check;  // nothing the caller needs before the next call
  if (!defer) {  // earlier queued dispatches go to `pending`, so layer_acc ends up holding this layer alone
    harvest_all(b);
    if (int rc = pull_tally(b)) return rc;   // (a copy + sync only when something was queued and never collected)
    add_stats(b->pending, b->layer_acc);
    b->layer_acc = HaloLayerStats{};
  }
  if (b->opt.capture) {
    const uint64_t need = b->exits_pending + n * static_cast<uint64_t>(b->scene.max_hits + 1);
    if (need > b->exits.cap) {
      DevBuf<HaloExitRecord> bigger;
      HIPCHK(b, bigger.reserve(need));
      if (b->exits_pending)
        HIPCHK(b, hipMemcpyAsync(bigger.ptr, b->exits.ptr, b->exits_pending * sizeof(HaloExitRecord), hipMemcpyDeviceToDevice, main_q(b)));
      if (int rc = sync_all(b)) return rc;
      b->exits.swap(bigger);   // (the old buffer goes with `bigger`)
    }
  }
  if (rays && layer == 0) {   // host rays bring their own weights (and hand them on to the layers behind)
    for (uint64_t i = 0; i < n; i++) b->sess_max_w = std::max(b->sess_max_w, static_cast<double>(std::fabs(rays->w[i])));
    // a queued session's kernel on a trace stream (async + overlap) may still be reading the previous batch out of these buffers: the copies
    // go behind everything the trace / auxiliary streams hold, and a buffer only grows with all streams idle
    if (int rc = join_aux(b)) return rc;
    if (int rc = reserve_idle(b, b->host_f, n * 7)) return rc;
    if (int rc = reserve_idle(b, b->host_u, n)) return rc;
    HIPCHK(b, hipMemcpyAsync(b->host_f.ptr, rays->d, n * 3 * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
    HIPCHK(b, hipMemcpyAsync(b->host_f.ptr + n * 3, rays->p, n * 3 * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
    HIPCHK(b, hipMemcpyAsync(b->host_f.ptr + n * 6, rays->w, n * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
    HIPCHK(b, hipMemcpyAsync(b->host_u.ptr, rays->tf, n * sizeof(uint32_t), hipMemcpyHostToDevice, main_q(b)));
    HIPCHK(b, hipStreamSynchronize(main_q(b)));
  }
  // the launches: an entry's tables and shared parameters are made when its first launch comes up
  EntryTables T;
  DispatchParams P{};
  int cur = -1;
  if (plans.size() == 1u) plans[0].only = c.final_layer;
  if (b->shard_count > 1) {
    if (int rc = trace_shard(b, c, plans, per_ci)) return rc;
    return close_layer(b, c, defer, stats);
  }
  for (LaunchPlan& p : plans) {
    if (p.ci != cur) {
      cur = p.ci;
      prepare_entry_tables(b, c, cur, T);
      P = fill_params(b, c, cur);
    }
    if (int rc = trace_launch(b, c, p, T, P)) return rc;
  }
  return close_layer(b, c, defer, stats);
}

int halo_generate_shapes(halo_handle_t b, const HaloCrystal* crystal, uint64_t first_index, uint32_t n, int on_device, HaloGeomTables* out) {
  if (!b || !crystal || (!out && n)) return HALO_FATAL;
  if (crystal->kind != HALO_CRYSTAL_PRISM && crystal->kind != HALO_CRYSTAL_PYRAMID) return fail(b, HALO_FATAL, "unknown crystal kind");
  std::vector<ShapeDev> pool(n);
  if (on_device == 2 && crystal->kind == HALO_CRYSTAL_PRISM) {   // the prism-pool generator (1360-byte ShapePrism records, one team of 16 lanes per crystal)
    HIPCHK(b, hipSetDevice(b->device));
    DevBuf<ShapePrism> dev;
    HIPCHK(b, dev.reserve(n));
    std::vector<ShapePrism> recs(n);
    hipError_t ge = launch_shapegen(dev.ptr, true, n, b->seed, host::MakeRecipe(*crystal), first_index, main_q(b), b->opt.gen_serial != 0);
    if (ge == hipSuccess) ge = hipMemcpyAsync(recs.data(), dev.ptr, static_cast<size_t>(n) * sizeof(ShapePrism), hipMemcpyDeviceToHost, main_q(b));
    if (ge == hipSuccess) ge = hipStreamSynchronize(main_q(b));
    dev.release();
    if (ge != hipSuccess) return hip_fail(b, ge, "halo_prismgen_team_kernel");
    for (uint32_t k = 0; k < n; k++) {   // same members, shorter rows: widen to the general record
      const ShapePrism& r = recs[k];
      ShapeDev& d = pool[k];
      std::memset(&d, 0, sizeof(d));
      d.face_cnt = r.face_cnt, d.tri_cnt = r.tri_cnt, d.slab_cnt = r.slab_cnt, d.single_cnt = r.single_cnt;
      std::memcpy(d.face, r.face, sizeof(r.face));
      std::memcpy(d.slab, r.slab, sizeof(r.slab));
      std::memcpy(d.tri_v, r.tri_v, sizeof(r.tri_v));
      std::memcpy(d.tri_na, r.tri_na, sizeof(r.tri_na));
      std::memcpy(d.tri_face, r.tri_face, sizeof(r.tri_face));
      std::memcpy(d.face_number, r.face_number, sizeof(r.face_number));
      std::memcpy(d.single, r.single, sizeof(r.single));
    }
  } else if (on_device) {
    HIPCHK(b, hipSetDevice(b->device));
    DevBuf<ShapeDev> dev;
    HIPCHK(b, dev.reserve(n));
    hipError_t ge = launch_shapegen(dev.ptr, false, n, b->seed, host::MakeRecipe(*crystal), first_index, main_q(b), b->opt.gen_serial != 0);
    if (ge == hipSuccess) ge = hipMemcpyAsync(pool.data(), dev.ptr, static_cast<size_t>(n) * sizeof(ShapeDev), hipMemcpyDeviceToHost, main_q(b));
    if (ge == hipSuccess) ge = hipStreamSynchronize(main_q(b));
    dev.release();
    if (ge != hipSuccess) return hip_fail(b, ge, "halo_shapegen_kernel");
  } else {
    for (uint32_t k = 0; k < n; k++) host::MakeShapeDev(b->seed, *crystal, first_index + k, pool[k]);
  }
  for (uint32_t k = 0; k < n; k++) host::FromShapeDev(pool[k], out[k]);
  return HALO_OK;
}

int halo_set_color(halo_handle_t b, const HaloColorSet* sets, int n_sets, const HaloColorClass* classes, int n_classes) {
  if (!b || n_sets < 0 || n_classes < 0 || (n_sets && !sets) || (n_classes && !classes)) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "halo_set_color inside a session");
  if (n_classes > HALO_COLOR_MAX_CLASSES) return fail(b, HALO_FATAL, "more than HALO_COLOR_MAX_CLASSES colour classes");
  for (int i = 0; i < n_sets; i++) {
    if (sets[i].term_count < 0 || sets[i].term_count > HALO_COLOR_MAX_TERMS) return fail(b, HALO_FATAL, "colour set term_count out of range");
    for (int k = 0; k < sets[i].term_count; k++)
      if (sets[i].terms[k].bit < 0 || sets[i].terms[k].bit > 63) return fail(b, HALO_FATAL, "colour bit outside 0..63");
  }
  const bool same = static_cast<size_t>(n_sets) == b->color_sets.size() && static_cast<size_t>(n_classes) == b->color_classes.size() &&
                    (n_sets == 0 || std::memcmp(b->color_sets.data(), sets, sizeof(HaloColorSet) * static_cast<size_t>(n_sets)) == 0) &&
                    (n_classes == 0 || std::memcmp(b->color_classes.data(), classes, sizeof(HaloColorClass) * static_cast<size_t>(n_classes)) == 0);
  if (same) return HALO_OK;   // (handed over again unchanged, as the Lumice glue does at every BeginSession: the table cache stays)
  b->color_sets.assign(sets, sets + n_sets);
  b->color_classes.assign(classes, classes + n_classes);
  drop_table_cache(b);
  return HALO_OK;
}

int halo_last_sample_counts(halo_handle_t b, uint64_t* crystal_samples, uint64_t* orientation_samples) {
  if (!b) return HALO_FATAL;
  if (crystal_samples) *crystal_samples = b->sess_crystal_samples;
  if (orientation_samples) *orientation_samples = b->sess_orient_samples;
  return HALO_OK;
}

int halo_last_route(halo_handle_t b, HaloRouteInfo* out) {
  if (!b || !out) return HALO_FATAL;
  *out = b->route;
  return HALO_OK;
}

int halo_direct_closes(halo_handle_t b, uint64_t* out) {
  if (!b || !out) return HALO_FATAL;
  *out = b->direct_closes;
  return HALO_OK;
}

int halo_tile_appends(halo_handle_t b, uint64_t* out) {
  if (!b || !out) return HALO_FATAL;
  *out = b->tile_appends;
  return HALO_OK;
}

int halo_tile_tickets(halo_handle_t b, uint64_t* out) {
  if (!b || !out) return HALO_FATAL;
  *out = b->tile_tickets;
  return HALO_OK;
}

int halo_last_root_profile(halo_handle_t b, uint32_t* out) {
  if (!b || !out) return HALO_FATAL;
  *out = b->route_root;
  return HALO_OK;
}

int halo_reduce_accumulator(halo_handle_t b, void* nccl_comm, int root, int this_rank) {
  if (!b || !nccl_comm) return HALO_FATAL;
  if (!b->acc || b->acc_w <= 0) return fail(b, HALO_FATAL, "reduce_accumulator before any session");
  // ncclReduce(sendbuff, recvbuff, count, ncclFloat32 = 7, ncclSum = 0, root, comm, stream) — rccl.h:550
  typedef int (*nccl_reduce_fn)(const void*, void*, size_t, int, int, int, void*, hipStream_t);
  static nccl_reduce_fn reduce = nullptr;   // looked up once, whichever GPU's thread gets here first (one thread per GPU is a supported use)
  static std::once_flag reduce_once;
  std::call_once(reduce_once, [] {
    void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (lib) reduce = reinterpret_cast<nccl_reduce_fn>(dlsym(lib, "ncclReduce"));
  });
  if (!reduce) return fail(b, HALO_UNAVAILABLE, "RCCL (librccl.so: ncclReduce) cannot be loaded");
  HIPCHK(b, hipSetDevice(b->device));
  int rc = fold_if_dirty(b);   // an unfinished session still owes its planes to the accumulator
  if (rc != HALO_OK) return rc;
  const size_t n = static_cast<size_t>(b->acc_w) * static_cast<size_t>(b->acc_h) * 3 + 4;
  if (n > b->acc_floats) return fail(b, HALO_FATAL, "reduce_accumulator: the bound accumulator is smaller than width*height*3+4 floats");
  const int nr = reduce(b->acc, b->acc, n, 7 /* ncclFloat32 */, 0 /* ncclSum */, root, nccl_comm, main_q(b));
  if (nr != 0) return fail(b, HALO_FATAL, "ncclReduce failed with code " + std::to_string(nr));
  if (this_rank != root) HIPCHK(b, hipMemsetAsync(b->acc, 0, n * sizeof(float), main_q(b)));   // drained, in stream order
  return HALO_OK;
}

int halo_collect_stats(halo_handle_t b, HaloLayerStats* out) {
  if (!b || !out) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  harvest_all(b);
  if (int rc = pull_tally(b)) return rc;
  add_stats(b->pending, b->layer_acc);
  b->layer_acc = HaloLayerStats{};
  *out = b->pending;
  b->pending = HaloLayerStats{};
  return HALO_OK;
}

int halo_collect_timing(halo_handle_t b, double* trace_ms, double* post_ms, uint64_t* launches) {
  if (!b) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = sync_all(b)) return rc;
  harvest_all(b);   // (adds the kernel times to the layer tallies as well: each ring slot is harvested once, whoever asks first)
  if (trace_ms) *trace_ms = b->time_trace_ms;
  if (post_ms) *post_ms = b->time_post_ms;
  if (launches) *launches = b->time_launches;
  b->time_trace_ms = b->time_post_ms = 0.0;
  b->time_launches = 0;
  return HALO_OK;
}

int halo_recombine(halo_handle_t b, int shuffle, uint64_t* continuation_count) {
  if (!b) return HALO_FATAL;
  if (!b->in_session) return fail(b, HALO_FATAL, "Recombine outside a session");
  // No data moves: the pools swap roles and the Feistel permutation (shuffle_cont_kernel, cu:1633-1657) is
  // applied as a gather index by the next layer's kernel.
  if (b->opt.cont_order) {
    // Canonical order: the sharded pool is sorted by (root, interaction) into the pool the layer just traced has read (free now: its kernels were
    // joined and waited for at the end of TraceLayer), as ONE region; the next layer appends to the sharded pool again.  Queued on the session's
    // stream behind every launch of the layer, no host wait; the next layer's mask clear and counter reset queue behind it.
    const int src = b->cont_out_slot, dst = src ^ 1;
    const uint64_t n_cont = b->cont_in_n;
    const uint64_t planes = b->color_classes.empty() ? 5 : 7;
    const uint64_t stride = std::max<uint64_t>((n_cont + 63) & ~63ull, 64);
    HIPCHK(b, hipSetDevice(b->device));
    if (int rc = reserve_idle(b, b->cont[dst], stride * planes)) return rc;
    if (n_cont > 0) {
      const uint64_t tiles = (b->cont_roots + 2047) / 2048;   // (halo_kernels.hip kScanTile)
      if (int rc = reserve_idle(b, b->cont_base, std::max<uint64_t>(b->cont_roots, 1))) return rc;
      if (int rc = reserve_idle(b, b->cont_tiles, std::max<uint64_t>(tiles, 1))) return rc;
      const hipError_t e = launch_cont_reorder(b->cont[src].ptr, b->cont_stride[src], b->cont_region[src], b->cont_cnt.ptr, b->cont_fill_max, b->cont_mask.ptr,
                                               static_cast<uint32_t>(b->cont_roots), b->cont_tiles.ptr, b->cont_base.ptr, b->cont[dst].ptr, static_cast<uint32_t>(stride),
                                               static_cast<uint32_t>(n_cont), static_cast<uint32_t>(planes), b->cont_err.ptr, main_q(b));
      if (e != hipSuccess) return hip_fail(b, e, "halo_cont_scatter_kernel launch");
      // the reorder's invariants, checked before any layer reads the pool: one 4-byte read behind the scatter (which the next layer's kernels
      // wait for in any case)
      uint32_t err = 0;
      HIPCHK(b, hipMemcpyAsync(&err, b->cont_err.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, main_q(b)));
      HIPCHK(b, hipStreamSynchronize(main_q(b)));
      if (err != 0u) return cont_order_fail(b, err);
    }
    b->cont_stride[dst] = static_cast<uint32_t>(stride);
    b->cont_region[dst] = static_cast<uint32_t>(stride);
    b->cont_seg[0] = 0;   // one region: every logical index lies in shard 0
    for (int sI = 1; sI <= kContShards; sI++) b->cont_seg[sI] = static_cast<uint32_t>(n_cont);
    b->cont_shuffle = shuffle ? 1 : 0;
    b->layer_idx++;
    if (continuation_count) *continuation_count = b->cont_in_n;
    return HALO_OK;
  }
  b->cont_out_slot ^= 1;
  b->cont_shuffle = shuffle ? 1 : 0;
  b->layer_idx++;
  if (continuation_count) *continuation_count = b->cont_in_n;
  return HALO_OK;
}

int halo_drain_exits(halo_handle_t b, HaloExitRecord* out, uint64_t cap, uint64_t* count) {
  if (!b) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  // Piecewise drain (trace_backend.hpp:430-448): a call takes at most `cap` records from the front and the rest stays
  // pending; *count = records copied by THIS call.  out == NULL reports how many are pending without consuming any.
  const uint64_t n = b->exits_pending;
  if (!out) {
    if (count) *count = n;
    return HALO_OK;
  }
  const uint64_t take = std::min(n, cap);
  if (count) *count = take;
  if (take) HIPCHK(b, hipMemcpy(out, b->exits.ptr, take * sizeof(HaloExitRecord), hipMemcpyDeviceToHost));
  const uint64_t left = n - take;
  if (left && take) {  // move the tail to the front (ranges may overlap: go through a scratch copy)
    DevBuf<HaloExitRecord> tmp;
    HIPCHK(b, tmp.reserve(left));
    HIPCHK(b, hipMemcpy(tmp.ptr, b->exits.ptr + take, left * sizeof(HaloExitRecord), hipMemcpyDeviceToDevice));
    HIPCHK(b, hipMemcpy(b->exits.ptr, tmp.ptr, left * sizeof(HaloExitRecord), hipMemcpyDeviceToDevice));
    tmp.release();
  }
  b->exits_pending = left;
  const uint32_t left32 = static_cast<uint32_t>(left);  // the device append counter continues behind the kept tail
  HIPCHK(b, hipMemcpyAsync(b->counters.ptr + kCntExit, &left32, sizeof(uint32_t), hipMemcpyHostToDevice, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  return HALO_OK;
}

int halo_flush(halo_handle_t b) {
  if (!b) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "halo_flush inside a session");
  HIPCHK(b, hipSetDevice(b->device));
  return fold_if_dirty(b);   // queued; the backend's stream waits for it, the host does not
}

int halo_sync(halo_handle_t b) {
  if (!b) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  // with option defer_fold a caller-bound accumulator is brought up to date HERE (and by every reader): the closing folds of the ended sessions
  if (b->opt.defer_fold && !b->in_session)
    if (int rc = fold_if_dirty(b)) return rc;
  return sync_all(b);
}

int halo_take_landed(halo_handle_t b, double* landed) {
  if (!b || !landed) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  {
    int rc = fold_if_dirty(b);
    if (rc != HALO_OK) return rc;
  }
  return take_landed_delta(b, landed);
}

int halo_peek_fixed(halo_handle_t b, int32_t plane, uint64_t* sums, uint64_t n_pix, uint32_t* frac_bits, uint64_t* landed, uint32_t* landed_frac_bits) {
  if (!b) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "halo_peek_fixed inside a session");
  if (!b->mono_dirty || !b->fix_planes || b->acc != b->acc_own.ptr)
    return fail(b, HALO_FATAL, "halo_peek_fixed: no fixed-point planes are pending (needs deterministic = 1, lazy_fold = 1 and the backend's own accumulator, after halo_end and before any reader)");
  if (plane < 0 || static_cast<uint32_t>(plane) >= b->plane_cnt) return fail(b, HALO_FATAL, "halo_peek_fixed: plane outside the session's planes");
  if (sums && n_pix != static_cast<uint64_t>(b->acc_w) * static_cast<uint64_t>(b->acc_h)) return fail(b, HALO_FATAL, "halo_peek_fixed: n_pix is not the session's width * height");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = sync_all(b)) return rc;
  if (sums) {
    const size_t slots = static_cast<size_t>(kMonoRows) << b->mono_s_log2;
    std::vector<unsigned long long> host(slots);
    HIPCHK(b, hipMemcpy(host.data(), b->fix.ptr + static_cast<size_t>(plane) * slots, slots * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (uint64_t pix = 0; pix < n_pix; pix++) sums[pix] = host[MonoSlot(static_cast<uint32_t>(pix), b->mono_s_log2)];   // pixel order: the slot hash undone
  }
  if (frac_bits) *frac_bits = b->fix_frac;
  if (landed) {   // what landed since the last taker, as the integer it is (nothing is taken)
    double now[kSumNum];
    unsigned long long fix_now = 0ull;
    if (int rc = read_tally(b, now, &fix_now)) return rc;
    *landed = fix_now - b->fix_landed_seen;
  }
  if (landed_frac_bits) *landed_frac_bits = b->fix_frac_landed;
  return HALO_OK;
}

int halo_set_shard(halo_handle_t b, uint32_t index, uint32_t count) {
  if (!b) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "halo_set_shard inside a session");
  if (count == 0u || index >= count) return fail(b, HALO_FATAL, "halo_set_shard: index " + std::to_string(index) + " outside count " + std::to_string(count) + " (needs count >= 1 and index < count)");
  if (count > 1u && b->opt.rank != 0) return fail(b, HALO_FATAL, "halo_set_shard count > 1: option rank is set (shards trace the one-rank run's rays: they share its counter range)");
  b->shard_index = index;
  b->shard_count = count;
  return HALO_OK;
}

// What halo_export_fixed and halo_import_fixed ask of the handle: its last session was a deterministic one, on the backend's own accumulator.
static int fixed_layout_check(HaloBackend* b, const char* who, uint64_t n_words) {
  if (b->in_session) return fail(b, HALO_FATAL, std::string(who) + " inside a session");
  if (!b->det_session || !b->fix.ptr || !b->acc || b->acc != b->acc_own.ptr)
    return fail(b, HALO_FATAL, std::string(who) + ": the handle's last session was not a deterministic one on the backend's own accumulator");
  const uint64_t want = static_cast<uint64_t>(b->plane_cnt) * static_cast<uint64_t>(b->acc_w) * static_cast<uint64_t>(b->acc_h) + 1u;
  if (n_words != want)
    return fail(b, HALO_FATAL, std::string(who) + ": n_words " + std::to_string(n_words) + " is not plane_cnt * width * height + 1 = " + std::to_string(want) + " of the handle's last session (image size or plane count differ)");
  return HALO_OK;
}

int halo_export_fixed(halo_handle_t b, void* dev_words, uint64_t n_words, uint32_t* plane_cnt, uint32_t* frac_bits, uint32_t* landed_frac_bits) {
  if (!b) return HALO_FATAL;
  if (!dev_words) return fail(b, HALO_FATAL, "halo_export_fixed: dev_words is NULL");
  if (b->in_session) return fail(b, HALO_FATAL, "halo_export_fixed inside a session");
  if (!b->mono_dirty || !b->fix_planes || b->acc != b->acc_own.ptr)
    return fail(b, HALO_FATAL, "halo_export_fixed: no fixed-point planes are pending (needs deterministic = 1, lazy_fold = 1 and the backend's own accumulator, after halo_end and before any reader)");
  if (int rc = fixed_layout_check(b, "halo_export_fixed", n_words)) return rc;
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // the copy runs on the backend's stream, behind everything that adds to the planes
  double now[kSumNum];
  unsigned long long fix_now = 0ull;
  if (int rc = read_tally(b, now, &fix_now)) return rc;   // (waits for the device)
  const uint32_t npix = static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h);
  hipError_t e = launch_export_fixed(b->fix.ptr, static_cast<unsigned long long*>(dev_words), npix, b->mono_s_log2, b->plane_cnt, fix_now - b->fix_landed_seen, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_export_fixed_kernel launch");
  HIPCHK(b, hipStreamSynchronize(main_q(b)));   // the words are the caller's from here on, whatever stream it reads them on
  b->fix_landed_seen = fix_now;   // taken: nothing is counted twice
  b->landed_own = false;
  // (landed_carry — landed weight converted to a double when F_landed changed — stays with the handle and goes to its next taker: on a shard it
  //  can only come from imported words, fix_prepare sees to that, so it is weight of the whole image on the handle that folds it)
  if (plane_cnt) *plane_cnt = b->plane_cnt;
  if (frac_bits) *frac_bits = b->fix_frac;
  if (landed_frac_bits) *landed_frac_bits = b->fix_frac_landed;
  b->fix_hits = 0;
  b->fix_planes = false;
  b->fix_imported = false;
  b->mono_dirty = false;
  return HALO_OK;
}

int halo_import_fixed(halo_handle_t b, const void* dev_words, uint64_t n_words, uint32_t plane_cnt, uint32_t frac_bits, uint32_t landed_frac_bits, uint64_t rays) {
  if (!b) return HALO_FATAL;
  if (!dev_words) return fail(b, HALO_FATAL, "halo_import_fixed: dev_words is NULL");
  if (b->mono_dirty && !b->fix_planes) return fail(b, HALO_FATAL, "halo_import_fixed: float planes are pending (fold them first: halo_flush)");
  if (b->det_session && plane_cnt != b->plane_cnt)
    return fail(b, HALO_FATAL, "halo_import_fixed: plane count " + std::to_string(plane_cnt) + " is not the " + std::to_string(b->plane_cnt) + " of the handle's last session");
  if (int rc = fixed_layout_check(b, "halo_import_fixed", n_words)) return rc;
  if (frac_bits != b->fix_frac) return fail(b, HALO_FATAL, "halo_import_fixed: frac_bits (F) " + std::to_string(frac_bits) + " is not the handle's " + std::to_string(b->fix_frac));
  if (landed_frac_bits != b->fix_frac_landed)
    return fail(b, HALO_FATAL, "halo_import_fixed: landed_frac_bits (F_landed) " + std::to_string(landed_frac_bits) + " is not the handle's " + std::to_string(b->fix_frac_landed));
  const uint64_t held = b->mono_dirty ? b->fix_hits : 0u;
  if (rays > kFixBudgetHits || held + rays > kFixBudgetHits)
    return fail(b, HALO_FATAL, "halo_import_fixed: " + std::to_string(held) + " + " + std::to_string(rays) + " rays would pass the budget of 2^30 rays of one unfolded plane set");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // behind everything that adds to (or folds) the planes; what follows waits for the main stream
  const uint32_t npix = static_cast<uint32_t>(b->acc_w) * static_cast<uint32_t>(b->acc_h);
  hipError_t e = launch_import_fixed(b->fix.ptr, static_cast<const unsigned long long*>(dev_words), npix, b->mono_s_log2, b->plane_cnt, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_import_fixed_kernel launch");
  unsigned long long landed = 0ull;
  HIPCHK(b, hipMemcpyAsync(&landed, static_cast<const unsigned long long*>(dev_words) + (n_words - 1u), sizeof(landed), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  b->fix_landed_seen -= landed;   // untaken landed integer = device tally - seen (modulo 2^64): the word joins it
  b->fix_imported = !b->mono_dirty || b->fix_imported;   // (own pending planes stay a part: still not to be folded)
  b->fix_hits = held + rays;
  b->fix_planes = true;
  b->mono_dirty = true;
  return HALO_OK;
}

int halo_readback_xyz64(halo_handle_t b, float* xyz, int width, int height, double* landed) {
  if (!b || !xyz) return HALO_FATAL;
  if (!b->acc || width != b->acc_w || height != b->acc_h) return fail(b, HALO_FATAL, "readback size does not match the session render");
  HIPCHK(b, hipSetDevice(b->device));
  {
    int rc = fold_if_dirty(b);
    if (rc != HALO_OK) return rc;
  }
  const size_t n = static_cast<size_t>(width) * height * 3;
  HIPCHK(b, hipMemcpyAsync(xyz, b->acc, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipMemsetAsync(b->acc, 0, (n + 4) * sizeof(float), main_q(b)));  // readback ZEROES the accumulator (cu:4832-4846)
  double l = 0.0;
  if (int rc = take_landed_delta(b, &l)) return rc;   // (syncs the stream: the image copy above is complete behind it)
  if (landed) *landed = l;
  return HALO_OK;
}

int halo_readback_xyz(halo_handle_t b, float* xyz, int width, int height, float* landed_weight) {
  double l = 0.0;
  int rc = halo_readback_xyz64(b, xyz, width, height, &l);
  if (rc == HALO_OK && landed_weight) *landed_weight += static_cast<float>(l);  // ADDS (trace_backend.hpp:461-469)
  return rc;
}


}  // extern "C"
