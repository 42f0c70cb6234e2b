// halo_state.h — what the host units of the library share (halo_backend.cpp: sessions, trace path, fixed-point import / export, shards;
// halo_consumer.cpp: the consumer stages): the owning device and pinned buffers, the stream markers, the backend's state and the helpers that more than
// one unit calls.  Internal: not installed, not part of include/halo_trace.h.
#ifndef HALO_STATE_H_
#define HALO_STATE_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdint>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "halo_device.h"
#include "halo_host.hpp"
#include "halo_launch.h"
#include "halo_options.h"

namespace halo {

static_assert(Options().ticket_min == kTicketMin && Options().ticket_max == kTicketMax && Options().ticket_div == kTicketDiv, "halo_options.h repeats the ticket defaults of halo_device.h");

// Device memory that belongs to whoever holds the DevBuf: freed with it, never copied.
template <typename T>
struct DevBuf {
  T* ptr = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t n) {
    if (n <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), std::max<size_t>(n, 1) * sizeof(T));
    if (e == hipSuccess) cap = n;
    return e;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
  void swap(DevBuf& o) {
    std::swap(ptr, o.ptr);
    std::swap(cap, o.cap);
  }
};
// A pinned host mirror (hipHostMalloc), owned the same way.
template <typename T>
struct PinnedBuf {
  T* ptr = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (ptr) (void)hipHostFree(ptr);
  }
  hipError_t alloc(size_t n) { return hipHostMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T), hipHostMallocDefault); }
};

// "The last work of kind X": an event recorded behind that work, and whether anything has been recorded on it yet (nothing: nobody need wait).
// (Several markers that fall on one point of one stream share one recorded event: mark_at names an event somebody has just recorded there — a ring
//  slot's — instead of recording the marker's own.  Should that event be recorded again before the marker is, the marker waits for the later point.)
struct Marker {
  hipEvent_t ev = nullptr;
  hipEvent_t at = nullptr;   // the event that carries the marker now: `ev`, or a shared one
  bool set = false;
  hipError_t mark(hipStream_t s) {
    const hipError_t e = hipEventRecord(ev, s);
    if (e == hipSuccess) at = ev, set = true;
    return e;
  }
  hipError_t mark_at(hipEvent_t shared) {
    at = shared, set = true;
    return hipSuccess;
  }
  hipError_t wait_on(hipStream_t s) const { return set ? hipStreamWaitEvent(s, at, 0) : hipSuccess; }
  void clear() { set = false; }
};

// The consumer stages' own state (halo_consumer.cpp; RenderConsumer, server/render.hpp): Neumaier running image + total landed intensity, and the
// device buffers each stage stages its results in.  (The class lanes themselves are written by trace sessions: BackendState::lanes.)
struct Consumer {
  DevBuf<float> sum, comp, xyz_out, stage;
  DevBuf<uint8_t> rgb;
  DevBuf<float> comp_rgb, lanes_stage;   // halo_consumer_composite's linear image, halo_consumer_load_lanes' staging
  DevBuf<uint32_t> comp_hist;            // radix-select histogram (2048 bins)
  // halo_consumer_auto_ev: the candidate values, and one block of words — the select's AevRecord, then the multi-block select's histograms
  DevBuf<float> aev_vals;
  DevBuf<uint32_t> aev_ws;
  DevBuf<uint32_t> stats_ws;             // halo_consumer_stats: the StatsRecord, then the multi-block form's histograms (its values go to aev_vals)
  // halo_consumer_view: the view's four outputs before they are copied back
  DevBuf<uint8_t> view_rgb;
  DevBuf<float> view_xyz, view_dir;
  DevBuf<int32_t> view_map;
  int w = 0, h = 0;
  double total_intensity = 0.0;
};

// Everything a handle holds.  (HaloBackend, the C ABI's opaque struct, is this and nothing else: the members live in the namespace of their types.)
struct BackendState {
  int device = 0;
  uint32_t seed = 1;
  std::string error;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  int cu_count = 256;

  Options opt;                 // every knob of halo_set_option (halo_options.h)
  // Two sets of the hit-log / tile-list buffers, taken in turn by the launches that alternate between the two trace streams (<= 2^21 rays):
  // the one of exactly 2^21 rays that logs may run beside a neighbour.  Launches that fill the chip keep set 0.
  DevBuf<HitRec> bin_list_s[2], bin_list2_s[2];   // one-level tile lists / coarse lists / log regions; tile lists of the two-level and log routes
  DevBuf<uint32_t> bin_cnt_s[2], bin_cnt2_s[2];
  int log_set = 0;                      // the set the next logged launch writes
  Marker set_free[2];                   // the passes that last read log set s (they may still be running)
  // Auxiliary stream (round 5): the closing folds are queued here, behind everything the other streams hold, and nobody waits for them until
  // somebody reads the image or adds to the planes again — a session's fold (20 us) runs under the next session's first kernels instead of
  // in front of them.  (Two engines side by side on one GPU had measured +10 .. 15 % over one, tools/two_engines_probe.py; what that was,
  // looked at inside one engine, is the small things between kernels — folds, resets, uploads, the tails — not the trace kernels or their
  // passes, which gain nothing from running under each other: see queue_passes.)
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool aux_pending = false;             // work has been queued on `aux` that the main stream has not waited for
  // Two trace streams: consecutive launches alternate between them, so that launch k+1's workgroups fill the CUs that launch k's last
  // workgroups leave idle (kernels of ONE stream run one after the other: the tail of every 1.8 ms trace kernel, and the whole of a
  // latency-bound small launch, went unshared).  Trace kernels of different launches have nothing to order between them: each logs to its own
  // buffer set or adds with atomics, tallies and continuation appends are atomic.  What they must follow is on the main stream (table
  // uploads) or the auxiliary one (a fold or per-tile pass before a launch that adds to the planes itself): waited for by events.
  hipStream_t cs[2] = {nullptr, nullptr};
  hipEvent_t ev_cs[2] = {nullptr, nullptr}, ev_main = nullptr, ev_aux = nullptr;
  bool cs_pending[2] = {false, false};
  int cs_next = 0;
  bool main_dirty[2] = {true, true};    // the main stream has been given work (main_q) since trace stream i last waited for it
  uint64_t aux_seq = 0, cs_seen_aux[2] = {0, 0};   // (a trace stream waits for the auxiliary stream only when that holds work it has not waited for yet)
  int twin_set = 0;                     // which half of the fp64 twin the open / next session's overflows go to (the other half may still be folding)
  uint32_t mono_s_log2 = 0;    // log2 of the columns per row of the plane (kMonoRows rows; see MonoSlot)
  // Direct close: a logged launch that is its whole session — one plane, one copy, nothing pending in the planes — has its per-tile
  // pass add coef x sum to the XYZ image itself (launch_log_route_close): no plane write, no fold on the auxiliary stream, no stream hop in front of
  // the next session's trace kernel.  The pass is a PLAIN read-modify-write of the image and of the twin's half, on the launch's trace stream: a later
  // launch on the other trace stream waits for it (close_done), readers and folds join the trace streams as they always do.
  uint64_t direct_closes = 0;  // launches that closed their session directly, ever (halo_direct_closes)
  Marker close_done;           // the direct close queued last, on trace stream close_ts
  int close_ts = 0;
  bool cnt2_clean[2] = {false, false};   // log set s: the tile-list counters are known to be zero (the closing pass zeroes what it consumed)
  // Per-tile append: a directly closing launch whose kernel has a kAccTileFinal twin appends its records to per-tile chunks of each
  // workgroup (halo_trace.inl log_hit_tile) and the closing pass reads the chunks (launch_tile_route_close): the split pass and its tile lists go.
  uint64_t tile_appends = 0;   // launches that took the route, ever (halo_tile_appends)
  DevBuf<HitRec> tile_chunk_s[2];   // chunk[tile][workgroup][cap], one set per log set
  DevBuf<uint32_t> tile_cnt_s[2];   // cnt[tile][workgroup]
  // Wave tickets: a per-tile-append launch runs ONE resident round of workgroups whose waves draw their passes of the ray loop from a
  // counter (halo_device.h TicketSize, halo_trace.inl) — no static round's tail, and chunks four times as long for the closing pass.
  uint64_t tile_tickets = 0;   // launches that took tickets, ever (halo_tile_tickets)
  bool ticket_zeroed = false;  // the counters below exist and the one-time memset behind their reserve has completed
  DevBuf<uint32_t> ticket_cnt; // kTicketGroups counters per log set, kTicketStride words apart: zeroed when reserved, and by every closing pass after
  HaloRouteInfo route{};       // kernels that served the current / last session (halo_last_route)
  uint32_t route_root = 0;     // ... and the root profiles among them (halo_last_root_profile): bit kRootProfile* - 1

  // monotone ray counters: seeded once, never reset per session (cuda_trace_backend.cu:3724-3741)
  uint64_t gen_count = 0, gate_count = 0, transit_count = 0, shape_count = 0;
  double sess_max_w = 1.0;     // largest initial ray weight of the open session (wavelength-pool spd weights)

  // session
  bool in_session = false;
  HaloScene scene{};
  HaloRender render{};
  HaloWl wl{};
  ProjDev proj{};
  int layer_idx = 0;
  double carry[HALO_MAX_LAYERS][HALO_MAX_ENTRIES] = {};

  // device state
  DevBuf<float> acc_own;       // W*H*3 + 4
  float* acc = nullptr;        // bound accumulator (own or external)
  uint64_t acc_floats = 0;
  int acc_w = 0, acc_h = 0;    // image the bound accumulator (own or external) currently holds
  int own_w = 0, own_h = 0;    // image the OWNED buffer was last sized and zeroed for
  std::vector<HaloFilter> filters;  // table referenced by HaloEntry::filter_id
  std::vector<HaloColorSet> color_sets;      // table referenced by HaloEntry::color_id
  std::vector<HaloColorClass> color_classes; // raypath-colour classes (Y lanes)
  DevBuf<double> lanes;                      // class_count x W x H, accumulated in fp64 (handed out as float)
  int lanes_w = 0, lanes_h = 0;
  DevBuf<FilterDev> filter_dev;
  std::unique_ptr<FastTables> fast_scratch;  // host staging of a dispatch's fast filter tables (20 KB: not on the stack)
  DevBuf<float> mono;          // accumulation planes (see MonoSlot): plane_cnt x plane_copies x (kMonoRows << s_log2) floats
  DevBuf<double> ovf;          // fp64 twin of the planes' copy 0, laid out [plane][slot] (TwinOffset): where full log regions / tile lists overflow to
  DevBuf<uint32_t> ovf_flag;   // one word: something was written to the twin since the last fold
  bool mono_session = false;   // kernel variant: true = one scalar per hit (plane 0 or plane wl_idx), false = X,Y,Z planes
  bool mono_by_wl = false;     // illuminant session with one plane per wavelength-pool entry
  bool xyz_log = false;        // illuminant session on X, Y, Z planes whose big production launches go through the hit log
  bool mono_dirty = false;
  // Two plane SETS for sessions whose every launch goes through the hit log onto one scalar plane (round 6): a fold reads and zeroes the set its
  // session added to while the passes of the session after it add to the other set — on a discrete spectrum of short sessions the passes of
  // session k + 1 otherwise wait for the fold of session k, which waits for the passes of session k: one serial chain (bench.py --config 4d).
  bool mono_two = false;
  int mono_set = 0;
  size_t mono_half = 0;                                   // floats per set
  Marker set_folded[2];                                   // the fold that last zeroed the set
  uint32_t plane_cnt = 1, plane_copies = 8;
  std::vector<std::array<float, 3>> plane_coef;  // fold coefficients of the pending planes
  Consumer cons;               // the consumer stages' state (halo_consumer.cpp)
  bool had_session = false;    // `render` holds a session's render (halo_consumer_view's default source)
  DevBuf<double> tally;        // kTallyLines x kTallyStride doubles, [kSum*] per line: CUMULATIVE tallies of every kernel this backend ever launched
  PinnedBuf<double> tally_host;       // one snapshot of `tally`
  double tally_seen[kSumNum] = {};    // cumulative values already handed on: [kSumLanded] to a readback / take_landed, the rest to the layer statistics
  bool tally_unread = false;
  double time_trace_ms = 0.0, time_post_ms = 0.0;   // halo_collect_timing: the last layers' trace kernels' own spans and their passes', since the last call
  uint64_t time_launches = 0;          // a dispatch has been queued since the statistics were last pulled
  DevBuf<uint32_t> counters;   // kCntNum
  // dispatch ring: device slots, pinned host mirrors, pinned tally read-back, per-slot events
  static constexpr int kRing = 32;
  DevBuf<DispatchSlot> ring_dev;
  PinnedBuf<DispatchSlot> ring_host;
  hipEvent_t ring_ev0[kRing] = {}, ring_ev1[kRing] = {}, ring_ev2[kRing] = {}, ring_ev3[kRing] = {}, ring_done[kRing] = {};   // ev0..ev1 the trace kernel (main stream), ev2..ev3 its passes (post stream)
  // (the events that CARRY a slot's "passes begin" and "slot done" for its current launch: ring_ev2 / ring_done themselves, or — option
  //  lean_events — the neighbour recorded at the same point of the same stream: ring_ev1 where no wait lies between it and the passes, ring_ev3
  //  behind a direct close)
  hipEvent_t ring_t2[kRing] = {}, ring_fin[kRing] = {};
  bool ring_posts[kRing] = {};
  bool ring_final[kRing] = {};         // the slot's launch belongs to its session's last layer (halo_collect_timing counts those)
  bool ring_busy[kRing] = {};
  uint64_t ring_use[kRing] = {};       // how many launches have taken the slot (TableCacheEntry::read_use)
  int ring_next = 0;
  // Table cache (round 5): the dispatch-constant tables of a deterministic crystal entry (latitude LUT, wavelength pool, shape, entry-pick
  // tables, filter / colour tables) stay on the device from one dispatch to the next while scene, wavelength, filters, colour and options
  // are what they were — a server that sends one wavelength's rays as many equal small sessions (and every chunk of a long layer) then
  // pays neither the host-side builds (closed-form geometry, LUT, predicate tables) nor the 25-49 KB copy per dispatch.
  struct TableCacheEntry {
    bool valid = false;
    int mode = 0;
    bool use_filter = false, use_color = false, entry_fast = false, hex_regular = false, has_fast = false;
    // Two device slots per entry, taken in turn by the uploads: the kernels of the session before (queued on a trace stream, async) may still be
    // staging their tables out of the slot they were given.  An upload waits (on the stream, not the host) for the last kernel that read ITS
    // slot — two table sets back, as good as always finished — so consecutive sessions of different wavelengths still overlap.
    int cur = 0;
    // the slot's last reader = the dispatch-ring slot of the last launch that was given it (its ring_done event is recorded anyway: no
    // event of the cache's own, one HIP call less per small session) and that ring slot's use count then: a ring slot that has been taken
    // again since was harvested first, i.e. that launch is over
    int read_ring[2] = {-1, -1};
    uint64_t read_use[2] = {0, 0};
  };
  TableCacheEntry tcache[HALO_MAX_LAYERS][HALO_MAX_ENTRIES];
  DevBuf<DispatchSlot> tcache_dev;     // HALO_MAX_LAYERS x HALO_MAX_ENTRIES x 2 slots, reserved on first use
  HaloScene tcache_scene{};            // what the valid entries were built for
  HaloWl tcache_wl{};
  std::vector<HaloWl> tcache_spec;   // ... and the entry table of a spectrum session (empty otherwise)
  uint32_t spec_count = 0;           // entries of the open spectrum session (halo_begin_spectrum with count >= 2), 0 = not one
  HaloLayerStats pending{};    // harvested tallies not yet handed to the caller (async mode)
  HaloLayerStats layer_acc{};  // tallies of the layer being traced
  std::vector<WlEntryDev> wl_pool_host;
  uint32_t wl_pool_size = 0;
  struct LutKey { int32_t type; float center, spread; host::LatLut lut; };
  std::vector<LutKey> lut_cache;
  DevBuf<ShapeDev> shapes_s[2];   // sampled-crystal pools: launch k+1's generator must not overwrite what launch k still traces
  Marker shapes_free[2];                               // the trace kernel that last read the pool
  hipEvent_t ev_gen = nullptr;                         // the generator of a chip-filling launch, queued on trace stream 1 (see gen_ahead)
  int shapes_next = 0;
  // Plane ownership between the two trace streams.  The per-tile sums of a logged (or two-level binned) launch end in PLAIN read-modify-writes of
  // the planes; everything else that adds to them uses atomics.  So (1) a launch's sums wait for what the OTHER trace stream held when the launch
  // was queued (ev_gate), and (2) a later launch on the other stream whose trace kernel adds to the planes itself waits for those sums (rmw).
  // Logged trace kernels touch no plane (their overflow goes to the fp64 twin), so they run beside a neighbour's passes freely.
  hipEvent_t ev_gate = nullptr;
  Marker rmw[2];                  // the per-tile sums last queued on trace stream i
  // Deterministic sessions (option "deterministic"): every accumulating launch runs a kAccFixed kernel — 64-bit fixed-point sums from the first add
  // to the fold, so the plane sums depend on the set of rays alone.  The planes are a buffer of their own, [plane][slot], one copy,
  // all-zero between folds like the float planes; F and the budget belong to the PENDING plane set (they may span sessions under lazy_fold).
  bool det_session = false;                  // the open / last session is a deterministic one
  bool fix_planes = false;                   // the pending planes (mono_dirty) are the fixed-point ones
  DevBuf<unsigned long long> fix;
  uint32_t fix_frac = 32, fix_frac_landed = 32;   // F of the pending plane set; F_L of the landed integer (tally slot kSumFixLanded)
  uint64_t fix_hits = 0;                     // rays traced into the pending plane set since its last fold (<= kFixBudgetHits)
  unsigned long long fix_landed_seen = 0;    // the cumulative landed integer already handed on (like tally_seen)
  double landed_carry = 0.0;                 // landed integers converted when F_L had to change before anybody took them
  // Shards (halo_set_shard): the handle plans every session whole — partition, launches, counters — and launches only the part of each
  // planned launch that lies in its slice of the launch's crystal entry (shard_slice).  (0, 1), the default, is the whole of everything.
  uint32_t shard_index = 0, shard_count = 1;
  bool fix_imported = false;                 // the pending fixed-point planes came through halo_import_fixed: a whole image, which a sharded handle may fold
  bool landed_own = false;                   // count > 1: the untaken landed integer holds weight of this shard's own launches (a part, until it is exported)
  DevBuf<float> cont[2];       // SoA continuation pools, 5 planes
  uint32_t cont_stride[2] = {0, 0};
  uint32_t cont_region[2] = {0, 0};          // slots per shard region
  DevBuf<uint32_t> cont_cnt;                 // kContShards * kContCntStride
  uint32_t cont_seg[kContShards + 4] = {};   // prefix of the input pool's shard fill counts
  int cont_out_slot = 0;
  uint64_t cont_in_n = 0;
  int cont_shuffle = 1;
  DevBuf<uint32_t> cont_mask;                // cont_order = 1: per root of the layer being traced, the 128-bit mask of its continued exit seqs
  DevBuf<uint32_t> cont_err;                 // ... the session's error word (kContErr*: appends, scan and scatter), read at the end of every layer
  DevBuf<uint32_t> cont_base;                // ... each root's first canonical slot, and the scan's tile sums
  DevBuf<uint32_t> cont_tiles;
  uint32_t cont_fill_max = 0;                // fullest shard region of the last non-final layer (the scatter's grid)
  uint64_t cont_roots = 0;                   // roots of the last non-final layer
  DevBuf<HaloExitRecord> exits;
  uint64_t exits_pending = 0;
  DevBuf<float> host_f;        // injected rays: d | p | w
  DevBuf<uint32_t> host_u;
  uint64_t sess_crystal_samples = 0, sess_orient_samples = 0;  // this session's stochastic draws (halo_last_sample_counts)
  // every event made without timing: the one-shot ones, the joins' and the markers' (created in halo_create, destroyed in halo_destroy)
  std::vector<hipEvent_t*> untimed_events() {
    return {&ev_cs[0], &ev_cs[1], &ev_main, &ev_aux, &ev_fork, &ev_join, &ev_gen, &ev_gate, &set_free[0].ev, &set_free[1].ev, &shapes_free[0].ev,
            &shapes_free[1].ev, &rmw[0].ev, &rmw[1].ev, &set_folded[0].ev, &set_folded[1].ev, &close_done.ev};
  }
};

}  // namespace halo

struct HaloBackend : halo::BackendState {};

namespace halo {

// ---- helpers of more than one unit (defined in halo_backend.cpp) ----
int fail(HaloBackend* b, int code, const std::string& msg);
int hip_fail(HaloBackend* b, hipError_t e, const char* what);
#define HIPCHK(b, call)                                   \
  do {                                                    \
    hipError_t e__ = (call);                              \
    if (e__ != hipSuccess) return hip_fail(b, e__, #call); \
  } while (0)

// The main stream, for whoever queues work on it (or waits for it): the trace streams have not seen that work yet (next_trace_stream).
inline hipStream_t main_q(HaloBackend* b) {
  b->main_dirty[0] = b->main_dirty[1] = true;
  return b->stream;
}
// What the main stream is given from here on runs behind everything queued on the auxiliary and the trace streams (no host wait).
int join_aux(HaloBackend* b);
// Host waits for all streams.
int sync_all(HaloBackend* b);
// DevBuf::reserve frees the old allocation when it grows: nothing on either stream may still be using it.
template <typename T>
int reserve_idle(HaloBackend* b, DevBuf<T>& buf, size_t n, hipError_t* err = nullptr) {
  if (n > buf.cap) {
    if (int rc = sync_all(b)) return rc;
  }
  const hipError_t e = buf.reserve(n);
  if (err) {
    *err = e;
    return HALO_OK;
  }
  HIPCHK(b, e);
  return HALO_OK;
}
// The closing fold of the pending planes, with the main stream waiting for it: for readers of the image and for whoever hands the image on.
int fold_if_dirty(HaloBackend* b);
// The landed weight since the last taker (readback, take_landed, consumer fold).
int take_landed_delta(HaloBackend* b, double* landed);
void drop_table_cache(HaloBackend* b);

}  // namespace halo

#endif
