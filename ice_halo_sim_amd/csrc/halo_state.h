// halo_state.h — what the host units of the library share (halo_backend.cpp: sessions, trace path, fixed-point import / export, shards;
// halo_consumer.cpp: the consumer stages): the owning device and pinned buffers, the stream order over the real HIP calls (halo_order.h), the backend's
// state and the helpers that more than one unit calls.  Internal: not installed, not part of include/halo_trace.h.
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
#include "halo_order.h"

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

// The stream order (halo_order.h) over the real calls: streams that do not join the null stream, events timed (the ring's spans) or not.
struct HipOrderApi {
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  using Error = hipError_t;
  static constexpr Error kOk = hipSuccess;
  static Error record(Event e, Stream s) { return hipEventRecord(e, s); }
  static Error wait(Stream s, Event e) { return hipStreamWaitEvent(s, e, 0); }
  static Error sync(Stream s) { return hipStreamSynchronize(s); }
  static Error create_stream(Stream* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
  static Error destroy_stream(Stream s) { return hipStreamDestroy(s); }
  static Error create_event(Event* e, bool timed) { return timed ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming); }
  static Error destroy_event(Event e) { return hipEventDestroy(e); }
};
using Order = StreamOrder<HipOrderApi>;

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
  DevBuf<float> view_xyz, view_dir, view_tap;   // (view_tap: halo_consumer_view_filtered's fifth)
  DevBuf<int32_t> view_map;
  // halo_consumer_view_composite: the source-sized composite its gather reads (never copied back); halo_consumer_view_lanes: the class planes of the view
  DevBuf<uint8_t> view_comp_src;
  DevBuf<float> view_lanes;
  DevBuf<float> view_sky, view_val;   // halo_consumer_view_overlay: the sky coordinates and the value after the last layer
  int w = 0, h = 0;
  double total_intensity = 0.0;
};

// Everything a handle holds.  (HaloBackend, the C ABI's opaque struct, is this and nothing else: the members live in the namespace of their types.)
struct BackendState {
  int device = 0;
  uint32_t seed = 1;
  std::string error;
  int cu_count = 256;

  Options opt;                 // every knob of halo_set_option (halo_options.h)
  Order ord{&opt};             // the streams, every event that orders them, the markers and the dispatch ring (halo_order.h)
  // Two sets of the hit-log / tile-list buffers, taken in turn by the launches that alternate between the two trace streams (<= 2^21 rays):
  // the one of exactly 2^21 rays that logs may run beside a neighbour.  Launches that fill the chip keep set 0.
  DevBuf<HitRec> bin_list_s[2], bin_list2_s[2];   // one-level tile lists / coarse lists / log regions; tile lists of the two-level and log routes
  DevBuf<uint32_t> bin_cnt_s[2], bin_cnt2_s[2];
  int log_set = 0;                      // the set the next logged launch writes
  int twin_set = 0;                     // which half of the fp64 twin the open / next session's overflows go to (the other half may still be folding)
  uint32_t mono_s_log2 = 0;    // log2 of the columns per row of the plane (kMonoRows rows; see MonoSlot)
  // Direct close: a logged launch that is its whole session — one plane, one copy, nothing pending in the planes — has its per-tile
  // pass add coef x sum to the XYZ image itself (launch_log_route_close): no plane write, no fold on the auxiliary stream, no stream hop in front of
  // the next session's trace kernel.  (What a later launch on the other trace stream owes such a pass: Order::close_done.)
  uint64_t direct_closes = 0;  // launches that closed their session directly, ever (halo_direct_closes)
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
  // dispatch ring (Order::ring holds each slot's events and use count): device slots and their pinned host mirrors
  DevBuf<DispatchSlot> slots_dev;
  PinnedBuf<DispatchSlot> slots_host;
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
    // the slot's last reader = the dispatch-ring slot of the last launch that was given it (its slot-done event is recorded anyway: no
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
  int shapes_next = 0;
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
inline hipStream_t main_q(HaloBackend* b) { return b->ord.main_q(); }
// What the main stream is given from here on runs behind everything queued on the auxiliary and the trace streams (no host wait).
inline int join_aux(HaloBackend* b) {
  HIPCHK(b, b->ord.join());
  return HALO_OK;
}
// Host waits for all streams.
inline int sync_all(HaloBackend* b) {
  HIPCHK(b, b->ord.sync_all());
  return HALO_OK;
}
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
