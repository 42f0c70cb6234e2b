// halo_options.h — the knobs of halo_set_option as data: the values with their defaults (Options), one table row per key (kOptionTable) and the
// rule that judges a set (set_option) — refused, unchanged, or a change with the effects the backend must perform.  Standard library only, no HIP:
// tests/cpp/options_main.cpp compiles this header alone and runs every rule on the host.
#ifndef HALO_OPTIONS_H_
#define HALO_OPTIONS_H_

#include <cstdint>
#include <string>
#include <utility>

namespace halo {

struct Options {
  int capture = 0;             // "capture_exits"
  uint32_t geom_clock = 32;    // simulator.hpp:144 (rays per sampled shape)
  uint64_t chunk = 1ull << 28;         // rays per launch: configs[2]'s 237 M continuations per wavelength run 3.8 % faster as one launch than as four
  uint64_t stoch_chunk = 0;            // rays per dispatch with device-generated crystal pools (0 = by record size, see chunk_of)
  uint32_t bin_l1 = 128u;              // coarse lists of the two-level binned route (measured: 512 -> 128 lists 6 % faster, 64 slower)
  int aggregate = 1;
  int mono_enabled = 1;        // "mono"
  int bin = -1;                // binned accumulation: -1 auto (discrete session, full-sky render, launch >= 4 Mi rays), 0 off, 1 on
  int lean_events = 1;         // 1 = one recorded event where several markers fall on one point of a stream, no hop from a main stream
                               // that holds nothing new (queue_passes, next_trace_stream); 0 = every marker its own record, every launch the hop
  int overlap = 1;             // 0 queues the passes and folds on the main stream (round 4 behaviour)
  int defer_fold = 0;          // 1 = halo_end leaves the fold pending even when the accumulator is the caller's memory; the caller asks for
                               // it (halo_sync, or any reader) before it looks at its memory
  int lambda_planes = -1;      // illuminant sessions: -1 auto (by batch size), 0 never, 1 always one plane per pool entry
  int mono_copies = 8;         // power of two; copy = blockIdx & (copies-1)
  int blocks_per_cu = 24;      // cap on workgroups per CU of a launch's STATIC ray loop (five or six resident: several rounds even out the tail; a ticketed
                               // launch — tile_ticket — runs one resident round instead and evens the tail out wave by wave)
  int host_shapes = 0;         // 1: stochastic shape pools are built on the host and uploaded (A/B and test path)
  int gen_serial = 0;          // 1: pyramids are generated one thread per crystal (the serial builder) instead of one team of 32 lanes
  int small_blocks_per_cu = 0; // experiment knob: workgroups per CU that a small launch may spread over (0 = five, see blocks_of)
  int blocks_cap = 0;          // experiment knob: absolute cap on the workgroups of one launch (0 = none)
  int lazy_fold = 1;           // the closing fold of a session waits for the first READER of the image (or a session with other planes) when the accumulator is the backend's own
  int hit_log = -1;            // hit-log accumulation of cache misses: -1 auto (one-plane sessions, launches >= 2 Mi rays), 0 off, 1 on
  uint32_t hit_log_cap = 0;    // test knob: records per log region (0 = sized from the launch); the tile lists then get half their even share
  int hex_fast = 1;            // 1: regular hexagonal prisms of one-shape dispatches run the literal-normal next-face search
  int entry_fast = 1;          // 1: full prisms of one-shape dispatches take the slab-wise entry pick (EntryFastDev)
  int filter_fast = 1;         // 1: filtered / colour-tagged dispatches with max_hits <= 16 run the production-shaped kernels (FastTables); 0: the generic ones
  int async = 0;               // 1: final-layer dispatches are queued without a host sync; stats via halo_collect_stats
  uint32_t shuffle_chunk_log2 = 5;   // "shuffle_chunk": Recombine's shuffle moves chunks of 2^k pool entries (k = 0: per ray, like the reference)
  int spec_root = 1;           // A/B knob: 1 = last-layer plain hit-log launches over a regular prism whose root generation matches a root profile
                               // (halo_trace.inl kRoot*) run the instantiation that has it as constants; 0 = always the generic root generation
  int close_direct = -1;       // direct close: -1 auto (launches that fill the chip), 0 never, 1 wherever eligible
  int tile_append = -1;        // per-tile append: -1 auto (launches that fill the chip), 0 never, 1 wherever eligible
  int tile_ticket = -2;        // wave tickets: -2 auto (as -1, and the launch's static grid is more than one resident round), -1 auto (launches
                               // that take the append by tile_append's auto rule), 0 never, 1 every launch that appends per tile
  uint32_t ticket_min = 4u, ticket_max = 64u, ticket_div = 2u;   // experiment knobs, unsupported (defaults: halo_device.h kTicketMin / Max / Div): the sweep of
                                                                 // profiles/wave_tickets_ab.txt, and the tests' way to guided tickets on launches of a few milliseconds' worth
  int aev_agg_hist = 0;        // "auto_ev_hist": 1 = wave-aggregated adds in the histogram passes (measured slower: DESIGN 3.5, tools/auto_ev_cost.py)
  int aev_select = -1;         // "auto_ev_select": -1 by size (kAevSmallMax), 0 the multi-block select, 1 the one-workgroup select
  int stats_select = -1;       // -1 by size (kStatsSmallMax), 0 the multi-block form, 1 one workgroup
  int table_cache = 1;         // 0 uploads the tables with every dispatch (round 4 behaviour)
  int log_tiles_log2 = 7;      // experiment knob: the scalar hit-log route cuts a plane into up to 2^this tiles (<= 8)
  int alt_log2 = 25;           // experiment knob: launches of up to 2^alt_log2 rays alternate between the two trace streams
  int rehit_strategy = 1;      // 1 [default] the reference's CUDA next-face strategy (the child that leaves through the face it stands on is emitted where it is);
                               // 0 its legacy CPU strategy (that child is propagated over all faces with the relaxed accept threshold, optics.cpp:116-155 —
                               // SURVEY's stated ground truth): every launch then takes the generic kernels, which carry the re-hit test
  int pool_entry_fast = 1;     // A/B knob: prism pools under the hit log pick a sampled full prism's entry face slab by slab; 0 = the walk over its fan triangles
  int gen_ahead = 0;           // experiment knob: 1 queues the generator of a chip-filling launch on trace stream 1, beside the previous launch's kernels
  int deterministic = 0;       // 1 = every accumulating launch runs a kAccFixed kernel; not inside a session
  int cont_order = 0;          // 0 [default] continuations in append order; 1 canonical (root, interaction) order (Recombine sorts the pool)
  uint64_t rank = 0;           // what "rank" was last set to (0 again after "ray_base"): not to be combined with shards
};

// How a raw int64 becomes the stored value (lo / hi / note of the row are the rule's parameters).
enum OptRule : uint8_t {
  kOptBool,        // v ? 1 : 0
  kOptTri,         // -1 / 0 / 1 by sign
  kOptTicket,      // tile_ticket: below -1 is -2, else as kOptTri
  kOptInt,         // as given
  kOptClamp,       // into [lo, hi]
  kOptPositiveOr,  // v > 0 ? v : lo (non-positive means the default)
  kOptZeroOne,     // exactly 0 or 1, else refused: "<key> must be <note>"
  kOptPow2,        // a power of two in [lo, hi], else refused
  kOptPow2Log2,    // ... stored as its log2
  kOptChunk,       // non-positive means 2^28; never above the caller's ceiling (the kernels' grid-stride index is 32-bit)
  kOptCopies,      // mono_copies: rounded up to a power of two in [1, 64]
  kOptRank,        // rank: counters to v << 40; not with shards
  kOptRayBase,     // ray_base: counters to v, rank back to 0
  kOptSeed,        // seed: 0 means 1
};
enum : uint32_t { kOptInSession = 1u, kOptAlways = 2u, kOptSyncFirst = 4u };   // row flags: refused inside a session; never "unchanged"; sync_all before the value changes
// What the backend performs before it commits a set (OptionSet::effects).
enum : uint32_t { kFxDropCache = 1u, kFxSync = 2u, kFxFoldPlanes = 4u, kFxReleasePlanes = 8u, kFxCounters = 16u, kFxSeed = 32u };

// The member of Options a row writes (none: the seed is state of the backend).
struct OptField {
  int Options::*i = nullptr;
  uint32_t Options::*u = nullptr;
  uint64_t Options::*q = nullptr;
  constexpr OptField() {}
  constexpr OptField(int Options::*p) : i(p) {}
  constexpr OptField(uint32_t Options::*p) : u(p) {}
  constexpr OptField(uint64_t Options::*p) : q(p) {}
  int64_t get(const Options& o) const { return i ? static_cast<int64_t>(o.*i) : u ? static_cast<int64_t>(o.*u) : q ? static_cast<int64_t>(o.*q) : 0; }
  // v as the member will hold it: a raw value beyond the member's range wraps as the cast always did
  int64_t fit(int64_t v) const { return i ? static_cast<int64_t>(static_cast<int>(v)) : u ? static_cast<int64_t>(static_cast<uint32_t>(v)) : v; }
  void set(Options& o, int64_t v) const {
    if (i) o.*i = static_cast<int>(v);
    else if (u) o.*u = static_cast<uint32_t>(v);
    else if (q) o.*q = static_cast<uint64_t>(v);
  }
};
struct OptionRow {
  const char* key;
  OptField field;
  OptRule rule;
  uint32_t flags;
  int64_t lo, hi;
  const char* note;
};
constexpr int64_t kOptNoCap = INT64_MAX;
constexpr OptionRow kOptionTable[] = {
    // the session's plane layout (privatised copies, hit-log eligibility) was decided at halo_begin from capture_exits and filter_fast: changing
    // them with a session open would send direct atomics to a layout made for another route
    {"capture_exits", &Options::capture, kOptBool, kOptInSession, 0, 0, nullptr},
    {"geom_clock", &Options::geom_clock, kOptPositiveOr, 0, 32, 0, nullptr},
    {"chunk", &Options::chunk, kOptChunk, 0, 0, 0, nullptr},
    {"bin_l1", &Options::bin_l1, kOptPow2, 0, 8, 512, nullptr},   // the kernels index the coarse lists with `& (lists - 1)`
    {"stoch_chunk", &Options::stoch_chunk, kOptPositiveOr, 0, 0, 0, nullptr},
    {"aggregate", &Options::aggregate, kOptInt, 0, 0, 0, nullptr},
    {"mono", &Options::mono_enabled, kOptBool, 0, 0, 0, nullptr},
    {"async", &Options::async, kOptBool, 0, 0, 0, nullptr},
    {"lambda_planes", &Options::lambda_planes, kOptInt, 0, 0, 0, nullptr},
    {"bin", &Options::bin, kOptInt, 0, 0, 0, nullptr},
    {"host_shapes", &Options::host_shapes, kOptBool, 0, 0, 0, nullptr},
    {"entry_fast", &Options::entry_fast, kOptBool, 0, 0, 0, nullptr},
    {"hex_fast", &Options::hex_fast, kOptBool, 0, 0, 0, nullptr},
    {"filter_fast", &Options::filter_fast, kOptBool, kOptInSession, 0, 0, nullptr},
    {"spec_root", &Options::spec_root, kOptBool, 0, 0, 0, nullptr},
    {"hit_log", &Options::hit_log, kOptInt, 0, 0, 0, nullptr},
    {"hit_log_cap", &Options::hit_log_cap, kOptClamp, 0, 0, kOptNoCap, nullptr},
    {"gen_serial", &Options::gen_serial, kOptBool, 0, 0, 0, nullptr},
    {"shuffle_chunk", &Options::shuffle_chunk_log2, kOptPow2Log2, 0, 1, 64, nullptr},
    {"lazy_fold", &Options::lazy_fold, kOptBool, 0, 0, 0, nullptr},
    {"table_cache", &Options::table_cache, kOptBool, 0, 0, 0, nullptr},
    {"overlap", &Options::overlap, kOptBool, kOptSyncFirst, 0, 0, nullptr},
    {"defer_fold", &Options::defer_fold, kOptBool, 0, 0, 0, nullptr},
    {"auto_ev_hist", &Options::aev_agg_hist, kOptBool, 0, 0, 0, nullptr},
    {"auto_ev_select", &Options::aev_select, kOptTri, 0, 0, 0, nullptr},
    {"stats_select", &Options::stats_select, kOptTri, 0, 0, 0, nullptr},
    {"gen_ahead", &Options::gen_ahead, kOptBool, 0, 0, 0, nullptr},
    {"close_direct", &Options::close_direct, kOptTri, 0, 0, 0, nullptr},
    {"lean_events", &Options::lean_events, kOptBool, 0, 0, 0, nullptr},
    {"tile_append", &Options::tile_append, kOptTri, 0, 0, 0, nullptr},
    {"tile_ticket", &Options::tile_ticket, kOptTicket, 0, 0, 0, nullptr},
    {"ticket_min", &Options::ticket_min, kOptClamp, 0, 1, 1024, nullptr},
    {"ticket_max", &Options::ticket_max, kOptClamp, 0, 1, 1024, nullptr},
    {"ticket_div", &Options::ticket_div, kOptClamp, 0, 1, 64, nullptr},
    {"pool_entry_fast", &Options::pool_entry_fast, kOptBool, 0, 0, 0, nullptr},
    {"rehit_strategy", &Options::rehit_strategy, kOptBool, kOptInSession, 0, 0, nullptr},
    {"cont_order", &Options::cont_order, kOptZeroOne, kOptInSession, 0, 0, "0 (append order) or 1 (canonical order)"},
    {"deterministic", &Options::deterministic, kOptZeroOne, kOptInSession, 0, 0, "0 (float accumulation) or 1 (fixed-point accumulation)"},
    {"log_tiles_log2", &Options::log_tiles_log2, kOptClamp, 0, 0, 8, nullptr},
    {"alt_log2", &Options::alt_log2, kOptClamp, 0, 10, 28, nullptr},
    {"small_blocks_per_cu", &Options::small_blocks_per_cu, kOptClamp, 0, 0, kOptNoCap, nullptr},
    {"blocks_cap", &Options::blocks_cap, kOptClamp, 0, 0, kOptNoCap, nullptr},
    // (planes of ended sessions may still wait for their fold — lazy_fold — and nothing may still be reading what a changed count frees)
    {"mono_copies", &Options::mono_copies, kOptCopies, kOptInSession, 0, 0, nullptr},
    {"blocks_per_cu", &Options::blocks_per_cu, kOptClamp, 0, 1, 64, nullptr},
    // the layers of an open session draw their gate / transit / shape streams at indices that follow on from the first layer's.
    // rank: disjoint 64-bit counter ranges per shard — the hi word feeds pcg_seed_with_high, so ranks never share a stream
    {"rank", &Options::rank, kOptRank, kOptInSession | kOptAlways, 0, 0, nullptr},
    // re-seed between sessions (the reference's backends take their seed from the first non-zero SessionSpec::seed, cpu_trace_backend.cpp:252)
    {"seed", OptField(), kOptSeed, kOptInSession | kOptAlways, 0, 0, nullptr},
    // the session's first 64-bit ray index (SplitPcgRayBase, trace_backend.hpp:184: lo feeds the stream index, hi pcg_seed_with_high)
    {"ray_base", &Options::rank, kOptRayBase, kOptInSession | kOptAlways, 0, 0, nullptr},
};

inline bool operator==(const Options& a, const Options& b) {
  for (const OptionRow& r : kOptionTable)
    if (r.field.get(a) != r.field.get(b)) return false;
  return true;
}
inline bool operator!=(const Options& a, const Options& b) { return !(a == b); }

// The verdict on one set.  Refused: `message`, and nothing else is to happen.  Otherwise the backend performs `effects`, then commits.
struct OptionSet {
  enum Status { kRefused, kUnchanged, kChanged } status = kRefused;
  std::string message;
  const OptionRow* row = nullptr;
  int64_t value = 0;           // normalised, as the member will hold it (seed: the seed)
  uint32_t effects = 0;        // kFx*
  uint64_t counter_base = 0;   // kFxCounters: where the four ray counters go
  void commit(Options& o) const {
    if (row) row->field.set(o, value);
  }
};

// Most options shape the tables or the kernels that read them: a CHANGED option drops the table cache.  A caller that sets its options before
// every session (the Lumice glue does) sets them to what they are: "unchanged" — the normalised value is the option's current one — keeps the
// cache.  Counter / seed options always act (they move state).  `chunk_top`: the ceiling of "chunk", from the device's CU count.
inline OptionSet set_option(const Options& cur, bool in_session, uint32_t shard_count, uint64_t chunk_top, const char* key, int64_t v) {
  OptionSet r;
  auto refuse = [&r](std::string why) {
    r.message = std::move(why);
    return r;
  };
  const std::string k(key);
  for (const OptionRow& row : kOptionTable)
    if (k == row.key) r.row = &row;
  if (!r.row) return refuse("unknown option: " + k);
  const OptionRow& row = *r.row;
  if ((row.flags & kOptInSession) && in_session)
    return refuse(k + (row.rule == kOptCopies ? " cannot change while a session's plane is pending" : " cannot change inside a session"));
  int64_t n = v;
  switch (row.rule) {
    case kOptBool: n = v ? 1 : 0; break;
    case kOptTri: n = v < 0 ? -1 : (v ? 1 : 0); break;
    case kOptTicket: n = v < -1 ? -2 : v < 0 ? -1 : (v ? 1 : 0); break;
    case kOptInt: break;
    case kOptClamp: n = v < row.lo ? row.lo : v > row.hi ? row.hi : v; break;
    case kOptPositiveOr: n = v > 0 ? v : row.lo; break;
    case kOptZeroOne:
      if (v != 0 && v != 1) return refuse(k + " must be " + row.note);
      break;
    case kOptPow2:
    case kOptPow2Log2:
      if (v < row.lo || v > row.hi || (v & (v - 1)) != 0)
        return refuse(k + " must be a power of two in [" + std::to_string(row.lo) + ", " + std::to_string(row.hi) + "]");
      if (row.rule == kOptPow2Log2)
        for (n = 0; (1ll << n) < v;) n++;
      break;
    case kOptChunk: {
      const uint64_t want = static_cast<uint64_t>(v > 0 ? v : (1ll << 28));
      n = static_cast<int64_t>(want < chunk_top ? want : chunk_top);
      break;
    }
    case kOptCopies:
      for (n = 1; n < v && n < 64;) n <<= 1;
      r.effects |= kFxFoldPlanes;
      break;
    case kOptRank:
      if (v != 0 && shard_count > 1) return refuse("rank: not with halo_set_shard count > 1 (shards trace the one-rank run's rays: they share its counter range)");
      r.counter_base = static_cast<uint64_t>(v) << 40;
      r.effects |= kFxCounters;
      break;
    case kOptRayBase:
      n = 0;
      r.counter_base = static_cast<uint64_t>(v);
      r.effects |= kFxCounters;
      break;
    case kOptSeed:
      n = static_cast<uint32_t>(v) ? static_cast<uint32_t>(v) : 1u;
      r.effects |= kFxSeed;
      break;
  }
  r.value = row.field.fit(n);
  if (row.flags & kOptSyncFirst) r.effects |= kFxSync;
  const bool changed = (row.flags & kOptAlways) || r.value != row.field.get(cur);
  if (changed) r.effects |= kFxDropCache | (row.rule == kOptCopies ? kFxSync | kFxReleasePlanes : 0u);
  r.status = changed ? OptionSet::kChanged : OptionSet::kUnchanged;
  return r;
}

}  // namespace halo

#endif
