// options_main.cpp — the option rules of halo_set_option (csrc/halo_options.h) on the host: keys, defaults, every value rule at its edges, the
// refusals inside a session, "refused leaves nothing behind", "unchanged" and "always acts".  Built from the header alone (tests/test_cpp_options.py);
// prints one line per failed check and "ok" when there is none.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>

#include "../../ice_halo_sim_amd/csrc/halo_options.h"

using namespace halo;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      failures++;                                         \
      std::printf("line %d: %s: ", __LINE__, #cond);      \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
    }                                                     \
  } while (0)

constexpr uint64_t kTop = (1ull << 32) - 256ull * 64ull * 256ull - 256ull;   // the "chunk" ceiling of a 256-CU device

static OptionSet ask(const Options& o, const char* key, int64_t v, bool in_session = false, uint32_t shards = 1) {
  return set_option(o, in_session, shards, kTop, key, v);
}
// A set outside a session on default options: the stored value, which must not be refused.
static int64_t stored(const char* key, int64_t v) {
  const OptionSet s = ask(Options(), key, v);
  CHECK(s.status != OptionSet::kRefused, "%s = %lld refused: %s", key, static_cast<long long>(v), s.message.c_str());
  return s.value;
}
static void expect(const char* key, std::initializer_list<int64_t> raw, std::initializer_list<int64_t> want) {
  auto w = want.begin();
  for (int64_t v : raw) {
    const int64_t got = stored(key, v);
    CHECK(got == *w, "%s = %lld stores %lld, expected %lld", key, static_cast<long long>(v), static_cast<long long>(got), static_cast<long long>(*w));
    ++w;
  }
}
static void expect_refused(const Options& o, const char* key, int64_t v, bool in_session, const char* message, uint32_t shards = 1) {
  const OptionSet s = ask(o, key, v, in_session, shards);
  CHECK(s.status == OptionSet::kRefused && s.message == message && s.effects == 0u, "%s = %lld: status %d, message \"%s\"", key, static_cast<long long>(v),
        static_cast<int>(s.status), s.message.c_str());
}

struct Default { const char* key; int64_t legal, value; };   // a legal raw value; the value the key's member starts with (seed: none)
static const Default kDefaults[] = {
    {"capture_exits", 1, 0}, {"geom_clock", 16, 32}, {"chunk", 1 << 20, 1ll << 28}, {"bin_l1", 64, 128}, {"stoch_chunk", 1 << 20, 0},
    {"aggregate", 0, 1}, {"mono", 0, 1}, {"async", 1, 0}, {"lambda_planes", 1, -1}, {"bin", 1, -1},
    {"host_shapes", 1, 0}, {"entry_fast", 0, 1}, {"hex_fast", 0, 1}, {"filter_fast", 0, 1}, {"spec_root", 0, 1},
    {"hit_log", 1, -1}, {"hit_log_cap", 2048, 0}, {"gen_serial", 1, 0}, {"shuffle_chunk", 4, 5}, {"lazy_fold", 0, 1},
    {"table_cache", 0, 1}, {"overlap", 0, 1}, {"defer_fold", 1, 0}, {"auto_ev_hist", 1, 0}, {"auto_ev_select", 1, -1},
    {"stats_select", 1, -1}, {"gen_ahead", 1, 0}, {"close_direct", 1, -1}, {"lean_events", 0, 1}, {"tile_append", 1, -1},
    {"tile_ticket", 1, -2}, {"ticket_min", 8, 4}, {"ticket_max", 32, 64}, {"ticket_div", 4, 2}, {"pool_entry_fast", 0, 1},
    {"rehit_strategy", 0, 1}, {"cont_order", 1, 0}, {"deterministic", 1, 0}, {"log_tiles_log2", 5, 7}, {"alt_log2", 20, 25},
    {"small_blocks_per_cu", 3, 0}, {"blocks_cap", 100, 0}, {"mono_copies", 4, 8}, {"blocks_per_cu", 12, 24}, {"rank", 3, 0},
    {"seed", 7, 0}, {"ray_base", 1000, 0},
};

static int64_t legal_of(const char* key) {
  for (const Default& d : kDefaults)
    if (std::strcmp(d.key, key) == 0) return d.legal;
  return 0;
}

int main() {
  const Options def;
  constexpr size_t kKeys = sizeof(kOptionTable) / sizeof(kOptionTable[0]);

  // ---- keys and defaults: the table and the list above name the same 47 keys
  CHECK(kKeys == 47 && sizeof(kDefaults) / sizeof(kDefaults[0]) == kKeys, "%zu keys in the table", kKeys);
  for (const OptionRow& row : kOptionTable) {
    const Default* d = nullptr;
    for (const Default& c : kDefaults)
      if (std::strcmp(c.key, row.key) == 0) d = &c;
    CHECK(d != nullptr, "%s is missing from the test's list", row.key);
    if (!d) continue;
    if (std::strcmp(row.key, "seed") != 0) CHECK(row.field.get(def) == d->value, "%s defaults to %lld", row.key, static_cast<long long>(row.field.get(def)));
    const OptionSet s = ask(def, row.key, d->legal);
    CHECK(s.status == OptionSet::kChanged && s.row == &row && (s.effects & kFxDropCache), "%s = %lld: status %d", row.key, static_cast<long long>(d->legal), static_cast<int>(s.status));
    Options o = def;
    s.commit(o);
    if (std::strcmp(row.key, "seed") != 0) CHECK(row.field.get(o) == s.value, "%s: committed %lld, verdict %lld", row.key, static_cast<long long>(row.field.get(o)), static_cast<long long>(s.value));
  }
  CHECK(def.spec_root == 1, "spec_root defaults to on");
  expect_refused(def, "no_such_option", 1, false, "unknown option: no_such_option");
  expect_refused(def, "", 1, false, "unknown option: ");

  // ---- value rules at their edges
  for (const OptionRow& row : kOptionTable) {
    if (row.rule == kOptBool) expect(row.key, {0, 1, 7, -3}, {0, 1, 1, 1});
    if (row.rule == kOptTri) expect(row.key, {-5, -1, 0, 2}, {-1, -1, 0, 1});
    if (row.rule == kOptClamp) {
      expect(row.key, {row.lo, row.lo - 1}, {row.lo, row.lo});
      if (row.hi != kOptNoCap) expect(row.key, {row.hi, row.hi + 1}, {row.hi, row.hi});
    }
  }
  expect("tile_ticket", {-3, -2, -1, 0, 5}, {-2, -2, -1, 0, 1});
  expect("aggregate", {0, 1, 2}, {0, 1, 2});   // (as given: the kernels compare it with 0 and 1)
  expect("ticket_min", {0, 1, 1024, 1025}, {1, 1, 1024, 1024});
  expect("ticket_div", {0, 1, 64, 65}, {1, 1, 64, 64});
  expect("log_tiles_log2", {-1, 0, 8, 9}, {0, 0, 8, 8});
  expect("alt_log2", {9, 10, 28, 29}, {10, 10, 28, 28});
  expect("blocks_per_cu", {0, 1, 64, 65}, {1, 1, 64, 64});
  expect("hit_log_cap", {-1, 0, 4096}, {0, 0, 4096});
  expect("small_blocks_per_cu", {-1, 0, 7}, {0, 0, 7});
  expect("blocks_cap", {-1, 0, 7}, {0, 0, 7});
  expect("bin_l1", {8, 512}, {8, 512});
  for (int64_t v : {4, 96, 1024}) expect_refused(def, "bin_l1", v, false, "bin_l1 must be a power of two in [8, 512]");
  expect("shuffle_chunk", {1, 2, 64}, {0, 1, 6});
  for (int64_t v : {0, 3, 128}) expect_refused(def, "shuffle_chunk", v, false, "shuffle_chunk must be a power of two in [1, 64]");
  expect("chunk", {0, static_cast<int64_t>(kTop) + 1, static_cast<int64_t>(kTop), 1000}, {1ll << 28, static_cast<int64_t>(kTop), static_cast<int64_t>(kTop), 1000});
  expect("mono_copies", {0, 1, 3, 64, 1000}, {1, 1, 4, 64, 64});
  expect("geom_clock", {0, -1, 5}, {32, 32, 5});
  expect("stoch_chunk", {0, -1, 5}, {0, 0, 5});
  expect("cont_order", {0, 1}, {0, 1});
  expect("deterministic", {0, 1}, {0, 1});
  for (int64_t v : {-1, 2}) {
    expect_refused(def, "cont_order", v, false, "cont_order must be 0 (append order) or 1 (canonical order)");
    expect_refused(def, "deterministic", v, false, "deterministic must be 0 (float accumulation) or 1 (fixed-point accumulation)");
  }
  expect("seed", {0, 5, 1ll << 32}, {1, 5, 1});

  // ---- effects: what the backend is asked to perform
  CHECK(ask(def, "overlap", 1).effects == kFxSync, "overlap syncs on every set, changed or not");
  CHECK(ask(def, "overlap", 0).effects == (kFxSync | kFxDropCache), "overlap = 0");
  CHECK(ask(def, "mono_copies", 8).effects == kFxFoldPlanes, "mono_copies folds on every set");
  CHECK(ask(def, "mono_copies", 4).effects == (kFxFoldPlanes | kFxSync | kFxReleasePlanes | kFxDropCache), "a changed mono_copies releases the planes");
  {
    const OptionSet r = ask(def, "rank", 3), b = ask(def, "ray_base", 1000), s = ask(def, "seed", 9);
    CHECK(r.effects == (kFxCounters | kFxDropCache) && r.counter_base == (3ull << 40) && r.value == 3, "rank = 3");
    CHECK(b.effects == (kFxCounters | kFxDropCache) && b.counter_base == 1000ull && b.value == 0, "ray_base = 1000");
    CHECK(s.effects == (kFxSeed | kFxDropCache) && s.value == 9, "seed = 9");
    Options o = def;
    r.commit(o);
    CHECK(o.rank == 3, "rank is remembered");
    ask(o, "ray_base", 5).commit(o);
    CHECK(o.rank == 0, "ray_base takes the rank back");
  }
  expect_refused(def, "rank", 1, false, "rank: not with halo_set_shard count > 1 (shards trace the one-rank run's rays: they share its counter range)", 2);
  CHECK(ask(def, "rank", 0, false, 2).status == OptionSet::kChanged, "rank = 0 is legal on a shard");

  // ---- inside a session: refused with the present message, nothing changes
  for (const OptionRow& row : kOptionTable) {
    if (!(row.flags & kOptInSession)) {
      CHECK(ask(def, row.key, legal_of(row.key), true).status == OptionSet::kChanged, "%s is legal inside a session", row.key);
      continue;
    }
    const Options before = def;
    const std::string want = std::string(row.key) + (std::strcmp(row.key, "mono_copies") == 0 ? " cannot change while a session's plane is pending" : " cannot change inside a session");
    expect_refused(def, row.key, 1, true, want.c_str());
    CHECK(before == def, "%s: the options changed under a refusal", row.key);
  }
  {
    int flagged = 0;
    for (const char* key : {"capture_exits", "filter_fast", "rehit_strategy", "cont_order", "deterministic", "mono_copies", "rank", "seed", "ray_base"})
      for (const OptionRow& row : kOptionTable)
        if (std::strcmp(row.key, key) == 0 && (row.flags & kOptInSession)) flagged++;
    int all = 0;
    for (const OptionRow& row : kOptionTable) all += (row.flags & kOptInSession) ? 1 : 0;
    CHECK(flagged == 9 && all == 9, "%d of the nine session keys carry the flag, %d rows carry it", flagged, all);
  }

  // ---- refused, then legal: the refusal is not remembered
  {
    Options o = def;
    expect_refused(o, "capture_exits", 1, true, "capture_exits cannot change inside a session");
    CHECK(o == def, "a refused set left something behind");
    const OptionSet s = ask(o, "capture_exits", 1, false);
    CHECK(s.status == OptionSet::kChanged && (s.effects & kFxDropCache), "the legal set after the refused one must drop the table cache");
    s.commit(o);
    CHECK(o.capture == 1 && o != def, "capture_exits = 1 committed");
  }

  // ---- unchanged: the normalised value is the current one
  for (const OptionRow& row : kOptionTable) {
    if (row.flags & kOptAlways) {
      CHECK(ask(def, row.key, row.field.get(def)).status == OptionSet::kChanged, "%s always acts", row.key);
      continue;
    }
    const int64_t raw = row.rule == kOptPow2Log2 ? (1ll << row.field.get(def)) : row.field.get(def);
    const OptionSet s = ask(def, row.key, raw);
    CHECK(s.status == OptionSet::kUnchanged && !(s.effects & kFxDropCache), "%s set to its current value: status %d", row.key, static_cast<int>(s.status));
  }
  CHECK(ask(def, "spec_root", 5).status == OptionSet::kUnchanged, "5 normalises to the boolean's current 1");
  CHECK(ask(def, "mono_copies", 7).status == OptionSet::kUnchanged, "7 rounds to the current 8 copies");
  CHECK(ask(def, "geom_clock", 0).status == OptionSet::kUnchanged, "0 means the default, which is current");
  CHECK(ask(def, "tile_ticket", -9).status == OptionSet::kUnchanged, "-9 normalises to the current -2");
  for (const char* key : {"rank", "ray_base", "seed"})
    for (int64_t v : {0, 1}) {
      Options o = def;
      for (int again = 0; again < 2; again++) {   // the second set finds the first one's value in place
        const OptionSet s = ask(o, key, v);
        CHECK(s.status == OptionSet::kChanged && (s.effects & kFxDropCache), "%s = %lld must act every time", key, static_cast<long long>(v));
        s.commit(o);
      }
    }

  if (failures == 0) std::printf("ok\n");
  return failures == 0 ? 0 : 1;
}
