// select_enum.h — every request a trace launch can make of the kernel selection, in one fixed order (tests/cpp/select_main.cpp, and the recorder
// that took tests/golden/kernel_selection.txt from the launcher ladder this selection replaced).
//
// A request is (DispatchParams, mode, geom, mono).  Its ordinal number counts the full product of the facts below, the first fact slowest:
//
//   mode         0..4                      geom        0..3                          mono         false, true
//   tile_chunk   null, set                 ticket      null | set, ticket_waves 0 | set, ticket_waves 1
//   tile fields  valid | tile_cnt null | tile_tiles 0 | tile_tiles > kTileAppendMax | tile_cap odd
//   fix          null, set                 bin_log     0, 1                          bin_list     null, set
//   no_land      0, 1                      cont_mask   null, set                     final_layer  0, 1
//   prob         0, 0.5                    mono_by_wl  0, 1                          spec_per     0, 7
//   lens         linear, fisheye equal area, dual fisheye equal area, rectangular, fisheye equidistant (one that is no template constant)
//   visible      upper, full, lower
//   orientation  LUT latitude + uniform azimuth + uniform roll | latitude full sphere | azimuth gauss | roll gauss
//   root_profile none, gen, transit        source      gen, transit, host
//
// 8 294 400 requests per (mode, geom, mono), 331 776 000 in all.  Pointers that are "set" hold one dummy address: nothing dereferences them.
#ifndef HALO_TESTS_SELECT_ENUM_H_
#define HALO_TESTS_SELECT_ENUM_H_

#include <stdint.h>

#include "../../ice_halo_sim_amd/csrc/halo_device.h"

namespace select_enum {

constexpr uint64_t kPerGroup = 2ull * 3 * 5 * 512 * 5 * 3 * 4 * 3 * 3;
constexpr int kGroups = 5 * 4 * 2;

// f(ordinal, P, mode, geom, mono) for every request of group `g` (= (mode * 4 + geom) * 2 + mono), in ordinal order
template <typename F>
void for_each_request(int g, F&& f) {
  static uint64_t dummy[2];
  void* const set = dummy;
  const int mode = g / 8, geom = (g / 2) % 4;
  const bool mono = (g & 1) != 0;
  uint64_t ord = static_cast<uint64_t>(g) * kPerGroup;
  static const int kLens[5] = {HALO_LENS_LINEAR, HALO_LENS_FISHEYE_EQUAL_AREA, HALO_LENS_DUAL_FISHEYE_EQUAL_AREA, HALO_LENS_RECTANGULAR, HALO_LENS_FISHEYE_EQUIDISTANT};
  static const int kVis[3] = {HALO_VISIBLE_UPPER, HALO_VISIBLE_FULL, HALO_VISIBLE_LOWER};
  static const uint32_t kProfile[3] = {halo::kRootProfileNone, halo::kRootProfileGen, halo::kRootProfileTransit};
  static const uint32_t kSource[3] = {halo::kSrcGen, halo::kSrcTransit, halo::kSrcHost};
  halo::DispatchParams P{};
  for (int tile = 0; tile < 2; tile++) {
    P.tile_chunk = tile ? static_cast<halo::HitRec*>(set) : nullptr;
    for (int ticket = 0; ticket < 3; ticket++) {
      P.ticket = ticket ? static_cast<uint32_t*>(set) : nullptr;
      P.ticket_waves = ticket == 2 ? 1u : 0u;
      for (int tf = 0; tf < 5; tf++) {
        P.tile_cnt = tf == 1 ? nullptr : static_cast<uint32_t*>(set);
        P.tile_tiles = tf == 2 ? 0u : tf == 3 ? halo::kTileAppendMax + 1u : 64u;
        P.tile_cap = tf == 4 ? 17u : 16u;
        for (int bits = 0; bits < 512; bits++) {
          P.fix = (bits & 256) ? static_cast<unsigned long long*>(set) : nullptr;
          P.bin_log = (bits & 128) ? 1u : 0u;
          P.bin_list = (bits & 64) ? static_cast<halo::HitRec*>(set) : nullptr;
          P.no_land = (bits & 32) ? 1u : 0u;
          P.cont_mask = (bits & 16) ? static_cast<uint32_t*>(set) : nullptr;
          P.final_layer = (bits & 8) ? 1u : 0u;
          P.prob = (bits & 4) ? 0.5f : 0.0f;
          P.mono_by_wl = (bits & 2) ? 1u : 0u;
          P.spec_per = (bits & 1) ? 7u : 0u;
          for (int lens = 0; lens < 5; lens++) {
            P.proj.proj_type = kLens[lens];
            for (int vis = 0; vis < 3; vis++) {
              P.proj.visible_range = kVis[vis];
              for (int orient = 0; orient < 4; orient++) {
                P.lat_path = orient == 1 ? halo::kLatFullSphere : halo::kLatLut;
                P.az_type = orient == 2 ? HALO_DIST_GAUSS : HALO_DIST_UNIFORM;
                P.roll_type = orient == 3 ? HALO_DIST_GAUSS : HALO_DIST_UNIFORM;
                for (int prof = 0; prof < 3; prof++) {
                  P.root_profile = kProfile[prof];
                  for (int src = 0; src < 3; src++) {
                    P.source = kSource[src];
                    f(ord++, P, mode, geom, mono);
                  }
                }
              }
            }
          }
        }
      }
    }
  }
}

// what a request chose: a kernel's nine template arguments, or an error code (hipError_t's value) with mode < 0
struct Choice {
  int mode, geom, mono, acc, lens, vis, nogate, canon, root;
  bool operator==(const Choice& o) const {
    return mode == o.mode && geom == o.geom && mono == o.mono && acc == o.acc && lens == o.lens && vis == o.vis && nogate == o.nogate && canon == o.canon && root == o.root;
  }
};
inline Choice error_choice(int err) { return Choice{-1, err, 0, 0, 0, 0, 0, 0, 0}; }

// One group's tally: per choice, the number of requests that made it and a 64-bit hash (FNV-1a over the ordinal numbers, as words, in order).
// Printed in order of first appearance, which is as fixed as the enumeration.
struct Tally {
  struct Row {
    Choice c;
    uint64_t n, h;
  };
  Row rows[256];
  int cnt = 0, last = 0;
  void add(const Choice& c, uint64_t ord) {
    if (cnt == 0 || !(rows[last].c == c)) {
      for (last = 0; last < cnt && !(rows[last].c == c); last++) {
      }
      if (last == cnt) {
        if (cnt == 256) __builtin_trap();
        rows[cnt++] = Row{c, 0u, 0xcbf29ce484222325ull};
      }
    }
    rows[last].n++;
    rows[last].h = (rows[last].h ^ ord) * 0x100000001b3ull;
  }
  template <typename Print>   // print(const char* line)
  void print(int g, Print&& out) const {
    char line[200];
    for (int i = 0; i < cnt; i++) {
      const Row& r = rows[i];
      const Choice& c = r.c;
      int k = __builtin_snprintf(line, sizeof line, "mode %d geom %d mono %d: ", g / 8, (g / 2) % 4, g & 1);
      if (c.mode < 0) k += __builtin_snprintf(line + k, sizeof line - k, "error %d", c.geom);
      else
        k += __builtin_snprintf(line + k, sizeof line - k, "halo_trace_kernel<%d, %d, %s, %d, %d, %d, %s, %s, %d>", c.mode, c.geom, c.mono ? "true" : "false", c.acc, c.lens,
                                c.vis, c.nogate ? "true" : "false", c.canon ? "true" : "false", c.root);
      __builtin_snprintf(line + k, sizeof line - k, "  requests %llu  hash %016llx", static_cast<unsigned long long>(r.n), static_cast<unsigned long long>(r.h));
      out(line);
    }
  }
};

}  // namespace select_enum

#endif
