// halo_select.h — which instantiation of halo_trace_kernel a launch runs, decided in one place.  Plain C++17: no kernel code, no launch.
//
//   KernelId        the nine template arguments of halo_trace_kernel (halo_trace.inl), as values
//   kernel_exists   the kernel set: an instantiation exists in the library exactly where this holds
//   KernelRequest   the facts of a launch that the choice reads; make_request fills it from (DispatchParams, mode, geom, mono)
//   select_kernel   request -> id, or the error the launch returns instead (every fall-back to a more generic form is here)
//   expand_kernel   run-time id -> template constants, handed to a callable; instantiates the callable for the ids of one family only
//
// halo_trace.inl launches through these (launch_family), halo_backend.cpp reads the route record and the per-tile append's conditions off
// them, tests/cpp/select_main.cpp checks select_kernel over every request against tests/golden/kernel_selection.txt.
// Adding a kernel family: DESIGN.md, "How a launch finds its kernel".
#ifndef HALO_SELECT_H_
#define HALO_SELECT_H_

#include <stdint.h>

#include <utility>

#include "halo_device.h"

namespace halo {

// ---- the template arguments' values -------------------------------------------------------------------------------------------------------
constexpr int kModePlain = 0, kModeFilter = 1, kModeCapture = 2, kModeGeneric = 3, kModeColor = 4;
constexpr bool mode_fast(int mode) { return mode == kModePlain || mode == kModeFilter || mode == kModeColor; }   // production-shaped kernels (ModeTraits::kFast)

constexpr int kGeomOne = 0, kGeomPool = 1, kGeomPoolPrism = 2;   // GEOM: one shape per dispatch | pool of ShapeDev | pool of ShapePrism (HBM records and LDS slots)
constexpr int kGeomOneHex = 3;   // one shape per dispatch AND it is a regular hexagonal prism (EntryFastDev::hex_regular): literal normals
constexpr bool geom_one(int geom) { return geom == kGeomOne || geom == kGeomOneHex; }

constexpr int kAccDirect = 0, kAccBin = 1, kAccLog = 2, kAccNone = 3, kAccLogFinal = 4;   // halo_trace_kernel ACC (None: a layer whose every exit continues — nothing lands)
constexpr int kAccFixed = 5;   // the integer twin of kAccDirect (option "deterministic"): FixCache in LDS, 64-bit integer atomics onto DispatchParams::fix
constexpr int kAccFixedLog = 6;   // ... and of the logging kernels: the same cache, but a hit that loses the claim leaves as a raw {slot, weight} record (log_hit_fixed)
constexpr int kAccTileFinal = 7;   // kAccLogFinal whose records go to per-tile chunks of the workgroup instead of its one region (log_hit_tile): no split pass

// Root profiles (halo_trace_kernel's ROOT): what the last-layer kernels of the regular prism know about their root generation at compile time.
// kRootAny keeps every choice a run-time test.  The two others are the orientation the shipped column / plate examples and the BASELINE
// configurations take — latitude by the LUT, azimuth and roll uniform — over generated roots or over the continuation pool: the tests on the
// source, the latitude path and the five distribution kinds (three of which carry logf / cosf / sinf) fold away, and with them 60 % of the
// kernel's code.  Same expressions, draws and stream slots.
constexpr int kRootAny = -1, kRootGenLutUniform = 0, kRootTransitLutUniform = 1;
// ... and the ticketed form of a kAccTileFinal kernel (DispatchParams::ticket, halo_device.h TicketSize) rides on the same template argument, so
// that no kernel of the static form changes its name: ROOT + kRootTicket is the ticketed twin of root form ROOT.
constexpr int kRootTicket = 16;
constexpr bool root_ticketed(int root) { return root >= kRootTicket + kRootAny; }
constexpr int root_form(int root) { return root_ticketed(root) ? root - kRootTicket : root; }

// the launch errors, as hipError_t's values (hipErrorInvalidValue, hipErrorNotSupported; halo_trace.inl holds them to that)
constexpr int kSelectInvalidValue = 1, kSelectNotSupported = 801;

// ---- KernelId ---------------------------------------------------------------------------------------------------------------------------------
struct KernelId {
  int mode = kModePlain, geom = kGeomOne;
  bool mono = false;
  int acc = kAccDirect;
  int lens = -1, vis = -1;   // >= 0: that HALO_LENS_* / HALO_VISIBLE_* as a constant; -1: read from the dispatch record
  bool nogate = false;       // prob <= 0 as a constant
  bool canon = false;        // a layer before the last under canonical continuation order: appends carry their key
  int root = kRootAny;       // kRoot*, + kRootTicket for the ticketed twin
};
constexpr bool operator==(const KernelId& a, const KernelId& b) {
  return a.mode == b.mode && a.geom == b.geom && a.mono == b.mono && a.acc == b.acc && a.lens == b.lens && a.vis == b.vis && a.nogate == b.nogate && a.canon == b.canon &&
         a.root == b.root;
}
// ... as template constants: what expand_kernel hands its callable
template <int MODE, int GEOM, bool MONO, int ACC, int LENS, int VIS, bool NOGATE, bool CANON, int ROOT>
struct KernelConst {
  static constexpr KernelId id() { return KernelId{MODE, GEOM, MONO, ACC, LENS, VIS, NOGATE, CANON, ROOT}; }
};

// The families: each is instantiated by one translation unit (halo_trace_m<mode>.hip, halo_trace_fx<mode>.hip, halo_trace_fxl<mode>.hip,
// halo_trace_tl0.hip), which compile side by side.
constexpr int kFamMode = 0, kFamFixed = 5, kFamFixedLog = 7, kFamTile = 9, kFamilies = 10;   // + mode (kFamMode: 0..4; the fixed-point ones: 0..1; kFamTile: 0)
constexpr int family_base(int family) { return family >= kFamTile ? kFamTile : family >= kFamFixedLog ? kFamFixedLog : family >= kFamFixed ? kFamFixed : kFamMode; }
constexpr int family_mode(int family) { return family - family_base(family); }
constexpr int family_of(const KernelId& k) {
  return k.acc == kAccTileFinal ? kFamTile + k.mode : k.acc == kAccFixedLog ? kFamFixedLog + k.mode : k.acc == kAccFixed ? kFamFixed + k.mode : kFamMode + k.mode;
}

// ---- the kernel set ---------------------------------------------------------------------------------------------------------------------------
// Lenses that are template constants: those of the reference's shipped examples (config_example.json: linear, dual fisheye equal area; the
// BASELINE configurations: fisheye equal area; bench_config_stoch.json: rectangular) x visible upper / full; anything else runs the generic
// kernel.  LENS / VIS >= 0 and NOGATE fold away the projection's dispatch over 11 lens types (uniform branches, and the SGPRs their parameters
// hold), the visibility tests and the gate stream: configs[1] 2.96 -> 2.73 (lens) -> 2.60 ms per launch.
constexpr bool lens_constant(int lens) {
  return lens == HALO_LENS_LINEAR || lens == HALO_LENS_FISHEYE_EQUAL_AREA || lens == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA || lens == HALO_LENS_RECTANGULAR;
}
constexpr bool vis_constant(int vis) { return vis == HALO_VISIBLE_UPPER || vis == HALO_VISIBLE_FULL; }

constexpr bool kernel_exists(const KernelId& k) {
  if (k.mode < kModePlain || k.mode > kModeColor || k.geom < kGeomOne || k.geom > kGeomOneHex) return false;
  const bool fast = mode_fast(k.mode), one = geom_one(k.geom), pool = !one;
  const bool generic = k.lens < 0 && k.vis < 0 && !k.nogate;   // the run-time lens form
  const bool plain_or_filter = k.mode == kModePlain || k.mode == kModeFilter;
  // the regular-prism search exists for the production-shaped kernels
  if (k.geom == kGeomOneHex && !fast) return false;
  // Root profiles: the last-layer plain hit-log kernels of the regular prism with lens, visible range and closed gate as constants.  Not the
  // continuation-pool profile under the linear lens over the full sky: that one instantiation's register allocation answers the profile with
  // 4 spilled VGPRs and scratch.
  // Wave tickets: the per-tile append's kernels.  Not for the dual fisheye: that instantiation's register allocation answers the ticket loop
  // with a spilled VGPR inside the ray loop (the pixel cache's slot index), and a ticketed kernel is held to none there.
  const int form = root_form(k.root);
  if (form != kRootAny && form != kRootGenLutUniform && form != kRootTransitLutUniform) return false;
  if (form != kRootAny && !(k.mode == kModePlain && k.geom == kGeomOneHex && k.mono && (k.acc == kAccLogFinal || k.acc == kAccTileFinal) && k.nogate && k.lens >= 0)) return false;
  if (form == kRootTransitLutUniform && k.lens == HALO_LENS_LINEAR && k.vis == HALO_VISIBLE_FULL) return false;
  if (root_ticketed(k.root) && !(k.acc == kAccTileFinal && k.lens != HALO_LENS_DUAL_FISHEYE_EQUAL_AREA)) return false;
  // Canonical continuation order: the CANON twins of the direct-accumulation and no-accumulation kernels (and the direct ones' integer twins) —
  // the host gives such a layer neither the hit log nor binned lists, so no other instantiation needs a twin.
  if (k.canon && k.acc != kAccDirect && k.acc != kAccNone && k.acc != kAccFixed) return false;
  switch (k.acc) {
    case kAccDirect: return generic;
    case kAccBin: return generic && k.mono && k.geom != kGeomOneHex;   // (the regular prism's instantiation: the direct and logged routes)
    case kAccNone: return generic && fast && one && k.mono;   // every exit continues: no cache, no queue; one (scalar) flavour serves every session
    // the fixed-point kernels: plain and fast-filter mode only, every GEOM, either plane layout, in the generic run-time lens form only
    case kAccFixed:
    case kAccFixedLog: return generic && plain_or_filter;
    // the last layer's one-shape scalar kernels, which carry no continuation-append code: lens, visible range and closed gate as constants
    case kAccLogFinal: return fast && one && k.mono && (generic || (plain_or_filter && lens_constant(k.lens) && vis_constant(k.vis) && k.nogate));
    case kAccLog:   // the hit log exists for the production-shaped kernels: scalar planes, or X/Y/Z planes of an illuminant session
      if (!fast) return false;
      if (generic) return true;
      // (round 6: the logging kernels of the layers BEFORE the last — their gate is open, the lens and the visible range are as constant as in
      //  the last layer, and the generic-lens form of them carried every lens's code: 8723 instructions, 120 spilled SGPRs, 10 spilled VGPRs and
      //  scratch against 4612 / 45 / 0 / none for the dual-fisheye instantiation, tools/isa_by_line.py.)
      if (one) return plain_or_filter && k.mono && lens_constant(k.lens) && vis_constant(k.vis) && !k.nogate;
      // (round 6, end: the reference's own stochastic benchmark — bench_config_stoch.json: rectangular lens, full sky, closed gate — as constants
      //  for the shape-pool kernels of both plane layouts.  The pool kernels project at the emit site, and the generic form of them holds every
      //  lens's code inside the interaction loop: 14 283 instructions, 157 spilled SGPRs, 3 spilled VGPRs and scratch against 9950 / 73 / 0 / none.)
      if (pool && k.mode == kModePlain && k.lens == HALO_LENS_RECTANGULAR && k.vis == HALO_VISIBLE_FULL && k.nogate) return true;
      // illuminant sessions over sampled crystals: a full-sky render with a closed gate (bench_config_stoch.json's shape) knows both at compile
      // time (configs[4] 5.52 -> 5.43 ms per step; its lens as a constant gains nothing more: 4.31 vs 4.32 ms per launch)
      return pool && k.mode == kModePlain && !k.mono && k.lens < 0 && k.vis == HALO_VISIBLE_FULL && k.nogate;
    // The per-tile append: the kAccTileFinal twins of the headline's kernels — plain mode, one regular prism, scalar plane, last layer with a
    // closed gate, lens and root form as constants, the upper sky (the closing per-tile pass, which reads the chunks, takes no full-sky render).
    case kAccTileFinal: return k.mode == kModePlain && k.geom == kGeomOneHex && k.mono && lens_constant(k.lens) && k.vis == HALO_VISIBLE_UPPER && k.nogate;
  }
  return false;
}

// ---- KernelRequest ----------------------------------------------------------------------------------------------------------------------------
struct KernelRequest {
  int mode, geom;   // geom: the launch's kGeom* (kGeomOneHex where the host found a regular prism; the selection may still answer kGeomOne)
  bool mono;        // scalar-plane session
  bool tile;        // DispatchParams::tile_chunk set: the per-tile append is asked for
  bool tile_ok;     // ... and its fields are usable: counters set, 1 .. kTileAppendMax tiles, an even chunk capacity
  bool ticket;      // DispatchParams::ticket set: the ticketed form is asked for
  bool ticket_ok;   // ... with a divisor (ticket_waves > 0)
  bool fix;         // DispatchParams::fix set: a deterministic launch
  bool bin_log, bin_list, no_land, cont_mask, final_layer, mono_by_wl;
  bool gate_open;   // prob > 0
  int lens, vis;    // proj.proj_type, proj.visible_range
  uint32_t lat_path, az_type, roll_type, root_profile, source;
  bool spectrum;    // spec_per != 0: the wavelength entry is the ray's block, not a draw
};
inline KernelRequest make_request(const DispatchParams& P, int mode, int geom, bool mono) {
  KernelRequest r;
  r.mode = mode, r.geom = geom, r.mono = mono;
  r.tile = P.tile_chunk != nullptr;
  r.tile_ok = P.tile_cnt != nullptr && P.tile_tiles != 0u && P.tile_tiles <= kTileAppendMax && (P.tile_cap & 1u) == 0u;
  r.ticket = P.ticket != nullptr;
  r.ticket_ok = P.ticket_waves != 0u;
  r.fix = P.fix != nullptr;
  r.bin_log = P.bin_log != 0u, r.bin_list = P.bin_list != nullptr, r.no_land = P.no_land != 0u, r.cont_mask = P.cont_mask != nullptr;
  r.final_layer = P.final_layer != 0u, r.mono_by_wl = P.mono_by_wl != 0u;
  r.gate_open = P.prob > 0.0f;
  r.lens = static_cast<int>(P.proj.proj_type), r.vis = static_cast<int>(P.proj.visible_range);
  r.lat_path = P.lat_path, r.az_type = P.az_type, r.roll_type = P.roll_type, r.root_profile = P.root_profile, r.source = P.source;
  r.spectrum = P.spec_per != 0u;
  return r;
}

// `r` with the per-tile append asked for over usable tile fields, in its static or its ticketed form: what halo_backend.cpp bind_tile_append
// asks the selector before it reserves the chunks
constexpr KernelRequest tile_request(KernelRequest r, bool ticket) {
  r.tile = r.tile_ok = true;
  r.ticket = r.ticket_ok = ticket;
  return r;
}

// ---- the selector -----------------------------------------------------------------------------------------------------------------------------
struct Selection {
  KernelId id;
  int err = 0;   // 0: `id` is the launch's kernel; else kSelect*, and no kernel
};
constexpr Selection select_error(int err) {
  Selection s;
  s.err = err;
  return s;
}
// `k` if it exists, else the error: what the selector returns where it does not fall back
constexpr Selection select_exact(const KernelId& k) {
  Selection s;
  s.id = k;
  s.err = kernel_exists(k) ? 0 : kSelectNotSupported;
  return s;
}
// the most special existing form of `k`: with the request's root profile and ticket, then without the profile, then `k` itself
constexpr KernelId with_root(KernelId k, const KernelRequest& r) {
  // a profile is taken only when the record itself says what the profile assumes: a record that does not runs the generic root generation
  const bool lut_uniform = r.lat_path == kLatLut && r.az_type == HALO_DIST_UNIFORM && r.roll_type == HALO_DIST_UNIFORM;
  const int form = !lut_uniform                                                                   ? kRootAny
                   : (r.root_profile == kRootProfileGen && r.source == kSrcGen && !r.spectrum)    ? kRootGenLutUniform
                   : (r.root_profile == kRootProfileTransit && r.source == kSrcTransit)           ? kRootTransitLutUniform
                                                                                                  : kRootAny;
  const int ticket = r.ticket ? kRootTicket : 0;
  const int tries[3] = {form + ticket, kRootAny + ticket, form};
  for (int root : tries) {
    KernelId t = k;
    t.root = root;
    if (kernel_exists(t)) return t;
  }
  return k;
}
// lens, visible range (and, NOGATE, the closed gate) as constants where the request's are ones that exist as such, else the generic form
constexpr KernelId with_lens(KernelId k, const KernelRequest& r, bool nogate) {
  if ((nogate && r.gate_open) || !lens_constant(r.lens) || !vis_constant(r.vis)) return k;
  KernelId t = k;
  t.lens = r.lens, t.vis = r.vis, t.nogate = nogate;
  return kernel_exists(t) ? with_root(t, r) : k;
}

constexpr Selection select_kernel(const KernelRequest& r) {
  KernelId k;
  k.mode = r.mode, k.geom = r.geom, k.mono = r.mono;
  // The per-tile append: its kernel, or an error — the host asks for the route only where one exists (halo_backend.cpp bind_tile_append asks
  // this function).
  if (r.tile) {
    if (r.mode != kModePlain) return select_error(kSelectNotSupported);
    if (r.ticket && !r.ticket_ok) return select_error(kSelectNotSupported);
    if (!r.tile_ok || !r.final_layer || !r.bin_log || r.gate_open || r.cont_mask || r.no_land || r.fix || r.mono_by_wl) return select_error(kSelectNotSupported);
    k.acc = kAccTileFinal, k.lens = r.lens, k.vis = r.vis, k.nogate = true;
    if (!kernel_exists(k)) return select_error(kSelectNotSupported);
    k = with_root(k, r);
    return (r.ticket && !root_ticketed(k.root)) ? select_error(kSelectNotSupported) : select_exact(k);   // a ticket, and no ticketed twin
  }
  if (r.mode < kModePlain || r.mode > kModeColor) return select_error(kSelectInvalidValue);
  const bool fast = mode_fast(r.mode);
  // a one-shape layer whose every exit continues accumulates nothing: no cache, no queue, no accumulation code — in a deterministic session too
  const bool none = r.no_land && fast && geom_one(r.geom);
  // a deterministic launch that accumulates: its fixed-point kernel, or an error — never a float route
  if (r.fix && !none) {
    k.geom = (r.geom == kGeomOneHex || r.geom == kGeomPoolPrism || r.geom == kGeomPool) ? r.geom : kGeomOne;
    k.acc = r.bin_log ? kAccFixedLog : kAccFixed;
    k.canon = r.cont_mask;   // (kAccFixedLog has no CANON twin: a canonical layer before the last never logs)
    return select_exact(k);
  }
  // the regular prism's instantiation: the production modes' direct and logged routes — not the binned lists
  if (r.geom == kGeomOneHex && !(fast && (!r.bin_list || r.bin_log || r.no_land))) k.geom = kGeomOne;
  if (k.geom != kGeomOneHex && k.geom != kGeomPoolPrism && k.geom != kGeomPool) k.geom = kGeomOne;
  const bool one = geom_one(k.geom);
  if (r.cont_mask) {
    k.canon = true;
    if (none) k.mono = true, k.acc = kAccNone;
    return select_exact(k);
  }
  if (none) {
    k.mono = true, k.acc = kAccNone;
    return select_exact(k);
  }
  if (fast && r.bin_log) {
    if (one && r.mono && r.final_layer) {
      k.acc = kAccLogFinal;
      return select_exact(with_lens(k, r, true));
    }
    k.acc = kAccLog;
    if (!one) {   // the shape-pool kernels: the whole render as constants, or (X/Y/Z planes) the full sky and the closed gate alone
      if (!r.gate_open && r.vis == HALO_VISIBLE_FULL) {
        KernelId t = k;
        t.lens = r.lens, t.vis = r.vis, t.nogate = true;
        if (kernel_exists(t)) return select_exact(t);
        t.lens = -1;
        if (kernel_exists(t)) return select_exact(t);
      }
      return select_exact(k);
    }
    return select_exact(r.mono ? with_lens(k, r, false) : k);
  }
  k.acc = (r.mono && r.bin_list && k.geom != kGeomOneHex) ? kAccBin : kAccDirect;
  return select_exact(k);
}

// ---- the expander -----------------------------------------------------------------------------------------------------------------------------
// The values ROOT takes anywhere in the kernel set (kernel_exists picks among the product of every argument's values; LENS and VIS: -1 and
// what lens_constant / vis_constant name).
constexpr int kRootValues[] = {kRootAny, kRootGenLutUniform, kRootTransitLutUniform, kRootTicket + kRootAny, kRootTicket + kRootGenLutUniform, kRootTicket + kRootTransitLutUniform};

// The kernels of one family, in the order of the loops below.
template <int FAMILY>
struct FamilyTable {
  static constexpr int kMax = 256;
  struct Ids {
    KernelId id[kMax];
    int n;
  };
  static constexpr Ids make() {
    Ids t{};
    for (int geom = kGeomOne; geom <= kGeomOneHex; geom++)
      for (int mono = 0; mono < 2; mono++)
        for (int acc = kAccDirect; acc <= kAccTileFinal; acc++) {
          if (family_of(KernelId{family_mode(FAMILY), geom, mono != 0, acc}) != FAMILY) continue;
          for (int canon = 0; canon < 2; canon++)
            for (int lens = -1; lens <= HALO_LENS_GLOBE; lens++) {
              if (lens >= 0 && !lens_constant(lens)) continue;
              for (int vis = -1; vis <= HALO_VISIBLE_FULL; vis++) {
                if (vis >= 0 && !vis_constant(vis)) continue;
                for (int nogate = 0; nogate < 2; nogate++)
                  for (int root : kRootValues) {
                    const KernelId k{family_mode(FAMILY), geom, mono != 0, acc, lens, vis, nogate != 0, canon != 0, root};
                    if (kernel_exists(k)) t.id[t.n++] = k;   // (more than kMax: not a constant expression, a compile error)
                  }
              }
            }
        }
    return t;
  }
  static constexpr Ids ids = make();
};

template <int FAMILY, typename F, typename Seq>
struct FamilyThunks;
template <int FAMILY, typename F, size_t... I>
struct FamilyThunks<FAMILY, F, std::index_sequence<I...>> {
  template <size_t K>
  static void call(F& f) {
    constexpr KernelId k = FamilyTable<FAMILY>::ids.id[K];
    f(KernelConst<k.mode, k.geom, k.mono, k.acc, k.lens, k.vis, k.nogate, k.canon, k.root>{});
  }
  static constexpr void (*fn[])(F&) = {&call<I>...};
};
// f(KernelConst<...>{}) for the kernel `id` of family FAMILY; false (and no call) if the family has no such kernel
template <int FAMILY, typename F>
bool expand_kernel(const KernelId& id, F&& f) {
  using Fn = typename std::remove_reference<F>::type;
  constexpr const auto& T = FamilyTable<FAMILY>::ids;
  for (int i = 0; i < T.n; i++)
    if (T.id[i] == id) {
      FamilyThunks<FAMILY, Fn, std::make_index_sequence<static_cast<size_t>(T.n)>>::fn[i](f);
      return true;
    }
  return false;
}

}  // namespace halo

#endif
