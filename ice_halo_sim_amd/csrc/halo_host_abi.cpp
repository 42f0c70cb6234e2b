// halo_host_abi.cpp — every export of include/halo_trace.h that takes no handle: the ABI's version and struct sizes, and the host-side rules and
// table producers (halo_host_*) the tests compare against the reference without a device.  No HIP call; what an export shares with the backend or
// the kernels — the ticket and spectrum rules of halo_device.h, fix_frac_bits and shard_slice of halo_host.hpp — has its one definition there.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "halo_device.h"
#include "halo_host.hpp"

using namespace halo;

extern "C" {

int halo_abi_version(void) { return HALO_ABI_VERSION; }

uint32_t halo_host_spectrum_entry(uint64_t m, uint32_t count, uint64_t r) {
  // The kernels' own function, given what the host would hand a launch that holds ray r — two ways: the launch that starts as late as a 32-bit
  // thread index allows (a long way into the launch, across many block edges), and one that starts at a multiple of 65521 rays (an offset in the
  // middle of a block).  They must agree; 0xFFFFFFFF says they did not.
  const uint64_t reach = 0xFFFFFFFEull, off_a = r > reach ? r - reach : 0ull, off_b = r - r % 65521ull;
  const SpectrumChunkDev a = SpectrumChunk(m, count, off_a), c = SpectrumChunk(m, count, off_b);
  const uint32_t ka = SpectrumEntry(a.per, a.k0, a.rem, a.last, static_cast<uint32_t>(r - off_a));
  const uint32_t kb = SpectrumEntry(c.per, c.k0, c.rem, c.last, static_cast<uint32_t>(r - off_b));
  return ka == kb ? ka : 0xFFFFFFFFu;
}

uint32_t halo_host_fixed_frac_bits(double max_w, uint64_t hits) { return fix_frac_bits(max_w, hits); }

// The ticket rule the ticketed kernels apply (halo_device.h TicketSize), for tests/test_ticket_size.py: no device needed.
uint32_t halo_host_ticket_size(uint32_t total, uint32_t seen, uint32_t waves, uint32_t lo, uint32_t hi) { return TicketSize(total, seen, waves, lo, hi); }
// ... and the ranges of a launch's passes with a counter each, and the range a wave turns to (TicketRangeOf, TicketNextRange)
uint32_t halo_host_ticket_groups(void) { return kTicketGroups; }
void halo_host_ticket_range(uint32_t all, uint32_t g, uint32_t* first, uint32_t* n) {
  const TicketRange r = TicketRangeOf(all, g);
  if (first) *first = r.first;
  if (n) *n = r.n;
}
uint32_t halo_host_ticket_next(uint64_t open, uint32_t home) { return open ? TicketNextRange(open, home) : kTicketGroups; }

int halo_host_shard_slice(uint64_t share, uint32_t clock, uint32_t index, uint32_t count, uint64_t* first, uint64_t* n) {
  if (!first || !n || clock == 0u || count == 0u || index >= count) return HALO_FATAL;
  shard_slice(share, clock, index, count, first, n);
  return HALO_OK;
}

// ---- auto exposure (gui/gui_ev_auto.hpp) ---------------------------------------------------------------------
float halo_host_ev_auto(float p99_y, float per_pixel_intensity, float target_white) {   // ComputeEvAuto, gui_ev_auto.hpp:143-155
  if (per_pixel_intensity <= 0.0f || p99_y <= 0.0f) return 0.0f;
  const float p99_norm = p99_y / per_pixel_intensity;
  const float t = target_white / 255.0f;
  const float target_linear = t <= 0.04045f ? t / 12.92f : std::pow((t + 0.055f) / 1.055f, 2.4f);
  if (target_linear <= 0.0f || p99_norm <= 0.0f) return 0.0f;
  const float ev = std::log2f(target_linear / p99_norm);
  return std::min(std::max(ev, -6.0f), 6.0f);
}

// ---- image statistics (halo_stats.hip) --------------------------------------------------------------------------
int halo_host_percentile_rank(double percentile, uint64_t n, uint64_t* rank, double* frac) {
  return host::PercentileRank(percentile, n, rank, frac) ? HALO_OK : HALO_FATAL;
}
int halo_host_binned_sum(const uint64_t* bins, int32_t squares, double* out) {
  if (!bins || !out) return HALO_FATAL;
  *out = host::BinnedSum(bins, squares != 0);
  return HALO_OK;
}

// ---- the view stage (halo_view.hip): the consumer's image through another lens -------------------------------
int halo_host_view_direction(const HaloRender* view, int32_t px, int32_t py, float dir[3]) {
  if (!view || !dir) return 0;
  return host::ViewDirection(*view, px, py, dir) ? 1 : 0;
}
int halo_host_view_source_pos(const HaloRender* source, const float dir[3], float pos[5]) {
  if (pos) pos[0] = pos[1] = pos[2] = pos[3] = pos[4] = 0.0f;
  if (!source || !dir || !pos) return 0;
  return host::ViewSourcePos(*source, dir, pos);
}
int halo_host_view_overlay_defaults(float view_fov_deg, const float sun_alt_az_deg[2], HaloViewOverlay* out) {
  if (!out) return 0;
  host::ViewOverlayDefaults(view_fov_deg, sun_alt_az_deg, out);
  return static_cast<int>(sizeof(HaloViewOverlay));
}
int halo_host_view_sky(const float dir[3], const float sun_dir[3], float sky3[3]) {
  if (sky3) sky3[0] = sky3[1] = sky3[2] = 0.0f;
  if (!dir || !sun_dir || !sky3) return 0;
  host::ViewSky(dir, sun_dir, sky3);
  return 1;
}
int halo_host_view_overlay_pixel(const uint8_t base_rgb[3], const float sky6[6], const float pixel_xy[2], const float marks9[9], const HaloViewOverlay* overlay,
                                 float value3[3]) {
  if (value3) value3[0] = value3[1] = value3[2] = 0.0f;
  if (!base_rgb || !sky6 || !pixel_xy || !marks9 || !overlay || !value3) return 0;
  if (overlay->sun_circle_count < 0 || overlay->sun_circle_count > HALO_VIEW_MAX_SUN_CIRCLES) return 0;   // (the one field that bounds a loop over the record)
  host::ViewOverlayPixel(base_rgb, sky6, pixel_xy, marks9, *overlay, value3);
  return 1;
}

// ---- display-side composite of the class lanes (server/component_compositor.cpp) -------------------------
int halo_host_parse_composite_mode(const char* mode) {   // ParseCompositeMode, component_compositor.cpp:118-134
  if (mode && std::strcmp(mode, "dominant") == 0) return HALO_COMPOSITE_DOMINANT;
  if (mode && std::strcmp(mode, "additive") == 0) return HALO_COMPOSITE_ADDITIVE;
  return HALO_COMPOSITE_PAINTER;
}

// ---- host-side pieces, exported for parity tests -------------------------------------------------------
int halo_host_prism_geometry(float h, const float dist[6], HaloGeomTables* out) {
  if (!out || !dist) return HALO_FATAL;
  host::BuildPrism(h, dist, *out);
  return HALO_OK;
}
int halo_host_pyramid_geometry(float wu, float wl, float h1, float h2, float h3, const float dist[6], HaloGeomTables* out) {
  if (!out || !dist) return HALO_FATAL;
  return host::BuildPyramid(wu, wl, h1, h2, h3, dist, *out) ? HALO_OK : HALO_UNAVAILABLE;
}
int halo_host_shape_scalars(const HaloCrystal* crystal, uint32_t seed, uint64_t shape_index, int via_plan, float out9[9]) {
  if (!crystal || !out9) return HALO_FATAL;
  const geom::CrystalRecipe rc = host::MakeRecipe(*crystal);
  if (via_plan) {
    for (int q = 0; q < 9; q++) out9[q] = geom::DrawShapeScalarOne(seed, rc, shape_index, q);
  } else {
    geom::DrawShapeScalars(seed, rc, shape_index, out9);
  }
  return HALO_OK;
}
int halo_host_build_lat_lut(const HaloDist* lat, float* theta, float* cdf, float* flip) {
  if (!lat || !theta || !cdf || !flip) return HALO_FATAL;
  host::LatLut l = host::BuildLatLut(*lat);
  std::copy(l.theta.begin(), l.theta.end(), theta);
  std::copy(l.cdf.begin(), l.cdf.end(), cdf);
  std::copy(l.flip.begin(), l.flip.end(), flip);
  return HALO_OK;
}
int halo_host_build_proj_params(const HaloRender* render, void* out76) {
  if (!render || !out76) return HALO_FATAL;
  ProjDev p = host::BuildProj(*render);
  static_assert(sizeof(ProjDev) == 76, "ProjDev mirrors lm_proj::ProjParams");
  std::memcpy(out76, &p, sizeof(p));
  return HALO_OK;
}
int halo_host_partition(const float* prop, int n, uint64_t ray_num, double* carry, uint64_t* out) {
  if (!prop || !carry || !out || n < 0) return HALO_FATAL;
  std::vector<uint64_t> v = host::Partition(prop, n, ray_num, carry);
  std::copy(v.begin(), v.end(), out);
  return HALO_OK;
}
int halo_host_reduce_raypath(const uint8_t* rp, int32_t n, int32_t symmetry, int32_t sigma_a, int32_t d_applicable, uint8_t* out) {
  if (!rp || !out || n < 0 || n > HALO_MAX_HITS) return HALO_FATAL;
  std::vector<uint8_t> v = host::ReduceRaypath(std::vector<uint8_t>(rp, rp + n), static_cast<uint8_t>(symmetry), sigma_a, d_applicable != 0);
  std::copy(v.begin(), v.end(), out);
  return HALO_OK;
}
int halo_host_filter_fast_check(const HaloFilter* f, const HaloAxis* axis, const uint8_t* path, int32_t n, const float dir[3], int32_t crystal_id, int32_t* pass) {
  if (!f || !axis || !pass || n < 0 || n > 16 || (n && !path) || !dir) return HALO_FATAL;
  // the tables of the (filter, axis) asked about last are kept: the tests sweep thousands of paths per filter
  struct Cache {
    HaloFilter f;
    HaloAxis axis;
    int32_t crystal_id = 0;
    bool valid = false, fits = false;
    FastTables tables;
  };
  static thread_local std::unique_ptr<Cache> cache;
  if (!cache) cache.reset(new Cache());
  if (!cache->valid || std::memcmp(&cache->f, f, sizeof(HaloFilter)) != 0 || std::memcmp(&cache->axis, axis, sizeof(HaloAxis)) != 0 || cache->crystal_id != crystal_id) {
    std::memset(&cache->tables, 0, sizeof(FastTables));
    cache->f = *f;
    cache->axis = *axis;
    cache->crystal_id = crystal_id;
    cache->fits = host::BuildFastTables(f, nullptr, *axis, static_cast<uint32_t>(crystal_id), cache->tables);
    cache->valid = true;
  }
  if (!cache->fits) return HALO_FATAL;
  *pass = host::FastFilterCheck(cache->tables, path, static_cast<uint32_t>(n), dir, static_cast<uint32_t>(crystal_id)) ? 1 : 0;
  return HALO_OK;
}
int halo_host_color_fast_mask(const HaloColorSet* colors, const HaloAxis* axis, const uint8_t* path, int32_t n, const float dir[3], int32_t crystal_id, uint64_t carried,
                              uint64_t* mask) {
  if (!colors || !axis || !mask || n < 0 || n > 16 || (n && !path) || !dir) return HALO_FATAL;
  std::unique_ptr<FastTables> tables(new FastTables());
  std::memset(tables.get(), 0, sizeof(FastTables));
  if (!host::BuildFastTables(nullptr, colors, *axis, static_cast<uint32_t>(crystal_id), *tables)) return HALO_FATAL;
  *mask = host::FastColorMask(*tables, carried, path, static_cast<uint32_t>(n), dir, static_cast<uint32_t>(crystal_id));
  return HALO_OK;
}
double halo_host_refractive_index(double wl) { return host::IceRefractiveIndex(wl); }
float halo_host_illuminant_spd(int illuminant, float wl) { return host::IlluminantSpd(illuminant, wl); }
int halo_host_wl_pool(const HaloWl* wl, float* entries5, int cap) {
  if (!wl || !entries5 || cap < 0) return 0;
  const std::vector<WlEntryDev> pool = host::BuildWlPool(*wl);
  for (size_t m = 0; m < pool.size() && static_cast<int>(m) < cap; m++) {
    float* e = entries5 + 5 * m;
    e[0] = pool[m].n_idx;
    e[1] = pool[m].spd_weight;
    e[2] = pool[m].cmf_x;
    e[3] = pool[m].cmf_y;
    e[4] = pool[m].cmf_z;
  }
  return static_cast<int>(pool.size());
}

// sizes of the boundary structs, for the Python layout check
uint64_t halo_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(HaloScene);
    case 1: return sizeof(HaloRender);
    case 2: return sizeof(HaloWl);
    case 3: return sizeof(HaloExitRecord);
    case 4: return sizeof(HaloGeomTables);
    case 5: return sizeof(HaloLayerStats);
    case 6: return sizeof(HaloEntry);
    case 7: return sizeof(HaloColorSet);
    case 8: return sizeof(HaloColorClass);
    case 9: return sizeof(HaloFilter);
    case 10: return sizeof(HaloRouteInfo);
    case 11: return sizeof(HaloComposite);
    case 12: return sizeof(HaloAutoEv);
    case 13: return sizeof(HaloStatsSpec);
    case 14: return sizeof(HaloImageStats);
    case 15: return sizeof(HaloViewSpec);
    case 16: return sizeof(HaloViewFilter);
    default: return 0;
  }
}

}  // extern "C"
