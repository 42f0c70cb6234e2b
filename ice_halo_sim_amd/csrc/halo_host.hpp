// halo_host.hpp — host-side producers of the tables the gfx950 kernels consume: crystal geometry, latitude
// LUT, projection POD, wavelength pool, ray partition.  Plain C++17, no device code, no torch.
#ifndef HALO_HOST_HPP_
#define HALO_HOST_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <vector>

#include "halo_device.h"
#include "halo_geom.h"

namespace halo {
namespace host {

// math.hpp:21-31 constants (float, as the reference evaluates them)
constexpr float kPi = 3.14159265359f;
constexpr float kPiHalf = kPi / 2.0f;
constexpr float kFloatEps = 1e-5f;
constexpr float kDegToRad = kPi / 180.0f;
constexpr float kSqrt3 = 1.73205080757f;

// Closed-form hexagonal prism → kernel tables. Returns false for the empty crystal
// (Crystal::MakePrismClosedForm crystal.cpp:349-368).
bool BuildPrism(float h, const float dist[6], HaloGeomTables& out);
bool BuildPyramid(float wedge_u_deg, float wedge_l_deg, float h1, float h2, float h3, const float dist[6],
                  HaloGeomTables& out);
void ToShapeDev(const HaloGeomTables& g, ShapeDev& out);
void FromShapeDev(const ShapeDev& s, HaloGeomTables& out);
geom::CrystalRecipe MakeRecipe(const HaloCrystal& c);   // wedge trig evaluated once, on the host

struct LatLut {
  std::array<float, kLutNodes> theta{}, cdf{}, flip{};
};
LatLut BuildLatLut(const HaloDist& latitude);               // lat_lut.cpp:74-204
uint32_t SelectLatPath(const HaloAxis& axis);               // lat_path_selection.hpp:62-75

ProjDev BuildProj(const HaloRender& render);                // lens_proj_build.hpp:79-137
double IceRefractiveIndex(double wavelength_nm);            // optics.cpp:180-197
float IlluminantSpd(int illuminant, float wavelength_nm);   // util/illuminant.cpp:113-134
std::vector<WlEntryDev> BuildWlPool(const HaloWl& wl);      // wl_pool.hpp:67-91
std::vector<uint64_t> Partition(const float* proportions, int n, uint64_t ray_num, double* carry);  // simulator.cpp:519-582

// Emit-gate filter descriptor: BuildDeviceFilterDesc / BuildComplexSubDescs (device_filter_desc.cpp:121-170) with the
// canonical sequences reduced by Crystal::ReduceRaypath (crystal.cpp:536-600).
FilterDev BuildFilter(const HaloFilter& f, const HaloAxis& axis);
std::vector<uint8_t> ReduceRaypath(const std::vector<uint8_t>& rp, uint8_t symmetry, int sigma_a, bool d_applicable);
// Fast form of a filter (nullptr = none) and of a crystal entry's colour predicates for the kernels that hold the path in a
// 128-bit register (halo_device.h FastTables).  false = it does not fit (member / matrix pools full): the caller takes the
// generic kernels.  `crystal_id`: the dispatch's crystal (crystal terms are constants of the dispatch and fold into len_mode).  The class table
// of `out` is the caller's.
bool BuildFastTables(const HaloFilter* filter, const HaloColorSet* colors, const HaloAxis& axis, uint32_t crystal_id, FastTables& out);
// The members of a raypath term: every sequence whose reduction equals `canon` (packed {hi, lo}, newest face in the low byte).
std::vector<std::array<uint64_t, 2>> RaypathMembers(const std::vector<uint8_t>& canon, uint8_t symmetry, int sigma_a, bool d_applicable);
// The fast tables evaluated on the host, step for step like halo_trace.inl fast_filter (test hook).
bool FastFilterCheck(const FastTables& F, const uint8_t* path, uint32_t len, const float dir[3], uint32_t crystal_id);
// the colour pass of the production colour kernels (fast_color_bits) on the host: carried | bits of the matching predicates
uint64_t FastColorMask(const FastTables& F, uint64_t carried, const uint8_t* path, uint32_t len, const float dir[3], uint32_t crystal_id);
int ComputeSigmaA(float roll_center_deg);       // crystal.cpp:720-726
bool IsDApplicable(const HaloAxis& axis);       // crystal.cpp:728-730

bool IsDeterministic(const HaloCrystal& c);                 // simulator.cpp:453-471
// One sampled crystal instance (MakeCrystal simulator.cpp:448 with SyncGroupSampler :361-393), shape scalars
// drawn from the host PCG stream (seed, shape_index).
bool MakeShape(uint32_t seed, const HaloCrystal& c, uint64_t shape_index, HaloGeomTables& out);
bool MakeShapeDev(uint32_t seed, const HaloCrystal& c, uint64_t shape_index, ShapeDev& out);   // same, device table layout

// Tables of the fast entry pick (EntryFastDev); false = the shape is not a full prism in the expected layout.
bool BuildEntryFast(const ShapeDev& s, EntryFastDev& out);

uint32_t PcgHash(uint32_t x);

// The host halves of halo_consumer_stats (halo_stats.hip).  PercentileRank: numpy's default ("linear") rule, vi = (percentile / 100) * (n - 1) in
// float64 with one product, rank = floor(vi), frac = vi - rank; false for a percentile outside [0, 100], n = 0 or a null pointer.
bool PercentileRank(double percentile, uint64_t n, uint64_t* rank, double* frac);
// The sum of positive floats (squares = false: bins[256], per exponent field the sum of the 24-bit significands) or of their exact squares
// (squares = true: bins[512], per exponent field the sums of the low and of the high 24 bits of the squared significands), rounded ONCE, to
// nearest even, from a fixed-width big integer.  +inf when the top exponent field holds anything.
double BinnedSum(const uint64_t* bins, bool squares);

// The host half of halo_consumer_view: the world exit direction the lens of `view` puts on the centre of pixel (px, py) — halo_view.h
// view_direction on BuildProj(view), the code halo_view_kernel runs.  false (and zeros) where the pixel has no direction or lies outside the frame.
bool ViewDirection(const HaloRender& view, int px, int py, float dir[3]);
// ... and of halo_consumer_view_filtered: where the exit direction `dir` lands under `source`, continuous — halo_view.h view_source_pos on
// BuildProj(source): {fx0, fy0, fx1, fy1, t}, the hit count returned (0 and zeros: culled, or an unknown lens).
int ViewSourcePos(const HaloRender& source, const float dir[3], float pos[5]);
// ... and of halo_consumer_view_overlay (halo_overlay.h): the reference's default record for a view of `fov` degrees and a sun at (alt, az) degrees;
// what the calls refuse in a record (nullptr: nothing; else the message's tail); the three marks {x, y, present} of zenith, nadir and sun under
// `view`, ViewSourcePos's primary hits; {alt, az, dist} of a direction; the value of one pixel that has a direction.
void ViewOverlayDefaults(float fov, const float sun_alt_az_deg[2], HaloViewOverlay* out);
const char* ViewOverlayRefusal(const HaloViewOverlay& o);
void ViewOverlayMarks(const HaloRender& view, const float sun_dir[3], float marks[9]);
void ViewSky(const float dir[3], const float sun_dir[3], float sky[3]);
void ViewOverlayPixel(const uint8_t base_rgb[3], const float sky[6], const float pixel_xy[2], const float marks[9], const HaloViewOverlay& o, float value[3]);

}  // namespace host

// ---- rules the backend applies and halo_host_abi.cpp exports for the tests: one definition ----

// Fractional bits of the per-tile fixed-point sums for a launch of `m` rays whose weights are at most `max_w`: the largest F <= 32 with
// 4 * max_w * m * 2^F < 2^62 (see halo_kernels.hip FixQ for the factor 4).
// The deterministic route applies the same bound to the rays a plane set may take before it is folded (kFixBudgetHits) and to the landed integer
// (kFixLandedHits): halo_host_fixed_frac_bits exports the rule.
inline uint32_t fix_frac_bits(double max_w, uint64_t m) {
  const double bound = 4.0 * std::max(max_w, 1e-30) * static_cast<double>(std::max<uint64_t>(m, 1));
  int e = 0;
  (void)std::frexp(bound, &e);   // bound < 2^e
  return static_cast<uint32_t>(std::min(32, std::max(0, 62 - e)));
}

// Rays one unfolded fixed-point plane set takes (F = 29 for weights up to 1: a hit is quantised to 1.9e-9): a constant, because F must not depend
// on how a run is cut into launches or sessions.  The landed integer's scale allows for the 2^32 rays of the largest layer.
constexpr uint64_t kFixBudgetHits = 1ull << 30, kFixLandedHits = 1ull << 32;

// Shard `index` of `count` takes rays [first, first + n) of a crystal entry's share: the share is cut in units of `clock` rays (the rays of one
// sampled shape; 1 for a fixed one), u = ceil(share / clock) of them, and the shard gets units [floor(index * u / count), floor((index + 1) * u / count)) —
// the last unit may be short.  Every shard gets a part of every entry, the parts differ by at most one unit, no unit is cut.
inline void shard_slice(uint64_t share, uint32_t clock, uint32_t index, uint32_t count, uint64_t* first, uint64_t* n) {
  typedef unsigned __int128 u128;
  const u128 c = clock ? clock : 1u, u = (static_cast<u128>(share) + c - 1u) / c;
  const u128 lo = std::min<u128>(c * (static_cast<u128>(index) * u / count), share), hi = std::min<u128>(c * ((static_cast<u128>(index) + 1u) * u / count), share);
  *first = static_cast<uint64_t>(lo);
  *n = static_cast<uint64_t>(hi - lo);
}

}  // namespace halo

#endif
