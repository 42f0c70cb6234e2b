// halo_launch.h — the host-side launchers of the kernels (namespace halo), declared once: halo_backend.cpp calls them, halo_kernels.hip and
// halo_shapegen.hip define them, tests/cpp/passes_shim.cpp hands them synthetic records.  A signature that drifts is a compile error.
#ifndef HALO_LAUNCH_H_
#define HALO_LAUNCH_H_

#include <hip/hip_runtime.h>

#include "halo_device.h"
#include "halo_select.h"

namespace halo {
namespace geom {
struct CrystalRecipe;
}

// (the kernel is halo_select.h select_kernel's choice for the request; `launched` receives it where the launch is made)
hipError_t launch_trace(const DispatchParams& P, int blocks, hipStream_t stream, int mode, int geom, bool mono, KernelId* launched = nullptr);
// workgroups of a ticketed kAccTileFinal kernel (DispatchParams::ticket) that one CU holds at once: the occupancy query, made once
int tile_ticket_resident_per_cu();
hipError_t launch_bin_accumulate(float* plane, const HitRec* list, uint32_t cap, uint32_t* cnt, uint32_t tiles, uint32_t frac_bits, hipStream_t stream);
hipError_t launch_bin_two_level(float* plane, const HitRec* list1, uint32_t cap1, uint32_t* cnt1, uint32_t lists1, HitRec* list2, uint32_t cap2,
                                uint32_t* cnt2, uint32_t tiles, uint32_t fan_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, hipStream_t stream, hipEvent_t before_sums);
hipError_t launch_log_route(float* plane, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2, uint32_t cap2, uint32_t* cnt2,
                            uint32_t tiles, uint32_t planes, uint32_t s_log2, bool interleaved, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, uint32_t copies_log2, hipStream_t stream,
                            hipEvent_t before_sums);
hipError_t launch_log_route_xyz(float* planes, uint32_t plane_stride, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, const WlEntryDev* pool, uint32_t pool_size, uint32_t frac_bits,
                                double* ovf, uint32_t* ovf_flag, uint32_t copies_log2, hipStream_t stream, hipEvent_t before_sums);
// (a launch that is its whole session, contiguous-tile scalar route: the per-tile pass adds coef x sum to the image itself — no plane, no fold)
hipError_t launch_log_route_close(float* xyz, uint32_t n_pix, const float* coef, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                  uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag,
                                  hipStream_t stream, hipEvent_t before_sums);
// (the same close over the per-tile chunks of a kAccTileFinal trace kernel of `wgs` workgroups: chunk[tiles][wgs][cap], cnt[tiles][wgs]; no split pass)
hipError_t launch_tile_route_close(float* xyz, uint32_t n_pix, const float* coef, const HitRec* chunk, uint32_t cap, const uint32_t* cnt, uint32_t wgs, uint32_t tiles,
                                   uint32_t s_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, hipStream_t stream, hipEvent_t before_sums,
                                   uint32_t* ticket = nullptr);   // ticket: a ticketed trace kernel's counter, which the pass returns to zero (halo_device.h TicketSize)
// (the deterministic route's log: integer planes, the session's F, atomics only — no fp64 twin, no ordering event)
hipError_t launch_log_route_fixed(unsigned long long* fix, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2, uint32_t cap2,
                                  uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, bool interleaved, uint32_t frac_bits, hipStream_t stream);
hipError_t launch_log_route_xyz_fixed(unsigned long long* fix, uint32_t plane_stride, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                      uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, const WlEntryDev* pool, uint32_t pool_size, uint32_t frac_bits,
                                      hipStream_t stream);
hipError_t launch_shapegen(void* pool, bool prism_records, uint32_t n, uint32_t seed, const geom::CrystalRecipe& rc, uint64_t first_index,
                           hipStream_t stream, bool serial_pyramid);
hipError_t launch_fold(float* xyz, float* planes, uint32_t n_pix, uint32_t s_log2, uint32_t copies, uint32_t n_planes, const FoldCoef& coef,
                       double* ovf, const uint32_t* ovf_flag, hipStream_t stream);
hipError_t launch_fold_fixed(float* xyz, unsigned long long* planes, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, const FoldCoef& coef, uint32_t frac_bits,
                             hipStream_t stream);
// (halo_export_fixed / halo_import_fixed: the fixed-point planes [plane][slot] out to / in from n_planes * n_pix words in pixel order; the export
//  zeroes what it takes and writes `landed` as word n_planes * n_pix, the import adds modulo 2^64)
hipError_t launch_export_fixed(unsigned long long* planes, unsigned long long* words, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, unsigned long long landed,
                               hipStream_t stream);
hipError_t launch_import_fixed(unsigned long long* planes, const unsigned long long* words, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, hipStream_t stream);
hipError_t launch_consumer_fold(float* acc, float* sum, float* comp, uint32_t n, int blocks, hipStream_t stream);
hipError_t launch_lane_hist(const double* lanes, uint32_t n_pix, const CompositeDev& cd, uint32_t shift, uint32_t bits, uint32_t prefix, uint32_t* hist, int blocks,
                            hipStream_t stream);
hipError_t launch_composite(const double* lanes, uint32_t n_pix, const CompositeDev& cd, float* rgb_out, uint8_t* srgb_out, int blocks, hipStream_t stream);
hipError_t launch_lanes_load(const float* src, double* lanes, uint64_t n, int blocks, hipStream_t stream);
hipError_t launch_lanes_drain(double* lanes, float* dst, uint64_t n, int blocks, hipStream_t stream);
hipError_t launch_lanes_add(const float* src, double* lanes, uint64_t n, int blocks, hipStream_t stream);
hipError_t launch_post_snapshot(const float* sum, const float* comp, uint8_t* rgb_out, float* xyz_out, uint32_t n_pix, float scale,
                                const float ray_color[3], const float background[3], int blocks, hipStream_t stream);
// halo_autoev.hip — the auto-exposure stage.  AevRecord is what the select leaves in device memory: the count of positive values, the index the
// reference's rule picks among them, the bit pattern of that order statistic (0 when count is 0); prefix / rank carry the select from pass to pass.
struct AevRecord {
  uint32_t count, idx, p99_bits, prefix, rank, reserved[3];
};
constexpr uint32_t kAevHistWords = 3u * 2048u;   // the multi-block select's three global histograms
// up to this many values one workgroup does the whole select: measured, it is 10-20 us ahead of the seven launches of the multi-block select up
// to 16 Ki values, level with them at 32 400 (the production shape) and 25 us behind at 64 Ki (profiles/auto_ev_cost.txt)
constexpr uint32_t kAevSmallMax = 1u << 15;
// (wc, hc > 0: box sums of f x f pixels into vals[wc * hc]; wc = hc = 0: the fine path, Y of every pixel into vals[width * height])
hipError_t launch_aev_values(const float* sum, const float* comp, uint32_t width, uint32_t height, uint32_t f, uint32_t wc, uint32_t hc, float* vals, int blocks,
                             hipStream_t stream);
hipError_t launch_aev_select(const float* vals, uint32_t n, AevRecord* rec, uint32_t* hist, bool one_workgroup, bool aggregate, int blocks, hipStream_t stream);
// halo_stats.hip — the image-statistics stage: one first sweep (values, first-digit histogram, counts, max, the exponent-binned integer sums of the
// moments), then a radix select of up to kStatsMaxRanks order statistics at once.  StatsAsk is what the caller wants (q = percentile / 100, divided
// on the host), StatsSel the select's state as it travels from kernel to kernel: the count of positive values, the K distinct ranks in ascending
// order — per rank the digits found so far (pref), the rank left inside that prefix and the group it belongs to — and the G distinct prefixes
// (gpref, ascending), one histogram each in the next pass.  StatsRecord is everything the host reads back, once.
constexpr uint32_t kStatsMaxQ = 16u, kStatsMaxRanks = 2u * kStatsMaxQ, kStatsExpBins = 256u;
struct StatsAsk {
  double q[kStatsMaxQ];
  uint32_t count, reserved;
};
struct StatsSel {
  uint32_t n, K, G, reserved;
  uint32_t pref[kStatsMaxRanks], rank[kStatsMaxRanks], group[kStatsMaxRanks], gpref[kStatsMaxRanks];
};
struct StatsRecord {
  StatsSel sel;
  uint32_t sat, max_bits;                                   // values with v / norm > 1; the largest positive bit pattern
  uint32_t idx_lo[kStatsMaxQ], idx_hi[kStatsMaxQ];          // percentile j's two ranks among the K distinct ones
  uint32_t lo_bits[kStatsMaxQ], hi_bits[kStatsMaxQ];        // ... and the order statistics found there
  uint64_t rank[kStatsMaxQ];                                // floor((n - 1) q)
  double frac[kStatsMaxQ];                                  // (n - 1) q - rank
  unsigned long long bins[3u * kStatsExpBins];              // per exponent field: sum of m, of (m * m) & 0xFFFFFF, of (m * m) >> 24 (halo_host_binned_sum)
};
constexpr uint32_t kStatsRecWords = sizeof(StatsRecord) / sizeof(uint32_t);
// the workspace: the record, then the multi-block form's global histograms (first digit; 32 x 2048 second; 32 x 1024 third)
constexpr uint32_t kStatsWsWords = kStatsRecWords + 2048u + kStatsMaxRanks * (2048u + 1024u);
// up to this many values one workgroup does the whole call in one launch: measured with the eleven-percentile call, it is 25-30 us ahead of the
// multi-block form's launches at 1 Ki values, 6-12 us ahead at 8 Ki and 20-33 us behind at 16 Ki (profiles/image_stats_cost.txt) — a quarter
// of kAevSmallMax, because one workgroup here makes up to nine sweeps where auto-EV's makes three
constexpr uint32_t kStatsSmallMax = 1u << 13;
// (lane == nullptr: the values are Y = sum[3 p + 1] + comp[3 p + 1]; else float(lane[p]).  vals: n_pix floats.  ws: kStatsWsWords words)
hipError_t launch_stats(const float* sum, const float* comp, const double* lane, uint32_t n_pix, float norm, const StatsAsk& ask, float* vals, uint32_t* ws,
                        bool one_workgroup, int blocks, hipStream_t stream);
// halo_view.hip — the view stage: per pixel of the `view` projection the direction of its centre (halo_view.h), the pixel of the `source`
// projection that direction lands on (project_exit's primary hit; -1 for none), that pixel's sum + comp and its display transform.  Every output
// may be null: rgb 3 bytes, xyz / dir 3 floats, map one int32 per view pixel.  `blocks` caps the grid; more tiles than that are strided over.
hipError_t launch_view(const float* sum, const float* comp, const ProjDev& view, const ProjDev& source, float scale, const float ray_color[3], const float background[3],
                       uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, int blocks, hipStream_t stream);
// ... and its filtered form (halo_consumer_view_filtered): the sample is bilinear (`bilinear`; else the copy above) at the continuous position
// halo_view.h view_source_pos gives, a dual source's overlap write is cross-faded in with the reference's tent weight (`blend`), and `tap_out`
// (may be null) takes the five floats {fx0, fy0, fx1, fy1, t} per view pixel the values were made from.  A kernel of its own: launch_view's stays.
hipError_t launch_view_filtered(const float* sum, const float* comp, const ProjDev& view, const ProjDev& source, float scale, const float ray_color[3],
                                const float background[3], bool bilinear, bool blend, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, float* tap_out,
                                int blocks, hipStream_t stream);
// halo_view_composite.hip — the same view of the raypath-colour images.  launch_view_composite: `srgb_src` is halo_composite_kernel's srgb_out
// of the source render (3 bytes per source pixel; null: no composite, only map_out / tap_out are written); a tap is its byte triple as floats in
// byte units, value_out (3 floats) the sampled and blended value, srgb_out (3 bytes) uint8(floorf(value + 0.5f)); zeros where map is -1.
// launch_view_lanes: `lanes` are the fp64 class lanes of the source render, class c at lanes[c * source pixels]; a tap is float(lane);
// lanes_out[c * view pixels + p] (null: the geometry alone).  map_out / tap_out are launch_view_filtered's, bit for bit; any output may be null.
hipError_t launch_view_composite(const uint8_t* srgb_src, const ProjDev& view, const ProjDev& source, bool bilinear, bool blend, uint8_t* srgb_out, float* value_out,
                                 int32_t* map_out, float* tap_out, int blocks, hipStream_t stream);
hipError_t launch_view_lanes(const double* lanes, uint32_t class_count, const ProjDev& view, const ProjDev& source, bool bilinear, bool blend, float* lanes_out,
                             int32_t* map_out, float* tap_out, int blocks, hipStream_t stream);
// halo_view_overlay.hip — the auxiliary lines over a gathered view (halo_overlay.h): `dir` and `rgb` are the gather's device buffers of a
// view_w x view_h view, rgb is rewritten in place (null: the sky coordinates alone); value_out (3 floats) and sky_out (6 floats per pixel) may be
// null.  marks: {x, y, present} of zenith, nadir and sun in view pixels.  launch_view_dir writes launch_view's dir_out alone.
hipError_t launch_view_overlay(const float* dir, const HaloViewOverlay& overlay, const float marks[9], int view_w, int view_h, uint8_t* rgb, float* value_out, float* sky_out,
                               int blocks, hipStream_t stream);
hipError_t launch_view_dir(const ProjDev& view, float* dir_out, int blocks, hipStream_t stream);
hipError_t launch_cont_reorder(const float* in, uint32_t in_stride, uint32_t region, const uint32_t* cnt, uint32_t max_fill, const uint32_t* mask, uint32_t n_roots,
                               uint32_t* tile_sum, uint32_t* base, float* out, uint32_t out_stride, uint32_t n_cont, uint32_t planes, uint32_t* err, hipStream_t stream);

}  // namespace halo

#endif
