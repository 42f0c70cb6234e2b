// hip_trace_backend.hpp — C++ adapter: the C ABI of include/halo_trace.h presented with the method set, state
// machine and error behaviour of `lumice::TraceBackend` (reference src/core/backend/trace_backend.hpp:367-641).
//
// Header-only, depends on nothing but <stdexcept>/<vector> and halo_trace.h, so it compiles in this repo (see
// tests/test_cpp_adapter.py) AND inside a Lumice checkout.  There, INTEGRATION.md shows the 30-line glue that
// derives from the real `lumice::TraceBackend`, converts SceneConfig/RenderConfig → HaloScene/HaloRender and
// forwards to this class; nothing here includes reference headers.
#ifndef HALO_HIP_TRACE_BACKEND_HPP_
#define HALO_HIP_TRACE_BACKEND_HPP_

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/halo_trace.h"

namespace halo {

// Mirrors lumice::BackendUnavailableError (trace_backend.hpp:140-158): the ONE recoverable error; the caller drops
// the backend for the rest of Run() and re-runs the wavelength on the legacy CPU path (simulator.cpp:1049-1062).
class BackendUnavailableError : public std::runtime_error {
 public:
  using std::runtime_error::runtime_error;
};

struct XyzImageData {  // trace_backend.hpp:356-360
  float* data = nullptr;
  int width = 0;
  int height = 0;
};

struct LayerHandle {  // trace_backend.hpp:309-333 (value type here: the device state lives in the backend)
  HaloLayerStats stats{};
  size_t ContinuationCount() const { return static_cast<size_t>(stats.continuation_count); }
};

class HipTraceBackend {
 public:
  // CreateBackend(BackendKind::kHip): simulator.cpp:854-919.  seed = effective_seed_ (non-zero).
  explicit HipTraceBackend(int device_ordinal = 0, uint32_t seed = 1) {
    int rc = halo_create(device_ordinal, seed, &h_);
    if (rc == HALO_UNAVAILABLE) throw BackendUnavailableError("halo: no usable gfx950 device");
    if (rc != HALO_OK) throw std::runtime_error("halo_create failed");
  }
  ~HipTraceBackend() { halo_destroy(h_); }
  HipTraceBackend(const HipTraceBackend&) = delete;
  HipTraceBackend& operator=(const HipTraceBackend&) = delete;

  void SetOption(const char* key, int64_t value) { Check(halo_set_option(h_, key, value)); }
  // option "deterministic" (halo_trace.h): fixed-point accumulation — a fixed seed and ray_base give the same image bytes on every run; a
  // multi-layer scene needs SetOption("cont_order", 1) beside it, and BeginSession throws for what the route does not cover.  Not inside a session.
  void SetDeterministic(bool on) { SetOption("deterministic", on ? 1 : 0); }

  // --- the seam ---------------------------------------------------------------------------------------------
  void BeginSession(const HaloScene& scene, const HaloRender& render, const HaloWl& wl, size_t ray_num = 0) {
    Check(halo_begin(h_, &scene, &render, &wl, ray_num));
    width_ = render.width;
    height_ = render.height;
  }
  // Beyond the reference's seam (its caller opens one session per wavelength, simulator.cpp:1098-1109): ONE session for a whole discrete spectrum,
  // halo_begin_spectrum — 1..HALO_WL_POOL_MAX discrete entries, dealt out to the roots of each crystal entry's share in blocks of consecutive
  // roots (halo_trace.h).  Everything after BeginSession is the same; one entry is that wavelength's discrete session.
  void BeginSpectrumSession(const HaloScene& scene, const HaloRender& render, const std::vector<HaloWl>& wls, size_t ray_num = 0) {
    Check(halo_begin_spectrum(h_, &scene, &render, wls.empty() ? nullptr : wls.data(), static_cast<int32_t>(wls.size()), ray_num));
    width_ = render.width;
    height_ = render.height;
  }
  // First call: host mode (count roots generated on device, or injected golden rays); later calls consume the
  // continuation returned by Recombine (trace_backend.hpp:380-389).
  LayerHandle TraceLayer(size_t count, const HaloHostRays* host = nullptr) {
    LayerHandle lh;
    Check(halo_trace_layer(h_, count, host, &lh.stats));
    return lh;
  }
  size_t Recombine(const LayerHandle&, bool shuffle = true) {
    uint64_t n = 0;
    Check(halo_recombine(h_, shuffle ? 1 : 0, &n));
    return static_cast<size_t>(n);
  }
  // TraceBackend::DrainExits (trace_backend.hpp:430-448): every record emitted since the previous drain, no clamp.  A
  // device-accumulating backend has none in production; with the "capture_exits" option (tests) the captured records come
  // back.  max_records > 0 drains in pieces: at most that many now, the rest stays pending for the next call.
  size_t DrainExits(std::vector<HaloExitRecord>& out, size_t max_records = 0) {
    uint64_t n = 0;
    Check(halo_drain_exits(h_, nullptr, 0, &n));  // pending count, nothing consumed
    if (max_records && n > max_records) n = max_records;
    out.resize(static_cast<size_t>(n));
    if (n) Check(halo_drain_exits(h_, out.data(), n, &n));
    out.resize(static_cast<size_t>(n));
    return out.size();
  }
  bool SupportsDeviceXyzAccum() const { return true; }
  bool SupportsThirdClockDrain() const { return true; }  // accumulator persists across sessions (cu:4801-4808)
  uint32_t WlPoolSize() const { return 64; }             // illuminant mode: per-ray pool (wl_pool.hpp:41)
  // Adds into landed_weight, copies W*H*3 floats, zeroes the device accumulator (trace_backend.hpp:461-469).
  void ReadbackXyzAccum(XyzImageData& xyz, float& landed_weight) {
    Check(halo_readback_xyz(h_, xyz.data, xyz.width, xyz.height, &landed_weight));
  }
  void EndSession() { Check(halo_end(h_)); }

  // --- beyond the reference's virtuals: tables the reference hands over inside SessionSpec, and the deferred tallies ---
  // physical filters referenced by HaloEntry::filter_id (reference: FilterSpec per scattering setting, filter_spec.hpp)
  void SetFilters(const std::vector<HaloFilter>& filters) {
    Check(halo_set_filters(h_, filters.empty() ? nullptr : filters.data(), static_cast<int32_t>(filters.size())));
  }
  // raypath colour (reference: SessionSpec::raypath_color → ColorGateTable / ColorClassTable)
  void SetColor(const std::vector<HaloColorSet>& sets, const std::vector<HaloColorClass>& classes) {
    Check(halo_set_color(h_, sets.empty() ? nullptr : sets.data(), static_cast<int>(sets.size()), classes.empty() ? nullptr : classes.data(),
                         static_cast<int>(classes.size())));
    class_count_ = classes.size();
  }
  // TraceBackend::ReadbackClassLanes (trace_backend.hpp:471-493): lane c at lane_data[c*W*H + py*W + px]; zeroes the device
  void ReadbackClassLanes(std::vector<float>& lane_data, size_t& class_count) {
    class_count = class_count_;
    lane_data.assign(class_count_ * static_cast<size_t>(width_) * static_cast<size_t>(height_), 0.0f);
    if (class_count_) Check(halo_readback_class_lanes(h_, lane_data.data(), width_, height_, static_cast<int>(class_count_)));
  }
  // Shards (halo_trace.h halo_set_shard): this backend is shard `index` of `count` of every session from here on — BeginSession / TraceLayer take the
  // WHOLE session's ray count, the backend plans it as one rank would and launches its slice.  With SetDeterministic(true) the shard's integer planes
  // leave through ExportFixed; the integer sum of all shards' words, imported into one backend (ImportFixed) that then reads back, is the one-rank
  // image bit for bit.  Throws for what sharding refuses (a multi-layer scene, host rays, option "rank").
  void SetShard(uint32_t index, uint32_t count) { Check(halo_set_shard(h_, index, count)); }
  struct FixedLayout {
    uint32_t plane_cnt = 0, frac_bits = 0, landed_frac_bits = 0;
  };
  // words the export of a session with `planes` planes writes: planes * W * H, then the landed integer
  uint64_t FixedWords(uint32_t planes) const { return static_cast<uint64_t>(planes) * static_cast<uint64_t>(width_) * static_cast<uint64_t>(height_) + 1u; }
  // MOVES the pending fixed-point planes and the untaken landed integer into n_words 64-bit words of DEVICE memory (pixel order, plane by plane)
  FixedLayout ExportFixed(void* dev_words, uint64_t n_words) {
    FixedLayout l;
    Check(halo_export_fixed(h_, dev_words, n_words, &l.plane_cnt, &l.frac_bits, &l.landed_frac_bits));
    return l;
  }
  // ADDS such words (device memory) into the planes of this backend's last deterministic session; `rays` = the rays they stand for
  void ImportFixed(const void* dev_words, uint64_t n_words, const FixedLayout& l, uint64_t rays) {
    Check(halo_import_fixed(h_, dev_words, n_words, l.plane_cnt, l.frac_bits, l.landed_frac_bits, rays));
  }
  // multi-GPU drain from a C++ host: one ncclReduce of the accumulator onto `root`, the other ranks drained (halo_reduce_accumulator)
  void ReduceAccumulator(void* nccl_comm, int root, int this_rank) { Check(halo_reduce_accumulator(h_, nccl_comm, root, this_rank)); }
  double TakeLanded() {
    double l = 0.0;
    Check(halo_take_landed(h_, &l));
    return l;
  }
  // option "async" = 1: final-layer TraceLayer only queues; the summed LayerStats of everything traced since the last call
  HaloLayerStats CollectStats() {
    HaloLayerStats st{};
    Check(halo_collect_stats(h_, &st));
    return st;
  }
  // RenderConsumer on the device (server/render.cpp:138-330)
  void ConsumeDeviceFused() { Check(halo_consumer_fold(h_)); }
  // ... and the same for a drained image the caller holds (SimData::xyz_pixel_data_ / xyz_landed_weight_ / lane_pixel_data_ of another rank or backend)
  void ConsumeDeviceFused(const float* xyz, int width, int height, float landed, const float* lanes = nullptr, int class_count = 0) {
    Check(halo_consumer_consume(h_, xyz, width, height, landed, lanes, class_count));
  }
  // CompositeColorClassesLinear + LinearRgbToSrgbU8 (server/component_compositor.cpp:180-303) on the device lanes, which stay; returns what the
  // reference's function returns (false: nothing referenced, or no energy in the participating lanes); either output may be null
  bool CompositeColorClasses(const HaloComposite& spec, float* linear_rgb_out, uint8_t* srgb_out, float* participating_p99_y = nullptr) {
    int32_t produced = 0;
    Check(halo_consumer_composite(h_, &spec, linear_rgb_out, srgb_out, participating_p99_y, &produced));
    return produced != 0;
  }
  // lanes summed elsewhere (other ranks, a saved consumer) become this consumer's lanes; total_intensity < 0 keeps the consumer's own
  void LoadClassLanes(const float* lanes, int width, int height, int class_count, double total_intensity = -1.0) {
    Check(halo_consumer_load_lanes(h_, lanes, width, height, class_count, total_intensity));
  }
  double Snapshot(const HaloDisplay& display, uint8_t* rgb_out, float* xyz_out = nullptr) {
    double total = 0.0;
    Check(halo_consumer_snapshot(h_, &display, rgb_out, xyz_out, &total));
    return total;
  }
  // The consumer's image through another lens (halo_consumer_view): per pixel of spec.view the direction of its centre, the pixel of the source
  // render that direction lands on, its raw XYZ and its display transform — what the reference's preview / export shaders gather from their
  // full-sky image, here from the image where it lies.  Every output may be null.
  void View(const HaloViewSpec& spec, uint8_t* rgb_out, float* xyz_out = nullptr, int32_t* map_out = nullptr, float* dir_out = nullptr) {
    Check(halo_consumer_view(h_, &spec, rgb_out, xyz_out, map_out, dir_out));
  }
  // ... with a filter (halo_consumer_view_filtered): bilinear taps around the continuous source position, a dual source's overlap band cross-faded
  // as the reference's sampleDualFisheye does; tap_out takes {fx0, fy0, fx1, fy1, t} per pixel.  {HALO_VIEW_NEAREST, 0} is the call above.
  void View(const HaloViewSpec& spec, const HaloViewFilter& filter, uint8_t* rgb_out, float* xyz_out = nullptr, int32_t* map_out = nullptr, float* dir_out = nullptr,
            float* tap_out = nullptr) {
    Check(halo_consumer_view_filtered(h_, &spec, &filter, rgb_out, xyz_out, map_out, dir_out, tap_out));
  }
  // The class composite through the view (halo_consumer_view_composite: the reference's preview in RGB mode): srgb_out 3 bytes, value_out 3 floats
  // in byte units, map_out / tap_out the filtered view's; returns CompositeColorClasses' answer.  spec.display is ignored; the source render has
  // the lanes' size.  {HALO_VIEW_NEAREST, 0} shows halo_consumer_composite's own bytes.
  bool ViewComposite(const HaloViewSpec& spec, const HaloViewFilter& filter, const HaloComposite& composite, uint8_t* srgb_out, float* value_out = nullptr,
                     int32_t* map_out = nullptr, float* tap_out = nullptr, float* participating_p99_y = nullptr) {
    int32_t produced = 0;
    Check(halo_consumer_view_composite(h_, &spec, &filter, &composite, srgb_out, value_out, map_out, tap_out, participating_p99_y, &produced));
    return produced != 0;
  }
  // ... and the class lanes themselves (halo_consumer_view_lanes): lanes_out float[class_count][view height][view width], raw
  void ViewLanes(const HaloViewSpec& spec, const HaloViewFilter& filter, float* lanes_out, int32_t* map_out = nullptr, float* tap_out = nullptr) {
    Check(halo_consumer_view_lanes(h_, &spec, &filter, lanes_out, map_out, tap_out));
  }
  // The filtered view with the auxiliary lines on it (halo_consumer_view_overlay: horizon, grid, sun circles, zenith / nadir rings, sun marker —
  // halo_host_view_overlay_defaults fills the reference's record): rgb_out 3 bytes, value_out 3 floats in byte units, sky_out 6 floats per pixel,
  // marks_out 9 floats, map_out / dir_out the view's
  void ViewOverlay(const HaloViewSpec& spec, const HaloViewFilter& filter, const HaloViewOverlay& overlay, uint8_t* rgb_out, float* value_out = nullptr,
                   float* sky_out = nullptr, float* marks_out = nullptr, int32_t* map_out = nullptr, float* dir_out = nullptr) {
    Check(halo_consumer_view_overlay(h_, &spec, &filter, &overlay, rgb_out, value_out, sky_out, marks_out, map_out, dir_out));
  }
  // ... and the class composite's view with them (halo_consumer_view_composite_overlay); returns CompositeColorClasses' answer: false, nothing drawn
  bool ViewCompositeOverlay(const HaloViewSpec& spec, const HaloViewFilter& filter, const HaloComposite& composite, const HaloViewOverlay& overlay, uint8_t* srgb_out,
                            float* value_out = nullptr, float* sky_out = nullptr, float* marks_out = nullptr, int32_t* map_out = nullptr, float* tap_out = nullptr,
                            float* dir_out = nullptr, float* participating_p99_y = nullptr) {
    int32_t produced = 0;
    Check(halo_consumer_view_composite_overlay(h_, &spec, &filter, &composite, &overlay, srgb_out, value_out, sky_out, marks_out, map_out, tap_out, dir_out,
                                               participating_p99_y, &produced));
    return produced != 0;
  }
  // The reference GUI's Adaptive Brightness anchor (gui/gui_ev_auto.hpp ComputeP99Y + ComputeEvAuto) on the device consumer: expose a
  // snapshot with display.intensity_factor * exp2(result.ev_auto); result.produced == 0 is the GUI's "auto: no data"
  HaloAutoEv AutoEv(int downsample = 8, float target_white = 135.f) {
    HaloAutoEv r{};
    Check(halo_consumer_auto_ev(h_, downsample, target_white, &r));
    return r;
  }
  // Exact percentiles and moments of the positive values of the consumer's Y (or of one class lane), computed where the image lies: the numbers of
  // the reference's doc/xyz-stats-tool.md.  An EV at another anchor than AutoEv's P99 of the box sums is one more call, e.g. for P99.5:
  // halo_host_ev_auto(float(stats.value[j]), AutoEv().per_pixel_intensity, target_white).  The seam has no counterpart: it is this backend's own.
  HaloImageStats ImageStats(const HaloStatsSpec& spec) {
    HaloImageStats r{};
    Check(halo_consumer_stats(h_, &spec, &r));
    return r;
  }
  // trace_backend.hpp:587,625 — real counts of the last session's stochastic draws (never stand-ins)
  size_t GetLastBatchStochasticCrystalSampleCount() const {
    uint64_t c = 0, o = 0;
    (void)halo_last_sample_counts(h_, &c, &o);
    return static_cast<size_t>(c);
  }
  size_t GetLastBatchStochasticOrientationSampleCount() const {
    uint64_t c = 0, o = 0;
    (void)halo_last_sample_counts(h_, &c, &o);
    return static_cast<size_t>(o);
  }
  bool IsCompatible(const HaloRender& render) const { return render.width > 0 && render.height > 0; }

 private:
  void Check(int rc) {
    if (rc == HALO_OK) return;
    std::string msg = halo_last_error(h_);
    if (rc == HALO_UNAVAILABLE) throw BackendUnavailableError(msg);
    throw std::runtime_error(msg);
  }
  halo_handle_t h_ = nullptr;
  int width_ = 0, height_ = 0;
  size_t class_count_ = 0;
};

}  // namespace halo

#endif
