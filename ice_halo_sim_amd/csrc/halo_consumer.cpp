// halo_consumer.cpp — the consumer stages of the C ABI (RenderConsumer, server/render.hpp, on the device): the Neumaier running image and its
// total landed intensity (reset, fold, consume), and what is made of them — snapshot, auto exposure, image statistics, the view through another
// lens, with or without the auxiliary lines — and of the class lanes: load, composite, composite and lanes through another lens, read-back.  Their state is HaloBackend::cons (halo_state.h Consumer); the lanes themselves are
// written by trace sessions and stay with the session state.  Host C++ only; built without FMA contraction like every host unit: the float
// expressions below are the reference's, operand for operand.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "halo_state.h"

using namespace halo;

namespace {

// ExposureScale (render.cpp:96-102) over the consumer's `npix` pixels, evaluated in float like the reference.
float exposure_scale(const HaloBackend* b, float intensity_factor, uint32_t npix) {
  const float snapshot_intensity = static_cast<float>(b->cons.total_intensity);
  return (npix == 0 || snapshot_intensity <= 0.0f) ? 0.0f : intensity_factor * 0.08f * static_cast<float>(npix) / snapshot_intensity;
}
// The per-pixel intensity of GetRawXyzResult (render.cpp:586-587) for an image of `total_pix` pixels, in float like the reference.
float per_pixel_intensity(const HaloBackend* b, int total_pix) {
  const float snapshot_intensity = static_cast<float>(b->cons.total_intensity);
  return total_pix > 0 ? snapshot_intensity / (0.08f * total_pix) : 0.0f;
}
// The running image for w x h pixels: reserved, zeroed, nothing landed yet.
int start_image(HaloBackend* b, int w, int h) {
  const size_t n = static_cast<size_t>(w) * h * 3;
  HIPCHK(b, b->cons.sum.reserve(n));
  HIPCHK(b, b->cons.comp.reserve(n));
  b->cons.w = w;
  b->cons.h = h;
  HIPCHK(b, hipMemsetAsync(b->cons.sum.ptr, 0, n * sizeof(float), main_q(b)));
  HIPCHK(b, hipMemsetAsync(b->cons.comp.ptr, 0, n * sizeof(float), main_q(b)));
  b->cons.total_intensity = 0.0;
  return HALO_OK;
}

// The view calls in two steps, so that a pass can run between them on the gather's device buffers (halo_consumer_view_overlay).
// view_launch: halo_consumer_view's and halo_consumer_view_filtered's (`filter` != nullptr: its kernel and its fifth output) argument checks and
// launch; `want` says which of the five device buffers the kernel fills, `any_output` whether the caller takes anything at all.  `who` names the
// call in the messages.
struct ViewWant {
  bool rgb, xyz, map, dir, tap;
};
struct ViewPlan {
  size_t npix = 0, n = 0;   // view pixels, and three per pixel
  float scale = 0.0f;       // the exposure scale (0: PostSnapshot's early-out, the bytes are zeros whatever the kernel wrote)
};
int view_launch(HaloBackend* b, const char* who, const HaloViewSpec* spec, const HaloViewFilter* filter, const ViewWant& want, bool any_output, ViewPlan* plan) {
  if (!b) return HALO_FATAL;
  const std::string name(who);
  if (!spec) return fail(b, HALO_FATAL, name + ": spec is NULL");
  if (!b->cons.sum.ptr) return fail(b, HALO_FATAL, name + " before consumer_fold");
  if (b->in_session) return fail(b, HALO_FATAL, name + " inside a session");
  if (!any_output) return fail(b, HALO_FATAL, name + ": every output is NULL");
  const HaloRender& view = spec->view;
  if (view.width <= 0 || view.height <= 0) return fail(b, HALO_FATAL, name + ": empty view");
  if (static_cast<uint64_t>(view.width) * static_cast<uint64_t>(view.height) > (1ull << 25))
    return fail(b, HALO_UNAVAILABLE, name + ": a view of more than 2^25 pixels");
  if (!spec->has_source && !b->had_session) return fail(b, HALO_FATAL, name + ": no source render (has_source = 0 on a handle that has had no session)");
  const HaloRender& source = spec->has_source ? spec->source : b->render;
  if (source.width != b->cons.w || source.height != b->cons.h) return fail(b, HALO_FATAL, name + ": the source render's size is not the consumer's");
  if (view.lens_type < HALO_LENS_LINEAR || view.lens_type > HALO_LENS_GLOBE || source.lens_type < HALO_LENS_LINEAR || source.lens_type > HALO_LENS_GLOBE)
    return fail(b, HALO_FATAL, name + ": unknown lens type");
  HIPCHK(b, hipSetDevice(b->device));
  const uint32_t cons_pix = static_cast<uint32_t>(b->cons.w) * static_cast<uint32_t>(b->cons.h);
  const size_t npix = static_cast<size_t>(view.width) * static_cast<size_t>(view.height), n = npix * 3;
  const float scale = exposure_scale(b, spec->display.intensity_factor, cons_pix);   // over the CONSUMER's pixels, as halo_consumer_snapshot: a view pixel is its source pixel's byte
  plan->npix = npix;
  plan->n = n;
  plan->scale = scale;
  if (want.rgb) HIPCHK(b, b->cons.view_rgb.reserve(n));
  if (want.xyz) HIPCHK(b, b->cons.view_xyz.reserve(n));
  if (want.dir) HIPCHK(b, b->cons.view_dir.reserve(n));
  if (want.map) HIPCHK(b, b->cons.view_map.reserve(npix));
  if (want.tap) HIPCHK(b, b->cons.view_tap.reserve(npix * 5));
  uint8_t* rgb_dev = want.rgb ? b->cons.view_rgb.ptr : nullptr;
  float* xyz_dev = want.xyz ? b->cons.view_xyz.ptr : nullptr;
  int32_t* map_dev = want.map ? b->cons.view_map.ptr : nullptr;
  float* dir_dev = want.dir ? b->cons.view_dir.ptr : nullptr;
  hipError_t e;
  if (filter)
    e = launch_view_filtered(b->cons.sum.ptr, b->cons.comp.ptr, host::BuildProj(view), host::BuildProj(source), scale, spec->display.ray_color, spec->display.background,
                             filter->filter == HALO_VIEW_BILINEAR, filter->blend != 0, rgb_dev, xyz_dev, map_dev, dir_dev, want.tap ? b->cons.view_tap.ptr : nullptr,
                             b->cu_count * 8, main_q(b));
  else
    e = launch_view(b->cons.sum.ptr, b->cons.comp.ptr, host::BuildProj(view), host::BuildProj(source), scale, spec->display.ray_color, spec->display.background, rgb_dev,
                    xyz_dev, map_dev, dir_dev, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, filter ? "halo_view_filtered_kernel launch" : "halo_view_kernel launch");
  return HALO_OK;
}
// view_copy_back: the device buffers of a launched view into the caller's (any may be null), one synchronise, and the early-out's zero bytes.
int view_copy_back(HaloBackend* b, const ViewPlan& plan, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, float* tap_out) {
  const size_t npix = plan.npix, n = plan.n;
  if (rgb_out) HIPCHK(b, hipMemcpyAsync(rgb_out, b->cons.view_rgb.ptr, n, hipMemcpyDeviceToHost, main_q(b)));
  if (xyz_out) HIPCHK(b, hipMemcpyAsync(xyz_out, b->cons.view_xyz.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  if (map_out) HIPCHK(b, hipMemcpyAsync(map_out, b->cons.view_map.ptr, npix * sizeof(int32_t), hipMemcpyDeviceToHost, main_q(b)));
  if (dir_out) HIPCHK(b, hipMemcpyAsync(dir_out, b->cons.view_dir.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  if (tap_out) HIPCHK(b, hipMemcpyAsync(tap_out, b->cons.view_tap.ptr, npix * 5 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  if (rgb_out && plan.scale == 0.0f) std::memset(rgb_out, 0, n);   // PostSnapshot's early-out, as halo_consumer_snapshot has it
  return HALO_OK;
}
int view_call(HaloBackend* b, const char* who, const HaloViewSpec* spec, const HaloViewFilter* filter, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out,
              float* tap_out) {
  ViewPlan plan;
  const ViewWant want{rgb_out != nullptr, xyz_out != nullptr, map_out != nullptr, dir_out != nullptr, tap_out != nullptr};
  if (int rc = view_launch(b, who, spec, filter, want, rgb_out || xyz_out || map_out || dir_out || tap_out, &plan)) return rc;
  return view_copy_back(b, plan, rgb_out, xyz_out, map_out, dir_out, tap_out);
}

// What halo_consumer_view_filtered refuses in a filter, for every call that takes one (nullptr: nothing).
const char* filter_refusal(const HaloViewFilter* filter) {
  if (filter->filter != HALO_VIEW_NEAREST && filter->filter != HALO_VIEW_BILINEAR) return ": unknown filter";
  if (filter->blend != 0 && filter->blend != 1) return ": blend must be 0 or 1";
  if (filter->reserved[0] != 0 || filter->reserved[1] != 0) return ": reserved words must be zero";
  return nullptr;
}

// The overlay pass behind a gather (halo_view_overlay.hip), for both overlay calls: the marks, the launch over the gather's view_dir and — null: the
// sky coordinates alone — its view_rgb, and the copies of what the pass alone makes (not synchronised: the caller's last copy-back waits).
int overlay_pass(HaloBackend* b, const HaloRender& view, const HaloViewOverlay& overlay, bool draw, float* value_out, float* sky_out, float* marks_out) {
  const size_t npix = static_cast<size_t>(view.width) * static_cast<size_t>(view.height);
  float marks[9];
  host::ViewOverlayMarks(view, overlay.sun_dir, marks);
  if (marks_out) std::memcpy(marks_out, marks, sizeof(marks));
  if (!draw && !sky_out) return HALO_OK;
  if (draw && value_out) HIPCHK(b, b->cons.view_val.reserve(npix * 3));
  if (sky_out) HIPCHK(b, b->cons.view_sky.reserve(npix * 6));
  hipError_t e = launch_view_overlay(b->cons.view_dir.ptr, overlay, marks, view.width, view.height, draw ? b->cons.view_rgb.ptr : nullptr,
                                     draw && value_out ? b->cons.view_val.ptr : nullptr, sky_out ? b->cons.view_sky.ptr : nullptr, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_view_overlay_kernel launch");
  if (draw && value_out) HIPCHK(b, hipMemcpyAsync(value_out, b->cons.view_val.ptr, npix * 3 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  if (sky_out) HIPCHK(b, hipMemcpyAsync(sky_out, b->cons.view_sky.ptr, npix * 6 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  return HALO_OK;
}

// What comes before halo_composite_kernel, for halo_consumer_composite and halo_consumer_view_composite alike: the argument checks (`who` names the
// call in the messages), GatherActiveClasses, the participating P99 by three histogram passes — the host waits for each — and
// ParticipatingExposureScale.  `state` says how far the reference's function gets:
enum {
  kCompositeNothing = 0,   // no class references a raypath bit: the reference returns false and touches nothing
  kCompositeBlack = 1,     // no active class: an all-black composite, still a valid one (P99 0)
  kCompositeNoScale = 2,   // the exposure scale is not positive: P99 published, no composite
  kCompositeReady = 3,     // cd is what halo_composite_kernel takes
};
struct CompositePlan {
  CompositeDev cd{};
  float p99 = 0.0f;
  uint32_t npix = 0;   // of the lanes
  int state = kCompositeNothing;
};
int composite_prepare(HaloBackend* b, const char* who, const HaloComposite* spec, CompositePlan* plan) {
  const std::string name(who);
  if (spec->mode < HALO_COMPOSITE_DOMINANT || spec->mode > HALO_COMPOSITE_PAINTER) return fail(b, HALO_FATAL, name + ": unknown mode");
  uint64_t referenced = 0;   // ColorClassTable::referenced_mask_ = OR of the classes' member bits (color_class_table.hpp:38-43)
  for (const HaloColorClass& c : b->color_classes) referenced |= c.bits;
  if (referenced == 0) return HALO_OK;   // component_compositor.cpp:183-185
  if (spec->class_count != static_cast<int>(b->color_classes.size())) return fail(b, HALO_FATAL, name + ": class_count differs from halo_set_color's");
  if (!b->lanes.ptr || b->lanes_w <= 0 || b->lanes_h <= 0) return fail(b, HALO_FATAL, name + " before any colour session (no lanes)");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  const uint32_t npix = static_cast<uint32_t>(b->lanes_w) * static_cast<uint32_t>(b->lanes_h);
  plan->npix = npix;
  // GatherActiveClasses (component_compositor.cpp:24-54): solo beats visible; stable sort by z_order; lane binding by class index
  bool any_solo = false;
  for (int c = 0; c < spec->class_count; c++) any_solo = any_solo || spec->classes[c].solo != 0;
  std::vector<int> order(static_cast<size_t>(spec->class_count));
  for (int c = 0; c < spec->class_count; c++) order[static_cast<size_t>(c)] = c;
  std::stable_sort(order.begin(), order.end(), [spec](int x, int y) { return spec->classes[x].z_order < spec->classes[y].z_order; });
  CompositeDev& cd = plan->cd;
  cd.mode = static_cast<uint32_t>(spec->mode);
  for (int c : order) {
    const HaloCompositeClass& k = spec->classes[c];
    if (!(any_solo ? k.solo != 0 : k.visible != 0)) continue;
    cd.lane[cd.n_active] = static_cast<uint32_t>(c);
    for (int j = 0; j < 3; j++) cd.color[cd.n_active][j] = k.color[j];
    cd.n_active++;
  }
  if (cd.n_active == 0) {
    plan->state = kCompositeBlack;
    return HALO_OK;
  }
  // ComputeParticipatingP99Y (:138-163) as a radix select: 11 + 11 + 10 bits of the float pattern, one histogram pass each
  HIPCHK(b, b->cons.comp_hist.reserve(2048));
  std::vector<uint32_t> hist(2048);
  const int blocks = b->cu_count * 8;
  float p99 = 0.0f;
  {
    uint32_t prefix = 0u;
    uint64_t rank = 0;   // 0-based rank wanted among the values that share `prefix`
    const uint32_t shifts[3] = {21u, 10u, 0u}, widths[3] = {11u, 11u, 10u};
    bool empty = false;
    for (int pass = 0; pass < 3 && !empty; pass++) {
      const uint32_t nb = 1u << widths[pass];
      HIPCHK(b, hipMemsetAsync(b->cons.comp_hist.ptr, 0, nb * sizeof(uint32_t), main_q(b)));
      hipError_t e = launch_lane_hist(b->lanes.ptr, npix, cd, shifts[pass], widths[pass], prefix, b->cons.comp_hist.ptr, blocks, main_q(b));
      if (e != hipSuccess) return hip_fail(b, e, "halo_lane_hist_kernel launch");
      HIPCHK(b, hipMemcpyAsync(hist.data(), b->cons.comp_hist.ptr, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, main_q(b)));
      HIPCHK(b, hipStreamSynchronize(main_q(b)));
      if (pass == 0) {
        uint64_t count = 0;
        for (uint32_t i = 0; i < nb; i++) count += hist[i];
        if (count == 0) {
          empty = true;
          break;
        }
        // idx = size * 0.99f in float, clamped (:156-159)
        uint64_t idx = static_cast<uint64_t>(static_cast<float>(count) * 0.99f);
        if (idx >= count) idx = count - 1;
        rank = idx;
      }
      uint32_t bin = 0;
      for (; bin < nb; bin++) {
        if (rank < hist[bin]) break;
        rank -= hist[bin];
      }
      if (bin >= nb) return fail(b, HALO_FATAL, name + ": lanes changed under the P99 select");
      prefix = (prefix << widths[pass]) | bin;
    }
    if (!empty) std::memcpy(&p99, &prefix, sizeof(float));
  }
  plan->p99 = p99;
  // ParticipatingExposureScale (render.cpp:120-135), in float like the reference
  const float snapshot_intensity = static_cast<float>(b->cons.total_intensity);
  float A = 0.0f;
  if (p99 > 0.0f && snapshot_intensity > 0.0f) {
    const float target_srgb = 135.0f / 255.0f;
    const float target_linear = target_srgb <= 0.04045f ? target_srgb / 12.92f : std::pow((target_srgb + 0.055f) / 1.055f, 2.4f);
    A = spec->intensity_factor * target_linear / p99;
  }
  if (!(A > 0.0f)) {
    plan->state = kCompositeNoScale;
    return HALO_OK;
  }
  cd.a = A;
  cd.s = A * spec->display_exposure_scale;
  cd.display = spec->display_exposure_scale;
  plan->state = kCompositeReady;
  return HALO_OK;
}

// halo_consumer_view_composite and halo_consumer_view_lanes: what both refuse, in one place.  On HALO_OK `*source` is the render the lanes lie under.
int lane_view_checks(HaloBackend* b, const std::string& name, const HaloViewSpec* spec, const HaloViewFilter* filter, bool any_output, const HaloRender** source) {
  if (!spec) return fail(b, HALO_FATAL, name + ": spec is NULL");
  if (b->in_session) return fail(b, HALO_FATAL, name + " inside a session");
  if (!any_output) return fail(b, HALO_FATAL, name + ": every output is NULL");
  if (filter) {
    if (filter->filter != HALO_VIEW_NEAREST && filter->filter != HALO_VIEW_BILINEAR) return fail(b, HALO_FATAL, name + ": unknown filter");
    if (filter->blend != 0 && filter->blend != 1) return fail(b, HALO_FATAL, name + ": blend must be 0 or 1");
    if (filter->reserved[0] != 0 || filter->reserved[1] != 0) return fail(b, HALO_FATAL, name + ": reserved words must be zero");
  }
  // (the second test: classes set after the lanes were made, for which no lane exists yet)
  if (!b->lanes.ptr || b->lanes_w <= 0 || b->lanes_h <= 0 || b->color_classes.size() * static_cast<size_t>(b->lanes_w) * static_cast<size_t>(b->lanes_h) > b->lanes.cap)
    return fail(b, HALO_FATAL, name + " before any colour session or consumer_load_lanes (no lanes)");
  const HaloRender& view = spec->view;
  if (view.width <= 0 || view.height <= 0) return fail(b, HALO_FATAL, name + ": empty view");
  if (static_cast<uint64_t>(view.width) * static_cast<uint64_t>(view.height) > (1ull << 25))
    return fail(b, HALO_UNAVAILABLE, name + ": a view of more than 2^25 pixels");
  if (!spec->has_source && !b->had_session) return fail(b, HALO_FATAL, name + ": no source render (has_source = 0 on a handle that has had no session)");
  const HaloRender& src = spec->has_source ? spec->source : b->render;
  if (src.width != b->lanes_w || src.height != b->lanes_h) return fail(b, HALO_FATAL, name + ": the source render's size is not the lanes'");
  if (view.lens_type < HALO_LENS_LINEAR || view.lens_type > HALO_LENS_GLOBE || src.lens_type < HALO_LENS_LINEAR || src.lens_type > HALO_LENS_GLOBE)
    return fail(b, HALO_FATAL, name + ": unknown lens type");
  *source = &src;
  return HALO_OK;
}

// halo_consumer_view_composite (`overlay` == nullptr: sky_out, marks_out and dir_out are null too) and halo_consumer_view_composite_overlay: stage 1,
// the gather and — with an overlay — the view's directions and the overlay pass over the gathered bytes; value_out is then the pass's.
int view_composite_call(HaloBackend* b, const std::string& name, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloComposite* composite,
                        const HaloViewOverlay* overlay, uint8_t* srgb_out, float* value_out, float* sky_out, float* marks_out, int32_t* map_out, float* tap_out, float* dir_out,
                        float* participating_p99_y, int32_t* produced) {
  if (!produced) return fail(b, HALO_FATAL, name + ": produced is NULL");
  *produced = 0;
  const HaloRender* source = nullptr;
  if (int rc = lane_view_checks(b, name, spec, filter, srgb_out || value_out || sky_out || marks_out || map_out || tap_out || dir_out, &source)) return rc;
  if (!composite) return fail(b, HALO_FATAL, name + ": composite is NULL");
  if (composite->mode < HALO_COMPOSITE_DOMINANT || composite->mode > HALO_COMPOSITE_PAINTER) return fail(b, HALO_FATAL, name + ": unknown mode");
  if (composite->class_count != static_cast<int>(b->color_classes.size())) return fail(b, HALO_FATAL, name + ": class_count differs from halo_set_color's");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be adding to the lanes on the trace / auxiliary streams)
  CompositePlan plan;
  if (int rc = composite_prepare(b, name.c_str(), composite, &plan)) return rc;
  const HaloRender& view = spec->view;
  const size_t npix = static_cast<size_t>(view.width) * static_cast<size_t>(view.height), n = npix * 3;
  const bool ready = plan.state == kCompositeReady;
  const uint8_t* src_dev = nullptr;
  if (ready && (srgb_out || value_out)) {
    HIPCHK(b, b->cons.view_comp_src.reserve(static_cast<size_t>(plan.npix) * 3u));
    hipError_t e = launch_composite(b->lanes.ptr, plan.npix, plan.cd, nullptr, b->cons.view_comp_src.ptr, b->cu_count * 8, main_q(b));
    if (e != hipSuccess) return hip_fail(b, e, "halo_composite_kernel launch");
    src_dev = b->cons.view_comp_src.ptr;
  }
  // with an overlay the gather always writes its bytes (the pass draws on them) and never its value: value_out is the colour after the last layer
  const bool gather_rgb = src_dev && (srgb_out || (overlay && value_out)), gather_value = src_dev && value_out && !overlay;
  bool pending = false;
  if (src_dev || map_out || tap_out) {
    if (gather_rgb) HIPCHK(b, b->cons.view_rgb.reserve(n));
    if (gather_value) HIPCHK(b, b->cons.view_xyz.reserve(n));
    if (map_out) HIPCHK(b, b->cons.view_map.reserve(npix));
    if (tap_out) HIPCHK(b, b->cons.view_tap.reserve(npix * 5));
    hipError_t e = launch_view_composite(src_dev, host::BuildProj(view), host::BuildProj(*source), filter && filter->filter == HALO_VIEW_BILINEAR, filter && filter->blend != 0,
                                         gather_rgb ? b->cons.view_rgb.ptr : nullptr, gather_value ? b->cons.view_xyz.ptr : nullptr,
                                         map_out ? b->cons.view_map.ptr : nullptr, tap_out ? b->cons.view_tap.ptr : nullptr, b->cu_count * 8, main_q(b));
    if (e != hipSuccess) return hip_fail(b, e, "halo_view_composite_kernel launch");
    pending = true;
  }
  if (overlay) {
    if (gather_rgb || sky_out || dir_out) {
      HIPCHK(b, b->cons.view_dir.reserve(n));
      hipError_t e = launch_view_dir(host::BuildProj(view), b->cons.view_dir.ptr, b->cu_count * 8, main_q(b));
      if (e != hipSuccess) return hip_fail(b, e, "halo_view_dir_kernel launch");
      if (dir_out) HIPCHK(b, hipMemcpyAsync(dir_out, b->cons.view_dir.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
      pending = true;
    }
    if (int rc = overlay_pass(b, view, *overlay, gather_rgb, value_out, sky_out, marks_out)) return rc;
  }
  if (pending) {
    if (gather_rgb && srgb_out) HIPCHK(b, hipMemcpyAsync(srgb_out, b->cons.view_rgb.ptr, n, hipMemcpyDeviceToHost, main_q(b)));
    if (gather_value) HIPCHK(b, hipMemcpyAsync(value_out, b->cons.view_xyz.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
    if (map_out) HIPCHK(b, hipMemcpyAsync(map_out, b->cons.view_map.ptr, npix * sizeof(int32_t), hipMemcpyDeviceToHost, main_q(b)));
    if (tap_out) HIPCHK(b, hipMemcpyAsync(tap_out, b->cons.view_tap.ptr, npix * 5 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
    HIPCHK(b, hipStreamSynchronize(main_q(b)));
  }
  // the cases that stop before a composite, as halo_consumer_composite has them
  if (plan.state == kCompositeNothing) return HALO_OK;   // neither image is written
  if (plan.state == kCompositeBlack) {
    if (srgb_out) std::memset(srgb_out, 0, n);
    if (value_out) std::memset(value_out, 0, n * sizeof(float));
    if (participating_p99_y) *participating_p99_y = 0.0f;
    *produced = 1;
    return HALO_OK;
  }
  if (participating_p99_y) *participating_p99_y = plan.p99;
  if (plan.state == kCompositeNoScale) {   // the bytes stay untouched; the value image is the zeros the reference assigns its linear buffer
    if (value_out) std::memset(value_out, 0, n * sizeof(float));
    return HALO_OK;
  }
  *produced = 1;
  return HALO_OK;
}

}  // namespace

extern "C" {

// ---- consumer on device ------------------------------------------------------------------------------------
int halo_consumer_reset(halo_handle_t b) {
  if (!b) return HALO_FATAL;
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  if (b->cons.sum.ptr) {
    const size_t n = static_cast<size_t>(b->cons.w) * b->cons.h * 3;
    HIPCHK(b, hipMemsetAsync(b->cons.sum.ptr, 0, n * sizeof(float), main_q(b)));
    HIPCHK(b, hipMemsetAsync(b->cons.comp.ptr, 0, n * sizeof(float), main_q(b)));
  }
  if (b->lanes.ptr) HIPCHK(b, hipMemsetAsync(b->lanes.ptr, 0, b->lanes.cap * sizeof(double), main_q(b)));   // RenderConsumer::Reset clears the class lanes too (render.cpp:598-612)
  b->cons.total_intensity = 0.0;
  return HALO_OK;
}

int halo_consumer_fold(halo_handle_t b) {
  if (!b) return HALO_FATAL;
  if (!b->acc || b->acc_w <= 0) return fail(b, HALO_FATAL, "consumer_fold before any session");
  HIPCHK(b, hipSetDevice(b->device));
  int rc = fold_if_dirty(b);
  if (rc != HALO_OK) return rc;
  const size_t n = static_cast<size_t>(b->acc_w) * b->acc_h * 3;
  if (b->cons.w != b->acc_w || b->cons.h != b->acc_h || !b->cons.sum.ptr)
    if (int rc = start_image(b, b->acc_w, b->acc_h)) return rc;
  hipError_t e = launch_consumer_fold(b->acc, b->cons.sum.ptr, b->cons.comp.ptr, static_cast<uint32_t>(n), b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_consumer_fold_kernel launch");
  double landed = 0.0;
  if (int rc = take_landed_delta(b, &landed)) return rc;
  b->cons.total_intensity += landed;  // total_intensity_ += xyz_landed_weight_ (render.cpp:149)
  return HALO_OK;
}

int halo_consumer_consume(halo_handle_t b, const float* xyz, int width, int height, float landed, const float* lanes, int class_count) {
  if (!b || !xyz) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "consumer_consume inside a session");
  if (width <= 0 || height <= 0) return fail(b, HALO_FATAL, "consumer_consume: empty image");
  if (static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > (1ull << 25)) return fail(b, HALO_UNAVAILABLE, "more than 2^25 pixels");
  if (b->cons.sum.ptr && (b->cons.w != width || b->cons.h != height)) return fail(b, HALO_FATAL, "consumer_consume: image size differs from the consumer's (halo_consumer_reset first)");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  const size_t n = static_cast<size_t>(width) * height * 3;
  if (!b->cons.sum.ptr)
    if (int rc = start_image(b, width, height)) return rc;
  // the caller's image goes through the staging buffer and the same Neumaier fold kernel the device accumulator takes (the kernel zeroes
  // what it folds: the staging buffer here)
  HIPCHK(b, b->cons.stage.reserve(n));
  HIPCHK(b, hipMemcpyAsync(b->cons.stage.ptr, xyz, n * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
  hipError_t e = launch_consumer_fold(b->cons.stage.ptr, b->cons.sum.ptr, b->cons.comp.ptr, static_cast<uint32_t>(n), b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_consumer_fold_kernel launch");
  if (lanes != nullptr && class_count > 0) {   // lane_pixel_data_: dst[p] += src[p] per class (render.cpp:176-185)
    if (class_count != static_cast<int>(b->color_classes.size())) return fail(b, HALO_FATAL, "consumer_consume: class count must equal halo_set_color's");
    const size_t nl = static_cast<size_t>(class_count) * width * height;
    if (!b->lanes.ptr || b->lanes_w != width || b->lanes_h != height) {
      HIPCHK(b, b->lanes.reserve(nl));
      HIPCHK(b, hipMemsetAsync(b->lanes.ptr, 0, b->lanes.cap * sizeof(double), main_q(b)));
      b->lanes_w = width;
      b->lanes_h = height;
    }
    HIPCHK(b, b->cons.lanes_stage.reserve(nl));
    HIPCHK(b, hipMemcpyAsync(b->cons.lanes_stage.ptr, lanes, nl * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
    e = launch_lanes_add(b->cons.lanes_stage.ptr, b->lanes.ptr, nl, b->cu_count * 8, main_q(b));
    if (e != hipSuccess) return hip_fail(b, e, "halo_lanes_add_kernel launch");
  }
  HIPCHK(b, hipStreamSynchronize(main_q(b)));   // `xyz` / `lanes` are the caller's (pageable) memory
  b->cons.total_intensity += static_cast<double>(landed);   // total_intensity_ += xyz_landed_weight_ (render.cpp:149)
  return HALO_OK;
}

int halo_consumer_snapshot(halo_handle_t b, const HaloDisplay* dsp, uint8_t* rgb_out, float* xyz_out, double* total_intensity) {
  if (!b || !dsp) return HALO_FATAL;
  if (!b->cons.sum.ptr) return fail(b, HALO_FATAL, "consumer_snapshot before consumer_fold");
  HIPCHK(b, hipSetDevice(b->device));
  const uint32_t npix = static_cast<uint32_t>(b->cons.w) * static_cast<uint32_t>(b->cons.h);
  const size_t n = static_cast<size_t>(npix) * 3;
  const float scale = exposure_scale(b, dsp->intensity_factor, npix);
  if (rgb_out) HIPCHK(b, b->cons.rgb.reserve(n));
  if (xyz_out) HIPCHK(b, b->cons.xyz_out.reserve(n));
  hipError_t e = launch_post_snapshot(b->cons.sum.ptr, b->cons.comp.ptr, rgb_out ? b->cons.rgb.ptr : nullptr,
                                      xyz_out ? b->cons.xyz_out.ptr : nullptr, npix, scale, dsp->ray_color, dsp->background,
                                      b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_post_snapshot_kernel launch");
  if (rgb_out) HIPCHK(b, hipMemcpyAsync(rgb_out, b->cons.rgb.ptr, n, hipMemcpyDeviceToHost, main_q(b)));
  if (xyz_out) HIPCHK(b, hipMemcpyAsync(xyz_out, b->cons.xyz_out.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  if (rgb_out && scale == 0.0f) std::memset(rgb_out, 0, n);  // PostSnapshot early-out (render.cpp:515-518)
  if (total_intensity) *total_intensity = b->cons.total_intensity;
  return HALO_OK;
}

int halo_consumer_auto_ev(halo_handle_t b, int32_t downsample_factor, float target_white, HaloAutoEv* out) {
  if (!b) return HALO_FATAL;
  if (!out) return fail(b, HALO_FATAL, "consumer_auto_ev: out is NULL");
  if (!b->cons.sum.ptr) return fail(b, HALO_FATAL, "consumer_auto_ev before consumer_fold");
  if (!(target_white > 0.0f && target_white <= 255.0f)) return fail(b, HALO_FATAL, "consumer_auto_ev: target_white must lie in (0, 255]");
  HIPCHK(b, hipSetDevice(b->device));
  const uint32_t w = static_cast<uint32_t>(b->cons.w), h = static_cast<uint32_t>(b->cons.h), npix = w * h;
  // ComputeP99Y's fallback order (:80-86): the coarse path only for f > 1 and a grid that does not collapse
  const uint32_t f = downsample_factor > 1 ? static_cast<uint32_t>(downsample_factor) : 1u;
  const bool coarse = f > 1u && w / f > 0u && h / f > 0u;
  const uint32_t wc = coarse ? w / f : 0u, hc = coarse ? h / f : 0u;
  const uint32_t n_vals = coarse ? wc * hc : npix;
  HIPCHK(b, b->cons.aev_vals.reserve(n_vals));
  constexpr size_t kRecWords = sizeof(AevRecord) / sizeof(uint32_t);
  HIPCHK(b, b->cons.aev_ws.reserve(kRecWords + kAevHistWords));
  AevRecord* rec_dev = reinterpret_cast<AevRecord*>(b->cons.aev_ws.ptr);
  hipError_t e = launch_aev_values(b->cons.sum.ptr, b->cons.comp.ptr, w, h, f, wc, hc, b->cons.aev_vals.ptr, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_aev value kernel launch");
  const bool one_wg = b->opt.aev_select < 0 ? n_vals <= kAevSmallMax : b->opt.aev_select == 1;
  e = launch_aev_select(b->cons.aev_vals.ptr, n_vals, rec_dev, b->cons.aev_ws.ptr + kRecWords, one_wg, b->opt.aev_agg_hist != 0, b->cu_count, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_aev select kernel launch");
  AevRecord rec{};
  HIPCHK(b, hipMemcpyAsync(&rec, rec_dev, sizeof(rec), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  float p99 = 0.0f;
  if (rec.count) std::memcpy(&p99, &rec.p99_bits, sizeof(float));
  if (coarse) p99 = p99 / (static_cast<float>(f) * static_cast<float>(f));   // the fine-equivalent P99 (:112-113)
  const float per_pixel = per_pixel_intensity(b, b->cons.w * b->cons.h);
  out->p99_y = p99;
  out->per_pixel_intensity = per_pixel;
  out->ev_auto = halo_host_ev_auto(p99, per_pixel, target_white);
  out->produced = (p99 > 0.0f && per_pixel > 0.0f) ? 1 : 0;
  out->value_count = rec.count;
  out->coarse_w = static_cast<int32_t>(wc);
  out->coarse_h = static_cast<int32_t>(hc);
  return HALO_OK;
}

// ---- image statistics (halo_stats.hip) --------------------------------------------------------------------------
int halo_consumer_stats(halo_handle_t b, const HaloStatsSpec* spec, HaloImageStats* out) {
  if (!b) return HALO_FATAL;
  if (!spec || !out) return fail(b, HALO_FATAL, "consumer_stats: spec or out is NULL");
  if (spec->percentile_count < 0 || spec->percentile_count > HALO_STATS_MAX_PERCENTILES)
    return fail(b, HALO_FATAL, "consumer_stats: percentile_count must lie in 0 .. 16");
  StatsAsk ask{};
  ask.count = static_cast<uint32_t>(spec->percentile_count);
  for (uint32_t j = 0; j < ask.count; j++) {
    if (!(spec->percentiles[j] >= 0.0 && spec->percentiles[j] <= 100.0)) return fail(b, HALO_FATAL, "consumer_stats: a percentile lies outside [0, 100]");
    ask.q[j] = spec->percentiles[j] / 100.0;
  }
  const bool lane = spec->plane >= 0;
  int w = b->cons.w, h = b->cons.h;
  if (lane) {
    if (spec->plane >= static_cast<int>(b->color_classes.size()) || !b->lanes.ptr || b->lanes_w <= 0 || b->lanes_h <= 0)
      return fail(b, HALO_FATAL, "consumer_stats: no such class lane (halo_set_color's class count; lanes exist after a colour session or halo_consumer_load_lanes)");
    w = b->lanes_w;
    h = b->lanes_h;
  } else if (spec->plane != HALO_STATS_PLANE_Y) {
    return fail(b, HALO_FATAL, "consumer_stats: plane must be HALO_STATS_PLANE_Y or a lane index");
  } else if (!b->cons.sum.ptr) {
    return fail(b, HALO_FATAL, "consumer_stats before consumer_fold");
  }
  HIPCHK(b, hipSetDevice(b->device));
  if (lane)
    if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be adding to the lanes on the trace / auxiliary streams)
  const uint32_t npix = static_cast<uint32_t>(w) * static_cast<uint32_t>(h);
  const float per_pixel = per_pixel_intensity(b, static_cast<int>(npix));
  const float norm = spec->norm > 0.0f ? spec->norm : per_pixel;
  std::memset(out, 0, sizeof(*out));
  out->pixel_count = npix;
  out->norm = norm;
  out->percentile_count = spec->percentile_count;
  if (!(norm > 0.0f)) return HALO_OK;   // no landed intensity to normalise by: nothing produced
  HIPCHK(b, b->cons.aev_vals.reserve(npix));
  HIPCHK(b, b->cons.stats_ws.reserve(kStatsWsWords));
  const bool one_wg = b->opt.stats_select < 0 ? npix <= kStatsSmallMax : b->opt.stats_select == 1;
  const double* lane_ptr = lane ? b->lanes.ptr + static_cast<size_t>(spec->plane) * npix : nullptr;
  hipError_t e = launch_stats(b->cons.sum.ptr, b->cons.comp.ptr, lane_ptr, npix, norm, ask, b->cons.aev_vals.ptr, b->cons.stats_ws.ptr, one_wg, b->cu_count, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_stats kernel launch");
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the record's bins are 64-bit words");
  auto rec = std::make_unique<StatsRecord>();
  HIPCHK(b, hipMemcpyAsync(rec.get(), b->cons.stats_ws.ptr, sizeof(StatsRecord), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  if (rec->sel.n == 0u) return HALO_OK;
  out->positive_count = rec->sel.n;
  out->saturated_count = rec->sat;
  const uint64_t* bins = reinterpret_cast<const uint64_t*>(rec->bins);
  out->sum = host::BinnedSum(bins, false);
  out->sum_sq = host::BinnedSum(bins + kStatsExpBins, true);
  std::memcpy(&out->max, &rec->max_bits, sizeof(float));
  out->produced = 1;
  for (uint32_t j = 0; j < ask.count; j++) {
    out->rank[j] = rec->rank[j];
    out->frac[j] = rec->frac[j];
    std::memcpy(&out->lo[j], &rec->lo_bits[j], sizeof(float));
    std::memcpy(&out->hi[j], &rec->hi_bits[j], sizeof(float));
    const double lo = out->lo[j], hi = out->hi[j];
    out->value[j] = lo + (hi - lo) * out->frac[j];   // (three roundings: this file is built without contraction)
  }
  return HALO_OK;
}

// ---- the view stage (halo_view.hip): the consumer's image through another lens -------------------------------
int halo_consumer_view(halo_handle_t b, const HaloViewSpec* spec, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out) {
  return view_call(b, "consumer_view", spec, nullptr, rgb_out, xyz_out, map_out, dir_out, nullptr);
}

int halo_consumer_view_filtered(halo_handle_t b, const HaloViewSpec* spec, const HaloViewFilter* filter, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out,
                                float* tap_out) {
  if (!b) return HALO_FATAL;
  if (!filter) return fail(b, HALO_FATAL, "consumer_view_filtered: filter is NULL");
  if (filter->filter != HALO_VIEW_NEAREST && filter->filter != HALO_VIEW_BILINEAR) return fail(b, HALO_FATAL, "consumer_view_filtered: unknown filter");
  if (filter->blend != 0 && filter->blend != 1) return fail(b, HALO_FATAL, "consumer_view_filtered: blend must be 0 or 1");
  if (filter->reserved[0] != 0 || filter->reserved[1] != 0) return fail(b, HALO_FATAL, "consumer_view_filtered: reserved words must be zero");
  return view_call(b, "consumer_view_filtered", spec, filter, rgb_out, xyz_out, map_out, dir_out, tap_out);
}

// ---- display-side composite of the class lanes (server/component_compositor.cpp) -------------------------
int halo_consumer_load_lanes(halo_handle_t b, const float* lanes, int width, int height, int class_count, double total_intensity) {
  if (!b || !lanes) return HALO_FATAL;
  if (b->in_session) return fail(b, HALO_FATAL, "consumer_load_lanes inside a session");
  if (width <= 0 || height <= 0 || class_count <= 0 || class_count != static_cast<int>(b->color_classes.size()))
    return fail(b, HALO_FATAL, "consumer_load_lanes: class count must equal halo_set_color's, image must not be empty");
  if (static_cast<uint64_t>(width) * static_cast<uint64_t>(height) > (1ull << 25)) return fail(b, HALO_UNAVAILABLE, "more than 2^25 pixels");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  const size_t n = static_cast<size_t>(class_count) * width * height;
  HIPCHK(b, b->lanes.reserve(n));
  b->lanes_w = width;
  b->lanes_h = height;
  HIPCHK(b, b->cons.lanes_stage.reserve(n));
  HIPCHK(b, hipMemcpyAsync(b->cons.lanes_stage.ptr, lanes, n * sizeof(float), hipMemcpyHostToDevice, main_q(b)));
  hipError_t e = launch_lanes_load(b->cons.lanes_stage.ptr, b->lanes.ptr, n, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_lanes_load_kernel launch");
  HIPCHK(b, hipStreamSynchronize(main_q(b)));   // `lanes` is the caller's (pageable) memory
  if (total_intensity >= 0.0) b->cons.total_intensity = total_intensity;
  return HALO_OK;
}

int halo_consumer_composite(halo_handle_t b, const HaloComposite* spec, float* linear_rgb_out, uint8_t* srgb_out, float* participating_p99_y, int32_t* produced) {
  if (!b || !spec || !produced) return HALO_FATAL;
  *produced = 0;
  CompositePlan plan;
  if (int rc = composite_prepare(b, "consumer_composite", spec, &plan)) return rc;
  if (plan.state == kCompositeNothing) return HALO_OK;   // component_compositor.cpp:183-185: nothing is touched
  const size_t n3 = static_cast<size_t>(plan.npix) * 3u;
  if (plan.state == kCompositeBlack) {   // "nothing visible -> all-black, still a valid composite" (:201-206)
    if (linear_rgb_out) std::memset(linear_rgb_out, 0, n3 * sizeof(float));
    if (srgb_out) std::memset(srgb_out, 0, n3);
    if (participating_p99_y) *participating_p99_y = 0.0f;
    *produced = 1;
    return HALO_OK;
  }
  if (participating_p99_y) *participating_p99_y = plan.p99;
  if (plan.state == kCompositeNoScale) {   // :209-214: P99 published, no composite; the linear buffer was already assigned zeros (:189)
    if (linear_rgb_out) std::memset(linear_rgb_out, 0, n3 * sizeof(float));
    return HALO_OK;
  }
  if (linear_rgb_out) HIPCHK(b, b->cons.comp_rgb.reserve(n3));
  if (srgb_out) HIPCHK(b, b->cons.rgb.reserve(n3));
  if (linear_rgb_out || srgb_out) {
    hipError_t e = launch_composite(b->lanes.ptr, plan.npix, plan.cd, linear_rgb_out ? b->cons.comp_rgb.ptr : nullptr, srgb_out ? b->cons.rgb.ptr : nullptr, b->cu_count * 8,
                                    main_q(b));
    if (e != hipSuccess) return hip_fail(b, e, "halo_composite_kernel launch");
    if (linear_rgb_out) HIPCHK(b, hipMemcpyAsync(linear_rgb_out, b->cons.comp_rgb.ptr, n3 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
    if (srgb_out) HIPCHK(b, hipMemcpyAsync(srgb_out, b->cons.rgb.ptr, n3, hipMemcpyDeviceToHost, main_q(b)));
    HIPCHK(b, hipStreamSynchronize(main_q(b)));
  }
  *produced = 1;
  return HALO_OK;
}

// ---- the raypath-colour images through another lens (halo_view_composite.hip) -------------------------------------
// The reference's preview in RGB mode (gui/preview_renderer.cpp:458-464, 660-678): stage 1 is halo_consumer_composite's source image, by its code,
// into a device buffer that stays there; stage 2 gathers the view from its bytes.
int halo_consumer_view_composite(halo_handle_t b, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloComposite* composite, uint8_t* srgb_out,
                                 float* value_out, int32_t* map_out, float* tap_out, float* participating_p99_y, int32_t* produced) {
  if (!b) return HALO_FATAL;
  return view_composite_call(b, "consumer_view_composite", spec, filter, composite, nullptr, srgb_out, value_out, nullptr, nullptr, map_out, tap_out, nullptr,
                             participating_p99_y, produced);
}

// ---- the auxiliary lines over a view (halo_view_overlay.hip, halo_overlay.h) ---------------------------------------------------------------
int halo_consumer_view_overlay(halo_handle_t b, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloViewOverlay* overlay, uint8_t* rgb_out, float* value_out,
                               float* sky_out, float* marks_out, int32_t* map_out, float* dir_out) {
  if (!b) return HALO_FATAL;
  const std::string name("consumer_view_overlay");
  if (filter)
    if (const char* why = filter_refusal(filter)) return fail(b, HALO_FATAL, name + why);
  if (!overlay) return fail(b, HALO_FATAL, name + ": overlay is NULL");
  if (const char* why = host::ViewOverlayRefusal(*overlay)) return fail(b, HALO_FATAL, name + ": " + why);
  const bool draw = rgb_out || value_out;
  ViewPlan plan;
  const ViewWant want{draw, false, map_out != nullptr, draw || sky_out || dir_out, false};
  if (int rc = view_launch(b, name.c_str(), spec, filter, want, rgb_out || value_out || sky_out || marks_out || map_out || dir_out, &plan)) return rc;
  if (draw && plan.scale == 0.0f) HIPCHK(b, hipMemsetAsync(b->cons.view_rgb.ptr, 0, plan.n, main_q(b)));   // PostSnapshot's early-out: the lines lie on zero bytes
  if (int rc = overlay_pass(b, spec->view, *overlay, draw, value_out, sky_out, marks_out)) return rc;
  if (rgb_out) HIPCHK(b, hipMemcpyAsync(rgb_out, b->cons.view_rgb.ptr, plan.n, hipMemcpyDeviceToHost, main_q(b)));
  return view_copy_back(b, plan, nullptr, nullptr, map_out, dir_out, nullptr);
}

int halo_consumer_view_composite_overlay(halo_handle_t b, const HaloViewSpec* spec, const HaloViewFilter* filter, const HaloComposite* composite,
                                         const HaloViewOverlay* overlay, uint8_t* srgb_out, float* value_out, float* sky_out, float* marks_out, int32_t* map_out,
                                         float* tap_out, float* dir_out, float* participating_p99_y, int32_t* produced) {
  if (!b) return HALO_FATAL;
  const std::string name("consumer_view_composite_overlay");
  if (!overlay) return fail(b, HALO_FATAL, name + ": overlay is NULL");
  if (const char* why = host::ViewOverlayRefusal(*overlay)) return fail(b, HALO_FATAL, name + ": " + why);
  return view_composite_call(b, name, spec, filter, composite, overlay, srgb_out, value_out, sky_out, marks_out, map_out, tap_out, dir_out, participating_p99_y, produced);
}

int halo_consumer_view_lanes(halo_handle_t b, const HaloViewSpec* spec, const HaloViewFilter* filter, float* lanes_out, int32_t* map_out, float* tap_out) {
  if (!b) return HALO_FATAL;
  const std::string name("consumer_view_lanes");
  const HaloRender* source = nullptr;
  if (int rc = lane_view_checks(b, name, spec, filter, lanes_out || map_out || tap_out, &source)) return rc;
  const HaloRender& view = spec->view;
  const size_t npix = static_cast<size_t>(view.width) * static_cast<size_t>(view.height);
  const size_t classes = b->color_classes.size();
  if (classes == 0) return fail(b, HALO_FATAL, name + ": no classes (halo_set_color)");
  if (static_cast<uint64_t>(classes) * npix > (1ull << 27)) return fail(b, HALO_UNAVAILABLE, name + ": class_count x view pixels of more than 2^27 floats");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be adding to the lanes on the trace / auxiliary streams)
  if (lanes_out) HIPCHK(b, b->cons.view_lanes.reserve(classes * npix));
  if (map_out) HIPCHK(b, b->cons.view_map.reserve(npix));
  if (tap_out) HIPCHK(b, b->cons.view_tap.reserve(npix * 5));
  hipError_t e = launch_view_lanes(b->lanes.ptr, static_cast<uint32_t>(classes), host::BuildProj(view), host::BuildProj(*source), filter && filter->filter == HALO_VIEW_BILINEAR,
                                   filter && filter->blend != 0, lanes_out ? b->cons.view_lanes.ptr : nullptr, map_out ? b->cons.view_map.ptr : nullptr,
                                   tap_out ? b->cons.view_tap.ptr : nullptr, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_view_lanes_kernel launch");
  if (lanes_out) HIPCHK(b, hipMemcpyAsync(lanes_out, b->cons.view_lanes.ptr, classes * npix * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  if (map_out) HIPCHK(b, hipMemcpyAsync(map_out, b->cons.view_map.ptr, npix * sizeof(int32_t), hipMemcpyDeviceToHost, main_q(b)));
  if (tap_out) HIPCHK(b, hipMemcpyAsync(tap_out, b->cons.view_tap.ptr, npix * 5 * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  return HALO_OK;
}

// ---- the class lanes out (the seam's float lanes) ----------------------------------------------------------
int halo_readback_class_lanes(halo_handle_t b, float* lanes, int width, int height, int class_count) {
  if (!b || !lanes) return HALO_FATAL;
  if (class_count != static_cast<int>(b->color_classes.size()) || width != b->lanes_w || height != b->lanes_h || !b->lanes.ptr)
    return fail(b, HALO_FATAL, "class lanes: size does not match the session (classes x width x height)");
  HIPCHK(b, hipSetDevice(b->device));
  if (int rc = join_aux(b)) return rc;   // (kernels of queued sessions may still be running on the trace / auxiliary streams)
  const size_t n = static_cast<size_t>(class_count) * width * height;
  // the lanes are summed in fp64 on the device (hot pixels), the seam hands out floats (trace_backend.hpp:471-493): narrowed and drained by
  // one kernel into the staging buffer, so half the bytes cross the bus and no host pass follows
  HIPCHK(b, b->cons.lanes_stage.reserve(n));
  hipError_t e = launch_lanes_drain(b->lanes.ptr, b->cons.lanes_stage.ptr, n, b->cu_count * 8, main_q(b));
  if (e != hipSuccess) return hip_fail(b, e, "halo_lanes_drain_kernel launch");
  HIPCHK(b, hipMemcpyAsync(lanes, b->cons.lanes_stage.ptr, n * sizeof(float), hipMemcpyDeviceToHost, main_q(b)));
  HIPCHK(b, hipStreamSynchronize(main_q(b)));
  return HALO_OK;
}

}  // extern "C"
