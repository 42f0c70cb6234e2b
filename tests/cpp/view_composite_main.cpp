// HipTraceBackend::ViewComposite and ViewLanes from a plain C++ host: three classes, lanes made by an integer rule the Python test repeats
// (tests/test_gpu_view_composite.py), a dual-fisheye source with an overlap band seen through a linear view, bilinear with the blend.  Prints
// FNV-1a checksums of the bytes each call returned; the test compares them with the Python calls'.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ice_halo_sim_amd/csrc/hip_trace_backend.hpp"

static uint64_t fnv1a(const void* data, size_t n) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

int main() {
  try {
    const int W = 128, H = 64, VW = 37, VH = 23, N = 3;
    halo::HipTraceBackend be(0, 5);
    std::vector<HaloColorClass> classes(N);
    for (int c = 0; c < N; c++) {
      std::memset(&classes[c], 0, sizeof(HaloColorClass));
      classes[c].bits = 1ull << c;
    }
    be.SetColor({}, classes);
    std::vector<float> lanes(static_cast<size_t>(N) * W * H);
    for (uint32_t i = 0; i < lanes.size(); i++) lanes[i] = static_cast<float>(((i * 2654435761u) >> 12) & 0xFFFFu) / 65536.0f;
    be.LoadClassLanes(lanes.data(), W, H, N, 1000.0);

    HaloViewSpec spec;
    std::memset(&spec, 0, sizeof(spec));
    spec.has_source = 1;
    spec.source.lens_type = HALO_LENS_DUAL_FISHEYE_EQUAL_AREA;
    spec.source.fov = 180.0f;
    spec.source.width = W;
    spec.source.height = H;
    spec.source.visible = HALO_VISIBLE_FULL;
    spec.source.overlap = 0.1f;
    spec.view.lens_type = HALO_LENS_LINEAR;
    spec.view.fov = 90.0f;
    spec.view.width = VW;
    spec.view.height = VH;
    spec.view.view_az = 40.0f;
    spec.view.view_el = 5.0f;
    spec.view.view_ro = 10.0f;
    spec.view.visible = HALO_VISIBLE_FULL;
    const HaloViewFilter filter = {HALO_VIEW_BILINEAR, 1, {0, 0}};
    HaloComposite comp;
    std::memset(&comp, 0, sizeof(comp));
    comp.mode = HALO_COMPOSITE_ADDITIVE;
    comp.display_exposure_scale = 1.0f;
    comp.intensity_factor = 1.0f;
    comp.class_count = N;
    const float colors[3][3] = {{1.0f, 0.25f, 0.125f}, {0.125f, 1.0f, 0.5f}, {0.25f, 0.5f, 1.0f}};
    for (int c = 0; c < N; c++) {
      std::memcpy(comp.classes[c].color, colors[c], sizeof(colors[c]));
      comp.classes[c].z_order = c;
      comp.classes[c].visible = 1;
    }
    std::vector<uint8_t> srgb(static_cast<size_t>(VW) * VH * 3);
    std::vector<float> value(srgb.size()), tap(static_cast<size_t>(VW) * VH * 5), view_lanes(static_cast<size_t>(N) * VW * VH);
    std::vector<int32_t> map(static_cast<size_t>(VW) * VH);
    float p99 = 0.0f;
    const bool produced = be.ViewComposite(spec, filter, comp, srgb.data(), value.data(), map.data(), tap.data(), &p99);
    be.ViewLanes(spec, filter, view_lanes.data());
    std::printf("produced %d\n", produced ? 1 : 0);
    std::printf("p99 %08x\n", [&] { uint32_t u; std::memcpy(&u, &p99, 4); return u; }());
    std::printf("srgb %016llx\n", static_cast<unsigned long long>(fnv1a(srgb.data(), srgb.size())));
    std::printf("value %016llx\n", static_cast<unsigned long long>(fnv1a(value.data(), value.size() * sizeof(float))));
    std::printf("map %016llx\n", static_cast<unsigned long long>(fnv1a(map.data(), map.size() * sizeof(int32_t))));
    std::printf("tap %016llx\n", static_cast<unsigned long long>(fnv1a(tap.data(), tap.size() * sizeof(float))));
    std::printf("lanes %016llx\n", static_cast<unsigned long long>(fnv1a(view_lanes.data(), view_lanes.size() * sizeof(float))));
    return 0;
  } catch (const halo::BackendUnavailableError& e) {
    std::printf("BackendUnavailableError: %s\n", e.what());
    return 3;
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
}
