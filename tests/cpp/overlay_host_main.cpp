// overlay_host_main.cpp — the host half of the view stage's auxiliary lines (halo_host.cpp ViewOverlayDefaults, ViewOverlayRefusal, ViewOverlayMarks,
// ViewSky, ViewOverlayPixel: halo_overlay.h, the code the device pass runs) as a stand-alone program: tests/test_cpp_overlay_host.py builds it from
// the host sources alone with -fsanitize=address,undefined and runs it on the CPU.  It sweeps all eleven lenses as views over odd and even sizes,
// builds every pixel's sky coordinates and quad footprint with the header's own functions and draws every layer, with records at their limits:
// sixteen circles, radius 0, a 0.5-degree grid, alphas 0 and 1.  No GPU, no HIP runtime, nothing loaded into Python.  Prints "ok" and returns 0, or
// says what was wrong and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ice_halo_sim_amd/csrc/halo_host.hpp"
#include "../../ice_halo_sim_amd/csrc/halo_overlay.h"

using namespace halo;
using namespace halo::host;

static int failures = 0;
#define EXPECT(c)                                       \
  do {                                                  \
    if (!(c)) {                                         \
      if (failures < 20) std::printf("line %d: %s\n", __LINE__, #c); \
      failures++;                                       \
    }                                                   \
  } while (0)

static HaloRender Render(int lens, int w, int h, float fov, float az, float el, float ro, int visible, float overlap) {
  HaloRender r{};
  r.lens_type = lens;
  r.fov = fov;
  r.width = w;
  r.height = h;
  r.view_az = az;
  r.view_el = el;
  r.view_ro = ro;
  r.visible = visible;
  r.overlap = overlap;
  return r;
}
static float Fov(int lens) { return lens == HALO_LENS_LINEAR ? 90.0f : lens == HALO_LENS_GLOBE ? 60.0f : lens == HALO_LENS_RECTANGULAR ? 360.0f : 180.0f; }

// one view under one record: every pixel's sky6 by the quad rule, every pixel's value
static void Sweep(const HaloRender& view, const HaloViewOverlay& o, long* drawn, long* changed) {
  const int w = view.width, h = view.height;
  std::vector<float> sky(static_cast<size_t>(w) * h * 3, 0.0f);
  std::vector<char> has(static_cast<size_t>(w) * h, 0);
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      float d[3];
      if (!ViewDirection(view, x, y, d)) continue;
      has[static_cast<size_t>(y) * w + x] = 1;
      ViewSky(d, o.sun_dir, &sky[(static_cast<size_t>(y) * w + x) * 3]);
    }
  float marks[9];
  ViewOverlayMarks(view, o.sun_dir, marks);
  for (int j = 0; j < 9; j++) EXPECT(std::isfinite(marks[j]));
  auto at = [&](int x, int y) -> const float* { return x >= 0 && x < w && y >= 0 && y < h && has[static_cast<size_t>(y) * w + x] ? &sky[(static_cast<size_t>(y) * w + x) * 3] : nullptr; };
  for (int y = 0; y < h; y++)
    for (int x = 0; x < w; x++) {
      const float* q = at(x, y);
      if (!q) continue;
      const float* qx = at(x ^ 1, y);
      if (!qx) qx = at((x & 1) ? x + 1 : x - 1, y);
      const float* qy = at(x, y ^ 1);
      if (!qy) qy = at(x, (y & 1) ? y + 1 : y - 1);
      float tx[3] = {0, 0, 0}, ty[3] = {0, 0, 0}, sky6[6] = {q[0], q[1], q[2], 0, 0, 0};
      for (int j = 0; j < 3; j++) {
        if (qx) tx[j] = overlay_fw_term(qx[j], q[j], j == 1);
        if (qy) ty[j] = overlay_fw_term(qy[j], q[j], j == 1);
      }
      overlay_footprint(tx, ty, sky6 + 3);
      EXPECT(sky6[3] >= 1e-4f && sky6[3] <= 2.0f && sky6[4] >= 1e-4f && sky6[4] <= 5.0f && sky6[5] >= 1e-4f && sky6[5] <= 2.0f);
      EXPECT(q[0] >= -90.001f && q[0] <= 90.001f && q[1] >= -180.001f && q[1] <= 180.001f && q[2] >= 0.0f && q[2] <= 180.001f);
      const uint8_t base[3] = {static_cast<uint8_t>(x * 7), static_cast<uint8_t>(y * 5), 200};
      const float xy[2] = {static_cast<float>(x), static_cast<float>(y)};
      float v[3];
      ViewOverlayPixel(base, sky6, xy, marks, o, v);
      for (int j = 0; j < 3; j++) {
        EXPECT(v[j] >= -1e-3f && v[j] <= 255.001f);   // a mix of values in [0, 255] stays there
        if (overlay_byte(v[j]) != base[j]) ++*changed;
      }
      ++*drawn;
    }
}

int main() {
  const float sun_a[2] = {25.0f, 10.0f}, sun_b[2] = {-90.0f, 0.0f};
  HaloViewOverlay def{};
  ViewOverlayDefaults(60.0f, sun_a, &def);
  EXPECT(ViewOverlayRefusal(def) == nullptr);
  EXPECT(def.grid_step_deg == 20.0f && def.sun_circle_count == 2 && def.show_grid == 0);
  HaloViewOverlay all = def;
  all.show_horizon = all.show_grid = all.show_sun_circles = all.show_zenith_nadir = all.show_sun_marker = 1;
  HaloViewOverlay limits{};
  ViewOverlayDefaults(1.0f, sun_b, &limits);   // the sun at the nadir, the finest grid
  limits.show_horizon = limits.show_grid = limits.show_sun_circles = limits.show_zenith_nadir = limits.show_sun_marker = 1;
  limits.sun_circle_count = HALO_VIEW_MAX_SUN_CIRCLES;
  for (int i = 0; i < HALO_VIEW_MAX_SUN_CIRCLES; i++) limits.sun_circle_deg[i] = 180.0f * static_cast<float>(i + 1) / HALO_VIEW_MAX_SUN_CIRCLES;
  limits.zenith_nadir_radius_px = limits.sun_marker_radius_px = 0.0f;
  limits.horizon_alpha = limits.sun_marker_alpha = 1.0f;
  limits.grid_alpha = 0.0f;
  EXPECT(ViewOverlayRefusal(limits) == nullptr);
  HaloViewOverlay off = def;   // every switch off: the base bytes
  const int sizes[][2] = {{37, 23}, {16, 16}, {17, 33}, {1, 1}, {5, 300}};
  long drawn = 0, changed = 0, off_changed = 0, off_drawn = 0;
  for (int lens = HALO_LENS_LINEAR; lens <= HALO_LENS_GLOBE; lens++)
    for (const auto& s : sizes)
      for (int look = 0; look < 2; look++) {
        const HaloRender view = Render(lens, s[0], s[1], Fov(lens), look ? 40.0f : 0.0f, look ? 25.0f : 0.0f, look ? 10.0f : 0.0f, look ? HALO_VISIBLE_UPPER : HALO_VISIBLE_FULL,
                                       look ? 0.2f : 0.0f);
        Sweep(view, all, &drawn, &changed);
        Sweep(view, limits, &drawn, &changed);
        Sweep(view, off, &off_drawn, &off_changed);
      }
  EXPECT(drawn > 0 && changed > 0 && off_drawn > 0 && off_changed == 0);
  // the refusals, one field at a time
  auto refused = [&](auto&& edit) {
    HaloViewOverlay o = all;
    edit(o);
    return ViewOverlayRefusal(o) != nullptr;
  };
  EXPECT(refused([](HaloViewOverlay& o) { o.grid_color[1] = 1.5f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.horizon_alpha = -0.1f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_marker_alpha = NAN; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.grid_step_deg = 0.0f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_circle_count = 17; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_circle_count = -1; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_circle_deg[1] = 0.0f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_circle_deg[0] = 180.5f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.zenith_nadir_radius_px = -1.0f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.sun_dir[0] += 0.01f; }));
  EXPECT(refused([](HaloViewOverlay& o) { o.reserved[1] = 1; }));
  EXPECT(!refused([](HaloViewOverlay& o) { o.show_grid = 0, o.grid_step_deg = 0.0f; }));
  EXPECT(!refused([](HaloViewOverlay& o) { o.show_sun_circles = o.show_sun_marker = 0, o.sun_dir[0] = 5.0f; }));
  // a direction that is no unit vector, signed zeros, the sun itself
  const float odd[][3] = {{0.0f, -0.0f, 1.0f}, {-0.0f, 0.0f, -1.0f}, {3, -4, 12}, {1e-30f, 0, 0}, {def.sun_dir[0], def.sun_dir[1], def.sun_dir[2]}};
  for (const auto& d : odd) {
    float sky[3];
    ViewSky(d, def.sun_dir, sky);
    for (int j = 0; j < 3; j++) EXPECT(std::isfinite(sky[j]));
  }
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
