// view_host_main.cpp — the host half of the view stage (halo_host.cpp ViewDirection: halo_view.h view_direction on BuildProj) swept over every
// lens, as a stand-alone program: tests/test_cpp_view_host.py builds it from the host sources alone with -fsanitize=address,undefined and runs it
// on the CPU.  No GPU, no HIP runtime, nothing loaded into Python.  Prints "ok" and returns 0, or says what was wrong and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../ice_halo_sim_amd/csrc/halo_host.hpp"

using halo::host::ViewDirection;

static int failures = 0;
#define EXPECT(c)                                       \
  do {                                                  \
    if (!(c)) {                                         \
      if (failures < 20) std::printf("line %d: %s\n", __LINE__, #c); \
      failures++;                                       \
    }                                                   \
  } while (0)

static HaloRender Render(int lens, int w, int h, float fov, float az, float el, float ro, int visible, float overlap, int sx, int sy) {
  HaloRender r{};
  r.lens_type = lens;
  r.fov = fov;
  r.width = w;
  r.height = h;
  r.lens_shift[0] = sx;
  r.lens_shift[1] = sy;
  r.view_az = az;
  r.view_el = el;
  r.view_ro = ro;
  r.visible = visible;
  r.overlap = overlap;
  return r;
}

// every pixel of the frame and a ring of pixels around it: a direction is a finite unit vector, no direction is three zeros
static long Sweep(const HaloRender& r) {
  long with = 0;
  for (int py = -2; py < r.height + 2; py++)
    for (int px = -2; px < r.width + 2; px++) {
      float d[3] = {7.0f, 7.0f, 7.0f};
      const bool ok = ViewDirection(r, px, py, d);
      const bool inside = px >= 0 && py >= 0 && px < r.width && py < r.height;
      if (!inside) EXPECT(!ok);
      if (!ok) {
        EXPECT(d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f);
        continue;
      }
      with++;
      const double n = std::sqrt(double(d[0]) * d[0] + double(d[1]) * d[1] + double(d[2]) * d[2]);
      EXPECT(std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]));
      EXPECT(std::fabs(n - 1.0) < 1e-3);   // (the globe next to its limb is the loosest: its root is taken of a difference)
      if (r.visible == HALO_VISIBLE_UPPER && (r.lens_type <= HALO_LENS_FISHEYE_STEREOGRAPHIC || r.lens_type == HALO_LENS_FISHEYE_ORTHOGRAPHIC)) EXPECT(!(d[2] > 0.0f));
      if (r.visible == HALO_VISIBLE_LOWER && (r.lens_type <= HALO_LENS_FISHEYE_STEREOGRAPHIC || r.lens_type == HALO_LENS_FISHEYE_ORTHOGRAPHIC)) EXPECT(!(d[2] < 0.0f));
    }
  return with;
}

int main() {
  const int sizes[][2] = {{37, 23}, {96, 54}, {1, 1}, {5, 300}, {64, 64}, {2, 1}};
  const float views[][3] = {{0, 0, 0}, {40, 25, 10}, {0, 90, 0}, {0, -90, 0}, {-170, 5, 180}};
  long total = 0;
  for (int lens = HALO_LENS_LINEAR; lens <= HALO_LENS_GLOBE; lens++) {
    const bool single = lens <= HALO_LENS_FISHEYE_STEREOGRAPHIC || lens == HALO_LENS_FISHEYE_ORTHOGRAPHIC;
    const bool dual = lens == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA || lens == HALO_LENS_DUAL_FISHEYE_EQUIDISTANT || lens == HALO_LENS_DUAL_FISHEYE_STEREOGRAPHIC ||
                      lens == HALO_LENS_DUAL_FISHEYE_ORTHOGRAPHIC;
    const float fovs_linear[] = {60.0f, 90.0f, 179.0f}, fovs_fish[] = {120.0f, 180.0f}, fovs_globe[] = {20.0f, 90.0f}, fovs_rect[] = {360.0f};
    const float* fovs = lens == HALO_LENS_LINEAR ? fovs_linear : lens == HALO_LENS_GLOBE ? fovs_globe : lens == HALO_LENS_RECTANGULAR ? fovs_rect : fovs_fish;
    const int n_fov = lens == HALO_LENS_LINEAR ? 3 : lens == HALO_LENS_RECTANGULAR ? 1 : 2;
    long lens_total = 0;
    for (const auto& s : sizes)
      for (int f = 0; f < n_fov; f++)
        for (const auto& v : views)
          for (int vis = HALO_VISIBLE_UPPER; vis <= HALO_VISIBLE_FULL; vis++)
            for (int ov = 0; ov < (dual ? 2 : 1); ov++)
              for (int sh = 0; sh < ((single || lens == HALO_LENS_GLOBE) ? 2 : 1); sh++)
                lens_total += Sweep(Render(lens, s[0], s[1], fovs[f], v[0], v[1], v[2], vis, ov ? 0.2f : 0.0f, sh ? 3 : 0, sh ? -2 : 0));
    EXPECT(lens_total > 0);
    total += lens_total;
  }
  // the frame's guards and degenerate renders
  float d[3];
  EXPECT(!ViewDirection(Render(HALO_LENS_LINEAR, 0, 0, 60, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), 0, 0, d));
  EXPECT(!ViewDirection(Render(HALO_LENS_LINEAR, -4, 3, 60, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), 0, 0, d));
  EXPECT(!ViewDirection(Render(HALO_LENS_DUAL_FISHEYE_EQUAL_AREA, 1, 1, 180, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), 0, 0, d));   // no circle fits
  EXPECT(ViewDirection(Render(HALO_LENS_LINEAR, 8192, 4096, 60, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), 8191, 4095, d));
  // the centre of an even-sized fisheye looks along the view axis: straight up for el = 90 (travel direction straight down)
  EXPECT(ViewDirection(Render(HALO_LENS_FISHEYE_EQUIDISTANT, 64, 64, 180, 0, 90, 0, HALO_VISIBLE_FULL, 0, 0, 0), 32, 32, d) && d[2] < -0.999999f);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf(total > 0 ? "ok\n" : "nothing swept\n");
  return 0;
}
