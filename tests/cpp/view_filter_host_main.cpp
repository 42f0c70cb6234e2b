// view_filter_host_main.cpp — the host half of the filtered view (halo_host.cpp ViewSourcePos: halo_view.h view_source_pos on BuildProj) swept over
// every lens as source, on the directions ViewDirection gives for every pixel of views of every lens, as a stand-alone program:
// tests/test_view_filter_model.py builds it from the host sources alone with -fsanitize=address,undefined and runs it on the CPU.  No GPU, no HIP
// runtime, nothing loaded into Python.  Prints "ok" and returns 0, or says what was wrong and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../ice_halo_sim_amd/csrc/halo_host.hpp"

using halo::host::ViewDirection;
using halo::host::ViewSourcePos;

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

static bool IsDual(int lens) {
  return lens == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA || lens == HALO_LENS_DUAL_FISHEYE_EQUIDISTANT || lens == HALO_LENS_DUAL_FISHEYE_STEREOGRAPHIC ||
         lens == HALO_LENS_DUAL_FISHEYE_ORTHOGRAPHIC;
}
static float Fov(int lens) { return lens == HALO_LENS_LINEAR ? 90.0f : lens == HALO_LENS_GLOBE ? 60.0f : lens == HALO_LENS_RECTANGULAR ? 360.0f : 180.0f; }

// one direction under one source: the record is finite, zeros where it says so, a second hit only in a dual source's band
static int Check(const HaloRender& src, const float d[3]) {
  float pos[5] = {7.0f, 7.0f, 7.0f, 7.0f, 7.0f};
  const int n = ViewSourcePos(src, d, pos);
  EXPECT(n >= 0 && n <= 2);
  for (int j = 0; j < 5; j++) EXPECT(std::isfinite(pos[j]));
  if (n == 0) EXPECT(pos[0] == 0.0f && pos[1] == 0.0f);
  if (n < 2) EXPECT(pos[2] == 0.0f && pos[3] == 0.0f && pos[4] == 0.0f);
  if (n == 2) {
    EXPECT(IsDual(src.lens_type) && src.overlap > 0.0f);
    EXPECT(pos[4] > 0.0f && pos[4] <= 0.5f);
  }
  if (IsDual(src.lens_type) || src.lens_type == HALO_LENS_RECTANGULAR) EXPECT(n >= 1);   // these lenses cull nothing
  if (n >= 1 && src.lens_type == HALO_LENS_RECTANGULAR) EXPECT(pos[0] > -1.0f && pos[0] < float(src.width) + 1.0f && pos[1] > -1.0f && pos[1] < float(src.height) + 1.0f);
  return n;
}

int main() {
  const int sizes[][2] = {{37, 23}, {1, 1}, {5, 300}};
  const float looks[][3] = {{0, 0, 0}, {40, 25, 10}, {-170, -90, 180}};
  long landed = 0, twice = 0;
  for (int sl = HALO_LENS_LINEAR; sl <= HALO_LENS_GLOBE; sl++)
    for (const auto& ss : {sizes[0], sizes[1]})
      for (int sv = 0; sv < 2; sv++)
        for (int ov = 0; ov < (IsDual(sl) ? 3 : 1); ov++) {
          const HaloRender src = Render(sl, ss[0] == 37 ? 128 : ss[0], ss[0] == 37 ? 64 : ss[1], Fov(sl), looks[sv][0], looks[sv][1], looks[sv][2],
                                        sv ? HALO_VISIBLE_UPPER : HALO_VISIBLE_FULL, ov == 0 ? 0.0f : ov == 1 ? 0.1f : sl == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA ? 1.5f : 0.3f, sv ? 3 : 0, sv ? -2 : 0);   // (1.5: the equal-area antipode clamp)
          for (int vl = HALO_LENS_LINEAR; vl <= HALO_LENS_GLOBE; vl++)
            for (const auto& vs : sizes)
              for (const auto& look : {vl & 1 ? looks[1] : looks[2]}) {
                const HaloRender view = Render(vl, vs[0], vs[1], Fov(vl), look[0], look[1], look[2], HALO_VISIBLE_FULL, vl & 1 ? 0.2f : 0.0f, 0, 0);
                for (int py = 0; py < view.height; py++)
                  for (int px = 0; px < view.width; px++) {
                    float d[3];
                    if (!ViewDirection(view, px, py, d)) continue;
                    const int n = Check(src, d);
                    landed += n > 0;
                    twice += n == 2;
                  }
              }
        }
  EXPECT(landed > 0 && twice > 0);
  // the axes, the horizon, the poles, signed zeros, a direction that is no unit vector, an unknown lens
  const float special[][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}, {0.0f, -0.0f, 1.0f}, {-0.0f, 0.0f, -1.0f}, {0, 0, 0}, {3, -4, 12}, {1e-30f, 0, 1}};
  for (int sl = HALO_LENS_LINEAR; sl <= HALO_LENS_GLOBE; sl++)
    for (const auto& d : special) {
      Check(Render(sl, 128, 64, Fov(sl), 0, 0, 0, HALO_VISIBLE_FULL, 0.1f, 0, 0), d);
      Check(Render(sl, 1, 1, Fov(sl), 40, 25, 10, HALO_VISIBLE_LOWER, 0.0f, 3, -2), d);
    }
  float pos[5] = {7.0f, 7.0f, 7.0f, 7.0f, 7.0f};
  const float down[3] = {0.0f, 0.6f, -0.8f};
  EXPECT(ViewSourcePos(Render(11, 128, 64, 180, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), down, pos) == 0 && pos[0] == 0.0f && pos[4] == 0.0f);
  EXPECT(ViewSourcePos(Render(-1, 128, 64, 180, 0, 0, 0, HALO_VISIBLE_FULL, 0, 0, 0), down, pos) == 0);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
