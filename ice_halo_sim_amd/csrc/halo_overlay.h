// halo_overlay.h — the auxiliary lines of the view stage (halo_consumer_view_overlay, halo_view_overlay.hip), written once for host AND device: the
// horizon, an altitude / azimuth grid, circles of constant angular distance from the sun, zenith and nadir rings and a sun marker, drawn per
// view pixel from the world direction the gather already has — what the reference's preview shader draws over its image (gui/preview_renderer.cpp
// overlayAuxLines), as a rule of the stage's own:
//   sky          w is the pixel's travel direction (sky position -w), s the sun's; D = 57.29578f:
//                alt = atan2f(-wz, sqrtf(wx wx + wy wy)) D;  az = atan2f(-wy, -wx) D in [-180, 180];  dist = atan2f(|w x s|, w . s) D — the atan2f
//                forms, well conditioned at the poles and at 0 / 180 degrees.
//   footprint    fw(q) = |q(partner_x) - q| + |q(partner_y) - q| over the 2 x 2 quad aligned to even coordinates, (x ^ 1, y) and (x, y ^ 1); a partner
//                outside the view or without a direction is replaced by the pixel's other neighbour on that axis, a term with neither is 0; the
//                azimuth difference is wrapped once (d > 180: d - 360; d < -180: d + 360); fw_alt, fw_dist in [1e-4, 2], fw_az in [1e-4, 5] degrees.
//   coverage     smoothstep(e0, e1, x) = t t (3 - 2 t), t = clamp((x - e0) / (e1 - e0), 0, 1); a line at distance d: 1 - smoothstep(0, 1.5 fw, d).
//   mixing       in BYTE units: c = float(byte), m = colour * 255, mix(c, m, k) = fma(m, k, c (1 - k)): k = 0 gives c and k = 1 gives m, exactly.
//                Layers in this order: grid, sun circles (list order), horizon, zenith ring, nadir ring, sun marker (a filled disc).
// Every operation below is ONE fp32 rounding (the file is built without contraction; the fma of the mix is spelled), so host and device differ by
// libm's atan2f alone: from the same six sky floats both give the same value to the bit.
#ifndef HALO_OVERLAY_H_
#define HALO_OVERLAY_H_

#include <math.h>
#include <stdint.h>

#include "halo_view.h"

namespace halo {

constexpr float kOverlayDeg = 57.29578f;

// what the kernel takes: the caller's record and the three marks {x, y, present} — zenith, nadir, sun — in view pixel coordinates (pixel n's centre at n)
struct OverlayDev {
  HaloViewOverlay o;
  float marks[9];
};

// {alt, az, dist} in degrees of the travel direction w against the sun's travel direction s
HALO_VIEW_HD void overlay_sky(const float w[3], const float s[3], float sky[3]) {
#pragma clang fp contract(off)
  const float rho = sqrtf(w[0] * w[0] + w[1] * w[1]);
  sky[0] = atan2f(-w[2], rho) * kOverlayDeg;
  sky[1] = atan2f(-w[1], -w[0]) * kOverlayDeg;
  const float cx = w[1] * s[2] - w[2] * s[1], cy = w[2] * s[0] - w[0] * s[2], cz = w[0] * s[1] - w[1] * s[0];
  const float cross = sqrtf(cx * cx + cy * cy + cz * cz);
  const float dot = w[0] * s[0] + w[1] * s[1] + w[2] * s[2];
  sky[2] = atan2f(cross, dot) * kOverlayDeg;
}

HALO_VIEW_HD bool overlay_has_dir(const float w[3]) { return w[0] != 0.0f || w[1] != 0.0f || w[2] != 0.0f; }

// one term of a footprint: |q(neighbour) - q|, the azimuth's wrapped once
HALO_VIEW_HD float overlay_fw_term(float q_other, float q, bool azimuth) {
#pragma clang fp contract(off)
  float d = q_other - q;
  if (azimuth) {
    if (d > 180.0f)
      d = d - 360.0f;
    else if (d < -180.0f)
      d = d + 360.0f;
  }
  return fabsf(d);
}

// the footprints {fw_alt, fw_az, fw_dist} from the two terms of each (0 where the axis has no neighbour)
HALO_VIEW_HD void overlay_footprint(const float tx[3], const float ty[3], float fw[3]) {
#pragma clang fp contract(off)
  fw[0] = fminf(fmaxf(tx[0] + ty[0], 1e-4f), 2.0f);
  fw[1] = fminf(fmaxf(tx[1] + ty[1], 1e-4f), 5.0f);
  fw[2] = fminf(fmaxf(tx[2] + ty[2], 1e-4f), 2.0f);
}

HALO_VIEW_HD float overlay_smoothstep(float e0, float e1, float x) {
#pragma clang fp contract(off)
  const float t = fminf(fmaxf((x - e0) / (e1 - e0), 0.0f), 1.0f);
  return t * t * (3.0f - 2.0f * t);
}

HALO_VIEW_HD float overlay_cover(float d, float fw) {
#pragma clang fp contract(off)
  return 1.0f - overlay_smoothstep(0.0f, 1.5f * fw, d);
}

HALO_VIEW_HD float overlay_mod(float x, float g) {
#pragma clang fp contract(off)
  return x - g * floorf(x / g);
}

HALO_VIEW_HD void overlay_mix(float c[3], const float colour[3], float k) {
#pragma clang fp contract(off)
  const float keep = 1.0f - k;
  for (int j = 0; j < 3; j++) c[j] = fmaf(colour[j] * 255.0f, k, c[j] * keep);
}

// The value of one pixel that HAS a direction: base[3] the view's bytes as floats, sky[6] = {alt, az, dist, fw_alt, fw_az, fw_dist}, (px, py) the
// pixel's centre, marks[9] the three marks.  v[3] is the value after the last mix, in byte units.  The switch tests depend on the record alone.
HALO_VIEW_HD void overlay_pixel(const float base[3], const float sky[6], float px, float py, const float marks[9], const HaloViewOverlay& o, float v[3]) {
#pragma clang fp contract(off)
  float c[3] = {base[0], base[1], base[2]};
  const float alt = sky[0], az = sky[1], dist = sky[2];
  if (o.show_grid) {
    const float step = o.grid_step_deg, h = step / 2.0f;
    const float d_alt = overlay_mod(fabsf(alt) + h, step) - h;
    float t = overlay_cover(fabsf(d_alt), sky[3]);
    if (fabsf(alt) < 85.0f) {   // (the azimuth lines crowd together at the poles)
      const float d_az = overlay_mod(az + 180.0f + h, step) - h;
      t = fmaxf(t, overlay_cover(fabsf(d_az), sky[4]));
    }
    overlay_mix(c, o.grid_color, t * o.grid_alpha);
  }
  if (o.show_sun_circles) {
    for (int i = 0; i < o.sun_circle_count; i++) overlay_mix(c, o.sun_circles_color, overlay_cover(fabsf(dist - o.sun_circle_deg[i]), sky[5]) * o.sun_circles_alpha);
  }
  if (o.show_horizon) overlay_mix(c, o.horizon_color, overlay_cover(fabsf(alt), sky[3]) * o.horizon_alpha);
  if (o.show_zenith_nadir) {
    for (int m = 0; m < 2; m++) {
      if (marks[3 * m + 2] == 0.0f) continue;   // (a mark the projection culls)
      const float dx = px - marks[3 * m], dy = py - marks[3 * m + 1];
      const float r = sqrtf(dx * dx + dy * dy);
      overlay_mix(c, o.zenith_nadir_color, (1.0f - overlay_smoothstep(0.0f, 1.5f, fabsf(r - o.zenith_nadir_radius_px))) * o.zenith_nadir_alpha);
    }
  }
  if (o.show_sun_marker && marks[8] != 0.0f) {
    const float dx = px - marks[6], dy = py - marks[7];
    const float r = sqrtf(dx * dx + dy * dy);
    overlay_mix(c, o.sun_marker_color, (1.0f - overlay_smoothstep(o.sun_marker_radius_px - 1.5f, o.sun_marker_radius_px + 1.5f, r)) * o.sun_marker_alpha);
  }
  v[0] = c[0], v[1] = c[1], v[2] = c[2];
}

HALO_VIEW_HD uint8_t overlay_byte(float v) { return static_cast<uint8_t>(floorf(fminf(fmaxf(v, 0.0f), 255.0f) + 0.5f)); }

}  // namespace halo

#endif
