// halo_view.h — the lens inverses of the view stage (halo_consumer_view, halo_view.hip), written once for host AND device.
//
// view_direction gives the world-space exit direction w (the trace kernels' convention: the ray's travel direction, sky position s = -w)
// that a render's lens puts on the CENTRE of pixel (px, py): the w for which project_exit (halo_trace.inl) computes the continuous
// coordinates (px, py) before its floor(. + 0.5).  It is written from the lens definitions and from project_exit / BuildProj, with the
// same scale, lens shift, rotation, az0, r_scale and circle layout:
//   single-view lenses   u = -(px - w/2 - shift_x) / scale, v = (py - h/2 - shift_y) / scale, r = |(u, v)| is the lens form of the camera-space
//                        direction c = R^T s:  linear (u, v) = (cx, cy) / cz;  equal area r^2 = 1 - cz;  equidistant r = theta / (pi/2);
//                        stereographic r = tan(theta / 2);  orthographic r = sin(theta).  The fisheyes stop at their rim r = 1 (cz = 0, which
//                        project_exit culls); s = R c; a direction the view's visible range culls in project_exit is no direction here.
//   dual lenses          the left / right circle layout of dual_to_pixel: the pixel belongs to the circle (left first) whose disc — radius 1 in
//                        the r_scale'd units of the form, i.e. out to the end of the overlap band — contains its centre.  A pixel in the band
//                        gets the direction of the OTHER hemisphere whose overlap write lands on it.  (The disc's last ring, |sz| = max_abs_dz,
//                        and the right circle's horizon ring are written by no exit: no direction there.)
//   rectangular          lon - az0 = (px - w/2) / scale, lat = -(py - h/2) / scale, inside |lon - az0| <= pi and |lat| <= pi/2.  A row whose
//                        centres are a pole keeps the longitude in a tilt of |cos(lat)| ~ 4e-8, which project_exit's atan2f reads back.
//   globe                the unit sphere seen from distance 4: the near intersection of the pixel's ray, inside the limb u^2 + v^2 < 1/15.
// Every sum of products is spelled as the HALO_FMA chain it is evaluated as (see halo_trace.inl), so host and device differ by libm only.
#ifndef HALO_VIEW_H_
#define HALO_VIEW_H_

#include <math.h>
#include <stdint.h>

#include "halo_device.h"

#if defined(__HIPCC__)
#define HALO_VIEW_HD __host__ __device__ inline
#else
#define HALO_VIEW_HD inline
#endif

#ifndef HALO_FMA   // (halo_trace.inl's, when that came first)
#if defined(HALO_STRICT) && HALO_STRICT
#define HALO_FMA(a, b, c) ((a) * (b) + (c))
#else
#define HALO_FMA(a, b, c) fmaf((a), (b), (c))
#endif
#endif

namespace halo {

constexpr float kViewPiF = 3.14159265358979323846f;    // LM_PI_F, LM_PI_2F: the float constants project_exit uses
constexpr float kViewPi2F = 1.5707963267948966f;
constexpr float kViewGlobeD = 4.0f;                     // the globe's camera distance

// lens families: what halo_view_kernel is instantiated for
enum { kViewSingle = 0, kViewDual = 1, kViewRect = 2, kViewGlobe = 3 };
HALO_VIEW_HD int view_family(int lens) {
  if (lens == HALO_LENS_RECTANGULAR) return kViewRect;
  if (lens == HALO_LENS_GLOBE) return kViewGlobe;
  if (lens == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA || lens == HALO_LENS_DUAL_FISHEYE_EQUIDISTANT || lens == HALO_LENS_DUAL_FISHEYE_STEREOGRAPHIC ||
      lens == HALO_LENS_DUAL_FISHEYE_ORTHOGRAPHIC)
    return kViewDual;
  return kViewSingle;
}

// the four floats project_exit reads behind its ProjDev (ProjLds / DispatchParams::proj_pre)
HALO_VIEW_HD void view_proj_pre(const ProjDev& p, float pre[4]) {
  pre[0] = static_cast<float>(p.img_w) / 2.0f;
  pre[1] = static_cast<float>(p.img_h) / 2.0f;
  pre[2] = static_cast<float>(p.lens_shift_x);
  pre[3] = static_cast<float>(p.lens_shift_y);
}

// Inverse of the four fisheye forms: (x, y) = form(dx, dy, dz, rs) -> the unit (dx, dy, dz).  `rim`: dz may not go below it (0 for the
// single-view lenses; a dual circle's disc is bounded by its radius instead: pass -2).  false = outside the form's image.
HALO_VIEW_HD bool view_form_inverse(int form, float x, float y, float rs, float rim, float d[3]) {
  const float xn = x / rs, yn = y / rs;
  const float r2 = HALO_FMA(xn, xn, yn * yn);
  float k, dz;
  if (form == 0) {          // equal area: r^2 = 1 - dz, (x, y) = (dx, dy) / sqrt(1 + dz)
    dz = 1.0f - r2;
    if (!(dz >= -1.0f)) return false;
    k = sqrtf(1.0f + dz);
  } else if (form == 1) {   // equidistant: r = theta / (pi/2), (x, y) = (dx, dy) theta / (pi/2 rho)
    const float r = sqrtf(r2), theta = r * kViewPi2F;
    if (!(theta <= kViewPiF)) return false;
    dz = cosf(theta);
    k = r > 0.0f ? sinf(theta) / r : 0.0f;
  } else if (form == 2) {   // stereographic: r = tan(theta / 2); dz = (1 - r^2) / (1 + r^2), rho / r = 2 / (1 + r^2)
    const float q = 1.0f + r2;
    dz = (1.0f - r2) / q;
    k = 2.0f / q;
  } else {                  // orthographic: r = rho
    const float c2 = 1.0f - r2;
    if (!(c2 >= 0.0f)) return false;
    dz = sqrtf(c2);
    k = 1.0f;
  }
  if (!(dz > rim)) return false;
  d[0] = k * xn;
  d[1] = k * yn;
  d[2] = dz;
  return true;
}

HALO_VIEW_HD int view_form_of(int lens) {
  if (lens == HALO_LENS_FISHEYE_EQUAL_AREA || lens == HALO_LENS_DUAL_FISHEYE_EQUAL_AREA) return 0;
  if (lens == HALO_LENS_FISHEYE_EQUIDISTANT || lens == HALO_LENS_DUAL_FISHEYE_EQUIDISTANT) return 1;
  if (lens == HALO_LENS_FISHEYE_STEREOGRAPHIC || lens == HALO_LENS_DUAL_FISHEYE_STEREOGRAPHIC) return 2;
  return 3;
}

// pre: view_proj_pre(p).  family >= 0: the lens family, known at compile time (else read from p).  w = 0 and false where the pixel has no direction.
HALO_VIEW_HD bool view_direction(const ProjDev& p, const float pre[4], int px, int py, float w[3], int family = -1) {
  w[0] = w[1] = w[2] = 0.0f;
  const int t = p.proj_type;
  const int fam = family >= 0 ? family : view_family(t);
  const float fpx = static_cast<float>(px), fpy = static_cast<float>(py);
  if (fam == kViewSingle || fam == kViewGlobe) {
    const float u = -((fpx - pre[0]) - pre[2]) / p.scale, v = ((fpy - pre[1]) - pre[3]) / p.scale;
    float c[3];
    if (fam == kViewGlobe) {
      // (u, v) = (cx, cy) / (4 + cz) on the unit sphere: (q + 1) cz^2 + 8 q cz + 16 q - 1 = 0 with q = u^2 + v^2, near root
      const float q = HALO_FMA(u, u, v * v);
      const float disc = HALO_FMA(-15.0f, q, 1.0f);
      if (!(disc > 0.0f)) return false;
      c[2] = -(HALO_FMA(kViewGlobeD, q, sqrtf(disc))) / (q + 1.0f);
      const float den = kViewGlobeD + c[2];
      c[0] = u * den;
      c[1] = v * den;
    } else if (t == HALO_LENS_LINEAR) {
      const float n = 1.0f / sqrtf(HALO_FMA(u, u, HALO_FMA(v, v, 1.0f)));
      c[0] = u * n;
      c[1] = v * n;
      c[2] = n;
    } else {
      if (!view_form_inverse(view_form_of(t), u, v, 1.0f, 0.0f, c)) return false;
    }
    // c = R^T s  =>  s = R c
    const float sx = HALO_FMA(p.rot[2], c[2], HALO_FMA(p.rot[1], c[1], p.rot[0] * c[0]));
    const float sy = HALO_FMA(p.rot[5], c[2], HALO_FMA(p.rot[4], c[1], p.rot[3] * c[0]));
    const float sz = HALO_FMA(p.rot[8], c[2], HALO_FMA(p.rot[7], c[1], p.rot[6] * c[0]));
    if (fam == kViewSingle && ((p.visible_range == HALO_VISIBLE_UPPER && -sz > 0.0f) || (p.visible_range == HALO_VISIBLE_LOWER && -sz < 0.0f))) return false;
    w[0] = -sx, w[1] = -sy, w[2] = -sz;
    return true;
  }
  if (fam == kViewRect) {
    const float lon = (fpx - static_cast<float>(p.img_w) / 2.0f) / p.scale, lat = -(fpy - static_cast<float>(p.img_h) / 2.0f) / p.scale;
    if (!(fabsf(lon) <= kViewPiF) || !(fabsf(lat) <= kViewPi2F)) return false;
    const float cl = fabsf(cosf(lat)), a = lon + p.az0;   // (|.|: cosf(LM_PI_2F) is -4.4e-8)
    w[0] = -(cl * cosf(a)), w[1] = -(cl * sinf(a)), w[2] = -sinf(lat);
    return true;
  }
  // dual lenses: dual_to_pixel's layout
  const int half_w = p.img_w / 2;
  const int short_res = half_w < p.img_h ? half_w : p.img_h;
  const float r = static_cast<float>(short_res) / 2.0f;
  const float cy = static_cast<float>(p.img_h) / 2.0f, mid = static_cast<float>(p.img_w) / 2.0f;
  const float xn = (fpy - cy) / r;
  const float yl = -(fpx - (mid - r)) / r, yr = (fpx - (mid + r)) / r;
  const bool left = HALO_FMA(xn, xn, yl * yl) <= 1.0f;
  if (!left && !(HALO_FMA(xn, xn, yr * yr) <= 1.0f)) return false;
  float d[3];
  if (!view_form_inverse(view_form_of(t), xn, left ? yl : yr, p.r_scale, -2.0f, d)) return false;
  // the left circle shows the hemisphere sz >= 0 and, in its band, sz down to -max_abs_dz; the right circle the mirror image.  Where
  // project_exit lands nothing the pixel has no direction: the horizon itself belongs to the left circle (sz >= 0 is "upper"), and the overlap
  // write needs |sz| < max_abs_dz — the last ring of a disc is never written.
  if (!(d[2] > 0.0f || fabsf(d[2]) < p.max_abs_dz || (left && d[2] == 0.0f))) return false;
  w[0] = -d[0], w[1] = -d[1], w[2] = left ? -d[2] : d[2];
  return true;
}

// ---- the forward half, continuous: where a direction lands in the source, before the floor ------------------------------------------------
// view_source_pos is project_exit's sibling (halo_trace.inl, which every trace kernel includes and which stays as it is): the same culls, the same
// expressions spelled as the same HALO_FMA chains, the same four floats behind the ProjDev (`pre`), up to — not including — floorf(. + 0.5f).
//   pos[0..1]  the primary hit (fx0, fy0): floorf(fx0 + 0.5f), floorf(fy0 + 0.5f) is project_exit's (px0, py0) — for the rectangular lens before
//              its wrap modulo the width (fx0 is the unwrapped x).  Pixel n's centre is n.  The single-view lenses and the globe add their 0.5
//              BEFORE the lens shift, g = fma(x, scale, w / 2) + 0.5f + shift: their coordinate is g - 0.5f, which is exact for 0.5 <= g < 2^23,
//              so fx0 + 0.5f is g again and the floor is project_exit's on every hit in the frame.
//   pos[2..3]  a dual source's overlap write (fx1, fy1), pos[4] the tent weight t = (max_abs_dz - |sz|) / (2 max_abs_dz) of the reference's
//              sampleDualFisheye (gui/preview_renderer.cpp:152-180) — one difference, one product, one quotient in fp32.  Zeros without a second hit.
// Returns the hit count (0: culled; pos is zeros).  Host and device differ by libm and by the equal-area form's reciprocal square root
// (v_rsq_f32 on the device, as project_exit has it; 1 / sqrtf on the host).  The body is built without contraction beyond what is spelled.
HALO_VIEW_HD float view_rsq(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rsqf(x);
#else
  return 1.0f / sqrtf(x);
#endif
}

// the four fisheye forms of project_exit's dual_forward / fisheye_*: false = the form culls the direction (orthographic, dz < 0; x = y = 0 then)
HALO_VIEW_HD bool view_form_forward(int form, float dx, float dy, float dz, float rs, float& x, float& y) {
#pragma clang fp contract(off)
  x = y = 0.0f;
  if (form == 0) {
    const float k = rs * view_rsq(1.0f + fminf(fmaxf(dz, -1.0f + 1e-6f), 1.0f));
    x = k * dx, y = k * dy;
    return true;
  }
  if (form == 3) {
    if (dz < 0.0f) return false;
    x = rs * dx, y = rs * dy;
    return true;
  }
  const float rho = sqrtf(HALO_FMA(dx, dx, dy * dy));
  if (rho < 1e-10f) return true;
  const float theta = acosf(fminf(fmaxf(dz, -1.0f), 1.0f));
  const float sc = form == 1 ? rs * theta / (kViewPi2F * rho) : rs * tanf(theta / 2.0f) / rho;
  x = sc * dx, y = sc * dy;
  return true;
}

HALO_VIEW_HD int view_source_pos(const ProjDev& src, const float pre[4], float wx, float wy, float wz, float pos[5]) {
#pragma clang fp contract(off)
  pos[0] = pos[1] = pos[2] = pos[3] = pos[4] = 0.0f;
  const int t = src.proj_type;
  const int fam = view_family(t);
  if (fam == kViewSingle) {
    if ((src.visible_range == HALO_VISIBLE_UPPER && wz > 0.0f) || (src.visible_range == HALO_VISIBLE_LOWER && wz < 0.0f)) return 0;
    const float cx = HALO_FMA(src.rot[6], -wz, HALO_FMA(src.rot[3], -wy, src.rot[0] * (-wx)));
    const float cy = HALO_FMA(src.rot[7], -wz, HALO_FMA(src.rot[4], -wy, src.rot[1] * (-wx)));
    const float cz = HALO_FMA(src.rot[8], -wz, HALO_FMA(src.rot[5], -wy, src.rot[2] * (-wx)));
    if (cz <= 0.0f) return 0;
    float x, y;
    if (t == HALO_LENS_LINEAR) {
      x = cx / cz, y = cy / cz;
    } else if (!view_form_forward(view_form_of(t), cx, cy, cz, 1.0f, x, y)) {
      return 0;
    }
    x = -x;
    pos[0] = (HALO_FMA(x, src.scale, pre[0]) + 0.5f + pre[2]) - 0.5f;
    pos[1] = (HALO_FMA(y, src.scale, pre[1]) + 0.5f + pre[3]) - 0.5f;
    return 1;
  }
  if (fam == kViewRect) {
    float lon = atan2f(-wy, -wx) - src.az0;
    const float lat = asinf(fminf(fmaxf(-wz, -1.0f), 1.0f));
    while (lon < -kViewPiF) lon += 2.0f * kViewPiF;
    while (lon > kViewPiF) lon -= 2.0f * kViewPiF;
    pos[0] = HALO_FMA(lon, src.scale, static_cast<float>(src.img_w) / 2.0f);
    pos[1] = HALO_FMA(-lat, src.scale, static_cast<float>(src.img_h) / 2.0f);
    return 1;
  }
  if (fam == kViewDual) {
    const float sx = -wx, sy = -wy, sz = -wz;
    const bool upper = sz >= 0.0f;
    const float z_hemi = upper ? sz : -sz;
    // dual_to_pixel's layout
    const int half_w = src.img_w / 2;
    const int short_res = half_w < src.img_h ? half_w : src.img_h;
    const float r = static_cast<float>(short_res) / 2.0f;
    const float cy = static_cast<float>(src.img_h) / 2.0f;
    const float cxu = static_cast<float>(src.img_w) / 2.0f - r, cxl = static_cast<float>(src.img_w) / 2.0f + r;
    const int form = view_form_of(t);
    float x, y;
    view_form_forward(form, sx, sy, z_hemi, src.r_scale, x, y);   // (project_exit lands a dual form's (0, 0) where the form culls)
    pos[0] = HALO_FMA(upper ? -y : y, r, upper ? cxu : cxl);
    pos[1] = HALO_FMA(x, r, cy);
    if (!(src.max_abs_dz > 0.0f && fabsf(sz) < src.max_abs_dz)) return 1;
    view_form_forward(form, sx, sy, -z_hemi, src.r_scale, x, y);
    pos[2] = HALO_FMA(upper ? y : -y, r, upper ? cxl : cxu);
    pos[3] = HALO_FMA(x, r, cy);
    pos[4] = (src.max_abs_dz - fabsf(sz)) / (2.0f * src.max_abs_dz);
    return 2;
  }
  // globe
  const float cx = HALO_FMA(src.rot[6], -wz, HALO_FMA(src.rot[3], -wy, src.rot[0] * (-wx)));
  const float cy = HALO_FMA(src.rot[7], -wz, HALO_FMA(src.rot[4], -wy, src.rot[1] * (-wx)));
  const float cz = HALO_FMA(src.rot[8], -wz, HALO_FMA(src.rot[5], -wy, src.rot[2] * (-wx)));
  if (cz >= -1.0f / kViewGlobeD) return 0;
  const float denom = kViewGlobeD + cz;
  pos[0] = (HALO_FMA(-cx / denom, src.scale, static_cast<float>(src.img_w) / 2.0f) + 0.5f + static_cast<float>(src.lens_shift_x)) - 0.5f;
  pos[1] = (HALO_FMA(cy / denom, src.scale, static_cast<float>(src.img_h) / 2.0f) + 0.5f + static_cast<float>(src.lens_shift_y)) - 0.5f;
  return 1;
}

}  // namespace halo

#endif
