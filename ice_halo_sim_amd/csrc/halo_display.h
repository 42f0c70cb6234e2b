// halo_display.h — the consumer's per-pixel display transform, written once: halo_post_snapshot_kernel (halo_kernels.hip) and halo_view_kernel
// (halo_view.hip) both call it, so a view's pixel is the snapshot's pixel byte for byte.  Device code only.
#ifndef HALO_DISPLAY_H_
#define HALO_DISPLAY_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace halo {

struct DisplayDev {
  float scale;
  float ray_color[3];
  float background[3];
};

// PostSnapshot (render.cpp:508-578) for one pixel whose raw snapshot value (sum + comp) is `raw`: scale → gamut clip (color_space.cpp
// GamutClipXyz) → XYZ→linear RGB → background + clamp → sRGB gamma → u8.
__device__ __forceinline__ void display_pixel(const float raw[3], const DisplayDev& dsp, uint8_t out[3]) {
  const float kWhite[3] = {0.95047f, 1.00000f, 1.08883f};                       // kWhitePointD65, util/color_data.hpp:6
  const float kM[9] = {3.2404542f, -1.5371385f, -0.4985314f, -0.9692660f, 1.8760108f, 0.0415560f,
                       0.0556434f, -0.2040259f, 1.0572252f};                    // kXyzToRgb, util/color_data.hpp:8-12
  float xyz[3], rgb[3];
#pragma unroll
  for (int j = 0; j < 3; j++) xyz[j] = raw[j] * dsp.scale;
  if (dsp.ray_color[0] < 0.0f) {
    float gray[3], diff[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      gray[j] = kWhite[j] * xyz[1];
      diff[j] = xyz[j] - gray[j];
    }
    float s = 1.0f;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float a = 0.0f, b = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        a += -gray[k] * kM[j * 3 + k];
        b += diff[k] * kM[j * 3 + k];
      }
      if (a * b > 0.0f && a / b < s) s = a / b;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float v = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) v += (diff[k] * s + gray[k]) * kM[j * 3 + k];
      rgb[j] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      float v = 0.0f;
#pragma unroll
      for (int k = 0; k < 3; k++) v += (kWhite[k] * xyz[1]) * kM[j * 3 + k];
      rgb[j] = v * dsp.ray_color[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    float v = rgb[j] + dsp.background[j];
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    v = (v < 0.0031308f) ? v * 12.92f : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f;
    out[j] = static_cast<uint8_t>(v * 255.0f);
  }
}

}  // namespace halo

#endif
