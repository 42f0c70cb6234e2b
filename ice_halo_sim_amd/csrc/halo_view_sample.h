// halo_view_sample.h — the sampling rule of the filtered views, written once for every image the view stage gathers from: the consumer's XYZ
// (halo_view.hip halo_view_filtered_kernel), the class composite's sRGB bytes and the class lanes (halo_view_composite.hip).  What differs
// between them is how ONE tap is fetched: `Tap` is a small struct with
//     static constexpr int kN                       values per tap (3: a colour; 1: one lane)
//     void operator()(int ix, int iy, float v[kN])  the image's value at source pixel (ix, iy), both inside the frame
//     void at(uint32_t pixel, float v[kN])          the same by row-major index (view_filtered_value's nearest copy)
// Device code only; include after halo_trace.inl.
#ifndef HALO_VIEW_SAMPLE_H_
#define HALO_VIEW_SAMPLE_H_

namespace halo {

constexpr uint32_t kViewTile = 16u;
static_assert(kViewTile * kViewTile == kBlock, "one thread per pixel of a tile");

__device__ __forceinline__ int view_clamp_index(float f, int n) {   // (the float first: whatever f is, the cast is defined)
  return static_cast<int>(fminf(fmaxf(f, 0.0f), static_cast<float>(n - 1)));
}

// The sample at the continuous position (fx, fy), pixel n's centre at n.  Bilinear: columns floor(fx) and floor(fx) + 1 clamped to the frame — or
// taken modulo the width, the rectangular lens's own wrap — rows clamped; three lerps per channel, each one subtraction and one fma, each a
// single fp32 rounding.  Nearest: the pixel floor(f + 0.5), clamped (wrapped) alike.  Every index is inside the frame whatever (fx, fy) is.
template <typename Tap>
__device__ __forceinline__ void view_sample(const Tap& tap, int w, int h, bool wrap, bool bilinear, float fx, float fy, float c[Tap::kN]) {
#pragma clang fp contract(off)
  const float bx = floorf(bilinear ? fx : fx + 0.5f), by = floorf(bilinear ? fy : fy + 0.5f);
  int x0, x1;
  if (wrap) {
    const int raw = static_cast<int>(fminf(fmaxf(bx, -1073741824.0f), 1073741824.0f));
    x0 = ((raw % w) + w) % w;
    x1 = x0 + 1 == w ? 0 : x0 + 1;
  } else {
    x0 = view_clamp_index(bx, w);
    x1 = view_clamp_index(bx + 1.0f, w);
  }
  const int y0 = view_clamp_index(by, h), y1 = view_clamp_index(by + 1.0f, h);
  float v00[Tap::kN];
  tap(x0, y0, v00);
  if (!bilinear) {
#pragma unroll
    for (int j = 0; j < Tap::kN; j++) c[j] = v00[j];
    return;
  }
  const float ax = fx - bx, ay = fy - by;   // (exact: a float less its own floor)
  float v10[Tap::kN], v01[Tap::kN], v11[Tap::kN];
  tap(x1, y0, v10);
  tap(x0, y1, v01);
  tap(x1, y1, v11);
#pragma unroll
  for (int j = 0; j < Tap::kN; j++) {
    const float top = fmaf(ax, v10[j] - v00[j], v00[j]);
    const float bot = fmaf(ax, v11[j] - v01[j], v01[j]);
    c[j] = fmaf(ay, bot - top, top);
  }
}

// What both filtered kernels do with a pixel once its geometry is known: the sample at the primary hit — nearest is the pixel `from` itself, the
// copy halo_view_kernel makes — and, on a dual source with `blend` and two hits, the cross-fade c = fma(t, c2 - c1, c1).  pos: view_source_pos's five.
template <bool DUAL_SRC, typename Tap>
__device__ __forceinline__ void view_filtered_value(const Tap& tap, int sw, int sh, bool wrap, int bilinear, int blend, int32_t from, int hits, const float pos[5],
                                                    float c[Tap::kN]) {
#pragma clang fp contract(off)
  if (bilinear)
    view_sample(tap, sw, sh, wrap, true, pos[0], pos[1], c);
  else
    tap.at(static_cast<uint32_t>(from), c);
  if (DUAL_SRC && blend && hits == 2) {
    float c2[Tap::kN];
    view_sample(tap, sw, sh, false, bilinear != 0, pos[2], pos[3], c2);
#pragma unroll
    for (int j = 0; j < Tap::kN; j++) c[j] = fmaf(pos[4], c2[j] - c[j], c[j]);
  }
}

}  // namespace halo

#endif
