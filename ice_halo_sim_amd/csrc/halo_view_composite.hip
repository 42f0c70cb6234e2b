// halo_view_composite.hip — the view stage for the raypath-colour images (halo_consumer_view_composite, halo_consumer_view_lanes): the class
// composite's sRGB bytes, and the class lanes themselves, seen through any lens.  What the reference's preview shader does in RGB mode
// (gui/preview_renderer.cpp:458-464, 660-678: the composited bytes as a GL_RGB8 texture, GL_LINEAR taps, sampleDualFisheye's cross-fade, no
// xyzToSrgb).  The geometry is halo_view_filtered_kernel's, statement for statement — view_direction, project_exit's primary hit, view_source_pos —
// and the sampling rule is the one of halo_view_sample.h; what differs is the image a tap is fetched from:
//   composite  a tap is the composite's byte triple as floats in BYTE units, float(b): the GL texel times 255, an exact integer, so that a
//              constant image stays that constant to the bit; the view's byte is uint8(floorf(value + 0.5f)), the framebuffer's round to nearest
//              (value lies in [0, 255]: every lerp is one rounding of a number between two bytes).  Nearest without a blend gives
//              floorf(float(b) + 0.5f) = b: the composite's own byte.
//   lanes      a tap is float(lane), the fp64 device lane narrowed as halo_lanes_drain_kernel narrows it; one thread does every class of its pixel,
//              geometry and tap positions computed once, and writes plane after plane: 16 consecutive floats per tile row.
// One thread per view pixel, 16 x 16-pixel tiles, no LDS, no atomics; projections, filter and blend are kernel arguments (scalar branches).
#include "halo_trace.inl"
#include "halo_launch.h"
#include "halo_view.h"
#include "halo_view_sample.h"

namespace halo {

namespace {

struct SrgbTap {   // the source composite, 3 bytes per pixel (halo_composite_kernel's srgb_out)
  static constexpr int kN = 3;
  const uint8_t* __restrict__ srgb;
  int w;
  __device__ __forceinline__ void at(uint32_t pixel, float v[3]) const {
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = static_cast<float>(srgb[3u * pixel + j]);
  }
  __device__ __forceinline__ void operator()(int ix, int iy, float v[3]) const { at(static_cast<uint32_t>(iy) * static_cast<uint32_t>(w) + static_cast<uint32_t>(ix), v); }
};

struct LaneTap {   // one class lane, fp64 where it lies
  static constexpr int kN = 1;
  const double* __restrict__ lane;
  int w;
  __device__ __forceinline__ void at(uint32_t pixel, float v[1]) const { v[0] = static_cast<float>(lane[pixel]); }
  __device__ __forceinline__ void operator()(int ix, int iy, float v[1]) const { at(static_cast<uint32_t>(iy) * static_cast<uint32_t>(w) + static_cast<uint32_t>(ix), v); }
};

// halo_view_filtered_kernel's geometry of view pixel (x, y): the source pixel (-1: none), view_source_pos's record and its hit count
template <int FAM>
__device__ __forceinline__ int32_t view_geometry(const ProjLds& view, const ProjLds& src, uint32_t x, uint32_t y, float pos[5], int& hits) {
#pragma clang fp contract(off)
  const int sw = src.p.img_w, sh = src.p.img_h;
  float w[3];
  const bool has_dir = view_direction(view.p, &view.half_w, static_cast<int>(x), static_cast<int>(y), w, FAM);
  int32_t from = -1;
  if (has_dir) {   // a pixel has a source iff the nearest call gives it one: project_exit's primary hit, inside the frame
    const Hits h = project_exit(src.p, w[0], w[1], w[2]);
    if (h.count > 0 && h.px0 >= 0 && h.px0 < sw && h.py0 >= 0 && h.py0 < sh) from = h.py0 * sw + h.px0;
  }
#pragma unroll
  for (int j = 0; j < 5; j++) pos[j] = 0.0f;
  hits = 0;
  if (from >= 0) hits = view_source_pos(src.p, &src.half_w, w[0], w[1], w[2], pos);
  return from;
}

}  // namespace

// FAM: the view's lens family.  DUAL_SRC: the source is a dual fisheye (the second sample and the blend are compiled for it alone).
template <int FAM, bool DUAL_SRC>
__global__ void __launch_bounds__(kBlock) halo_view_composite_kernel(const uint8_t* __restrict__ srgb_src, ProjLds view, ProjLds src, int bilinear, int blend,
                                                                      uint8_t* __restrict__ srgb_out, float* __restrict__ value_out, int32_t* __restrict__ map_out,
                                                                      float* __restrict__ tap_out, uint32_t tiles_x, uint32_t n_tiles) {
#pragma clang fp contract(off)
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  const uint32_t vw = static_cast<uint32_t>(view.p.img_w), vh = static_cast<uint32_t>(view.p.img_h);
  const int sw = src.p.img_w, sh = src.p.img_h;
  const bool wrap = !DUAL_SRC && src.p.proj_type == HALO_LENS_RECTANGULAR;
  const SrgbTap tap{srgb_src, sw};
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    if (x >= vw || y >= vh) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    float pos[5];
    int hits;
    const int32_t from = view_geometry<FAM>(view, src, x, y, pos, hits);
    if (map_out) map_out[p] = from;
    if (tap_out) {
#pragma unroll
      for (int j = 0; j < 5; j++) tap_out[5u * p + j] = pos[j];
    }
    if (srgb_src == nullptr || (value_out == nullptr && srgb_out == nullptr)) continue;   // (no composite: the geometry alone)
    float c[3] = {0.0f, 0.0f, 0.0f};   // a pixel without a source: the shader's final_color = vec3(0)
    if (from >= 0) view_filtered_value<DUAL_SRC>(tap, sw, sh, wrap, bilinear, blend, from, hits, pos, c);
    if (value_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) value_out[3u * p + j] = c[j];
    }
    if (srgb_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) srgb_out[3u * p + j] = static_cast<uint8_t>(floorf(c[j] + 0.5f));
    }
  }
}

// lanes: class c's lane at lanes[c * src_pix ..]; lanes_out: class c's plane at lanes_out[c * view pixels ..] (may be null: the geometry alone)
template <int FAM, bool DUAL_SRC>
__global__ void __launch_bounds__(kBlock) halo_view_lanes_kernel(const double* __restrict__ lanes, uint32_t class_count, ProjLds view, ProjLds src, int bilinear, int blend,
                                                                  float* __restrict__ lanes_out, int32_t* __restrict__ map_out, float* __restrict__ tap_out, uint32_t tiles_x,
                                                                  uint32_t n_tiles) {
#pragma clang fp contract(off)
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  const uint32_t vw = static_cast<uint32_t>(view.p.img_w), vh = static_cast<uint32_t>(view.p.img_h);
  const int sw = src.p.img_w, sh = src.p.img_h;
  const size_t src_pix = static_cast<size_t>(sw) * static_cast<size_t>(sh), view_pix = static_cast<size_t>(vw) * vh;
  const bool wrap = !DUAL_SRC && src.p.proj_type == HALO_LENS_RECTANGULAR;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    if (x >= vw || y >= vh) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    float pos[5];
    int hits;
    const int32_t from = view_geometry<FAM>(view, src, x, y, pos, hits);
    if (map_out) map_out[p] = from;
    if (tap_out) {
#pragma unroll
      for (int j = 0; j < 5; j++) tap_out[5u * p + j] = pos[j];
    }
    if (lanes_out == nullptr) continue;
    for (uint32_t c = 0; c < class_count; c++) {   // (a scalar loop: class_count is a kernel argument)
      float v[1] = {0.0f};
      if (from >= 0) view_filtered_value<DUAL_SRC>(LaneTap{lanes + c * src_pix, sw}, sw, sh, wrap, bilinear, blend, from, hits, pos, v);
      lanes_out[c * view_pix + p] = v[0];
    }
  }
}

namespace {

struct ViewGrid {
  ProjLds v, s;
  uint32_t tiles_x, n_tiles, grid;
  bool dual_src;
};

ViewGrid view_grid(const ProjDev& view, const ProjDev& source, int blocks) {
  ViewGrid g;
  g.v.p = view;
  g.s.p = source;
  view_proj_pre(view, &g.v.half_w);
  view_proj_pre(source, &g.s.half_w);
  g.tiles_x = (static_cast<uint32_t>(view.img_w) + kViewTile - 1u) / kViewTile;
  g.n_tiles = g.tiles_x * ((static_cast<uint32_t>(view.img_h) + kViewTile - 1u) / kViewTile);   // (at most 2^25 pixels: below 2^32 whatever the aspect)
  g.grid = g.n_tiles < static_cast<uint32_t>(blocks) ? g.n_tiles : static_cast<uint32_t>(blocks);
  g.dual_src = view_family(source.proj_type) == kViewDual;
  return g;
}

template <int FAM>
void launch_view_composite_family(const ViewGrid& g, hipStream_t stream, const uint8_t* srgb_src, int bilinear, int blend, uint8_t* srgb_out, float* value_out,
                                  int32_t* map_out, float* tap_out) {
  if (g.dual_src)
    hipLaunchKernelGGL((halo_view_composite_kernel<FAM, true>), dim3(g.grid), dim3(kBlock), 0, stream, srgb_src, g.v, g.s, bilinear, blend, srgb_out, value_out, map_out, tap_out,
                       g.tiles_x, g.n_tiles);
  else
    hipLaunchKernelGGL((halo_view_composite_kernel<FAM, false>), dim3(g.grid), dim3(kBlock), 0, stream, srgb_src, g.v, g.s, bilinear, blend, srgb_out, value_out, map_out, tap_out,
                       g.tiles_x, g.n_tiles);
}

template <int FAM>
void launch_view_lanes_family(const ViewGrid& g, hipStream_t stream, const double* lanes, uint32_t class_count, int bilinear, int blend, float* lanes_out, int32_t* map_out,
                              float* tap_out) {
  if (g.dual_src)
    hipLaunchKernelGGL((halo_view_lanes_kernel<FAM, true>), dim3(g.grid), dim3(kBlock), 0, stream, lanes, class_count, g.v, g.s, bilinear, blend, lanes_out, map_out, tap_out,
                       g.tiles_x, g.n_tiles);
  else
    hipLaunchKernelGGL((halo_view_lanes_kernel<FAM, false>), dim3(g.grid), dim3(kBlock), 0, stream, lanes, class_count, g.v, g.s, bilinear, blend, lanes_out, map_out, tap_out,
                       g.tiles_x, g.n_tiles);
}

}  // namespace

hipError_t launch_view_composite(const uint8_t* srgb_src, const ProjDev& view, const ProjDev& source, bool bilinear, bool blend, uint8_t* srgb_out, float* value_out,
                                 int32_t* map_out, float* tap_out, int blocks, hipStream_t stream) {
  const ViewGrid g = view_grid(view, source, blocks);
  const int bi = bilinear ? 1 : 0, bl = blend ? 1 : 0;
  switch (view_family(view.proj_type)) {
    case kViewSingle: launch_view_composite_family<kViewSingle>(g, stream, srgb_src, bi, bl, srgb_out, value_out, map_out, tap_out); break;
    case kViewDual: launch_view_composite_family<kViewDual>(g, stream, srgb_src, bi, bl, srgb_out, value_out, map_out, tap_out); break;
    case kViewRect: launch_view_composite_family<kViewRect>(g, stream, srgb_src, bi, bl, srgb_out, value_out, map_out, tap_out); break;
    default: launch_view_composite_family<kViewGlobe>(g, stream, srgb_src, bi, bl, srgb_out, value_out, map_out, tap_out); break;
  }
  return hipGetLastError();
}

hipError_t launch_view_lanes(const double* lanes, uint32_t class_count, const ProjDev& view, const ProjDev& source, bool bilinear, bool blend, float* lanes_out,
                             int32_t* map_out, float* tap_out, int blocks, hipStream_t stream) {
  const ViewGrid g = view_grid(view, source, blocks);
  const int bi = bilinear ? 1 : 0, bl = blend ? 1 : 0;
  switch (view_family(view.proj_type)) {
    case kViewSingle: launch_view_lanes_family<kViewSingle>(g, stream, lanes, class_count, bi, bl, lanes_out, map_out, tap_out); break;
    case kViewDual: launch_view_lanes_family<kViewDual>(g, stream, lanes, class_count, bi, bl, lanes_out, map_out, tap_out); break;
    case kViewRect: launch_view_lanes_family<kViewRect>(g, stream, lanes, class_count, bi, bl, lanes_out, map_out, tap_out); break;
    default: launch_view_lanes_family<kViewGlobe>(g, stream, lanes, class_count, bi, bl, lanes_out, map_out, tap_out); break;
  }
  return hipGetLastError();
}

}  // namespace halo
