// halo_view.hip — the view stage of the device consumer (halo_consumer_view): the consumer's image, accumulated under one render (the source),
// seen through any other lens, view direction or field of view (the view), by a gather where the image lies.  Per view pixel:
//   1. the view lens's inverse gives the world direction of the pixel's centre (halo_view.h view_direction);
//   2. project_exit — the function the trace kernels land their exits with — gives the source pixel that direction falls on (its PRIMARY hit;
//      a dual source's overlap write is not read);
//   3. the source pixel's raw value sum + comp is copied (nearest neighbour, no arithmetic) and
//   4. put through the snapshot's display transform (halo_display.h display_pixel).
// A gather with no Jacobian, like the reference's preview shader: from an equal-area source the view shows radiance, from any other the source
// pixels' energy as it lies.  One thread per view pixel, 16 x 16-pixel tiles per workgroup so that a workgroup's gathers stay close in the
// source; no LDS, no atomics.  Both projections are kernel arguments: every lens branch is a scalar branch, and the view's lens family is a
// template argument.
#include "halo_trace.inl"
#include "halo_display.h"
#include "halo_launch.h"
#include "halo_view.h"
#include "halo_view_sample.h"

namespace halo {

template <int FAM>
__global__ void __launch_bounds__(kBlock) halo_view_kernel(const float* __restrict__ sum, const float* __restrict__ comp, ProjLds view, ProjLds src, DisplayDev dsp,
                                                            uint8_t* __restrict__ rgb_out, float* __restrict__ xyz_out, int32_t* __restrict__ map_out,
                                                            float* __restrict__ dir_out, uint32_t tiles_x, uint32_t n_tiles) {
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  const uint32_t vw = static_cast<uint32_t>(view.p.img_w), vh = static_cast<uint32_t>(view.p.img_h);
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    if (x >= vw || y >= vh) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    float w[3];
    const bool has_dir = view_direction(view.p, &view.half_w, static_cast<int>(x), static_cast<int>(y), w, FAM);
    int32_t from = -1;
    if (has_dir) {
      const Hits h = project_exit(src.p, w[0], w[1], w[2]);
      if (h.count > 0 && h.px0 >= 0 && h.px0 < src.p.img_w && h.py0 >= 0 && h.py0 < src.p.img_h) from = h.py0 * src.p.img_w + h.px0;
    }
    if (dir_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) dir_out[3u * p + j] = w[j];
    }
    if (map_out) map_out[p] = from;
    if (xyz_out == nullptr && rgb_out == nullptr) continue;
    float raw[3] = {0.0f, 0.0f, 0.0f};
    if (from >= 0) {
#pragma unroll
      for (int j = 0; j < 3; j++) raw[j] = __fadd_rn(sum[3u * static_cast<uint32_t>(from) + j], comp[3u * static_cast<uint32_t>(from) + j]);
    }
    if (xyz_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) xyz_out[3u * p + j] = raw[j];
    }
    if (rgb_out == nullptr) continue;
    uint8_t px[3];
    display_pixel(raw, dsp, px);
#pragma unroll
    for (int j = 0; j < 3; j++) rgb_out[3u * p + j] = px[j];
  }
}

// ---- the filtered view (halo_consumer_view_filtered): bilinear taps and the overlap-band blend ----------------------------------------------
// What the reference's preview shader does with its GL_LINEAR, clamp-to-edge XYZ texture (gui/preview_renderer.cpp:554-557) and its
// sampleDualFisheye (:152-180).  A kernel of its own beside halo_view_kernel, whose instantiations keep their code.
namespace {

// one tap of halo_view_sample.h's view_sample: the snapshot's xyz_out of source pixel (ix, iy), both inside the frame
struct XyzTap {
  static constexpr int kN = 3;
  const float* __restrict__ sum;
  const float* __restrict__ comp;
  int w;
  __device__ __forceinline__ void at(uint32_t pixel, float v[3]) const {
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = __fadd_rn(sum[3u * pixel + j], comp[3u * pixel + j]);
  }
  __device__ __forceinline__ void operator()(int ix, int iy, float v[3]) const { at(static_cast<uint32_t>(iy) * static_cast<uint32_t>(w) + static_cast<uint32_t>(ix), v); }
};

}  // namespace

// FAM: the view's lens family.  DUAL_SRC: the source is a dual fisheye — the only source with a second hit: the second sample and the blend are
// compiled for it alone.  `bilinear` and `blend` are kernel arguments, like the projections: scalar branches.
template <int FAM, bool DUAL_SRC>
__global__ void __launch_bounds__(kBlock) halo_view_filtered_kernel(const float* __restrict__ sum, const float* __restrict__ comp, ProjLds view, ProjLds src, DisplayDev dsp,
                                                                     int bilinear, int blend, uint8_t* __restrict__ rgb_out, float* __restrict__ xyz_out,
                                                                     int32_t* __restrict__ map_out, float* __restrict__ dir_out, float* __restrict__ tap_out, uint32_t tiles_x,
                                                                     uint32_t n_tiles) {
#pragma clang fp contract(off)
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  const uint32_t vw = static_cast<uint32_t>(view.p.img_w), vh = static_cast<uint32_t>(view.p.img_h);
  const int sw = src.p.img_w, sh = src.p.img_h;
  const bool wrap = !DUAL_SRC && src.p.proj_type == HALO_LENS_RECTANGULAR;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    if (x >= vw || y >= vh) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    float w[3];
    const bool has_dir = view_direction(view.p, &view.half_w, static_cast<int>(x), static_cast<int>(y), w, FAM);
    int32_t from = -1;
    if (has_dir) {   // a pixel has a source iff the nearest call gives it one: project_exit's primary hit, inside the frame
      const Hits h = project_exit(src.p, w[0], w[1], w[2]);
      if (h.count > 0 && h.px0 >= 0 && h.px0 < sw && h.py0 >= 0 && h.py0 < sh) from = h.py0 * sw + h.px0;
    }
    float pos[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int hits = 0;
    if (from >= 0) hits = view_source_pos(src.p, &src.half_w, w[0], w[1], w[2], pos);
    if (dir_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) dir_out[3u * p + j] = w[j];
    }
    if (map_out) map_out[p] = from;
    if (tap_out) {
#pragma unroll
      for (int j = 0; j < 5; j++) tap_out[5u * p + j] = pos[j];
    }
    if (xyz_out == nullptr && rgb_out == nullptr) continue;
    float raw[3] = {0.0f, 0.0f, 0.0f};
    if (from >= 0) {
      if (bilinear) {
        view_sample(XyzTap{sum, comp, sw}, sw, sh, wrap, true, pos[0], pos[1], raw);
      } else {   // the copy halo_view_kernel makes
#pragma unroll
        for (int j = 0; j < 3; j++) raw[j] = __fadd_rn(sum[3u * static_cast<uint32_t>(from) + j], comp[3u * static_cast<uint32_t>(from) + j]);
      }
      if (DUAL_SRC && blend && hits == 2) {
        float c2[3];
        view_sample(XyzTap{sum, comp, sw}, sw, sh, false, bilinear != 0, pos[2], pos[3], c2);
#pragma unroll
        for (int j = 0; j < 3; j++) raw[j] = fmaf(pos[4], c2[j] - raw[j], raw[j]);
      }
    }
    if (xyz_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) xyz_out[3u * p + j] = raw[j];
    }
    if (rgb_out == nullptr) continue;
    uint8_t px[3];
    display_pixel(raw, dsp, px);
#pragma unroll
    for (int j = 0; j < 3; j++) rgb_out[3u * p + j] = px[j];
  }
}

template <int FAM>
static void launch_view_filtered_family(bool dual_src, uint32_t grid, hipStream_t stream, const float* sum, const float* comp, const ProjLds& v, const ProjLds& s,
                                        const DisplayDev& d, int bilinear, int blend, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, float* tap_out,
                                        uint32_t tiles_x, uint32_t n_tiles) {
  if (dual_src)
    hipLaunchKernelGGL((halo_view_filtered_kernel<FAM, true>), dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, bilinear, blend, rgb_out, xyz_out, map_out, dir_out,
                       tap_out, tiles_x, n_tiles);
  else
    hipLaunchKernelGGL((halo_view_filtered_kernel<FAM, false>), dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, bilinear, blend, rgb_out, xyz_out, map_out, dir_out,
                       tap_out, tiles_x, n_tiles);
}

hipError_t launch_view_filtered(const float* sum, const float* comp, const ProjDev& view, const ProjDev& source, float scale, const float ray_color[3],
                                const float background[3], bool bilinear, bool blend, uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, float* tap_out,
                                int blocks, hipStream_t stream) {
  ProjLds v, s;
  v.p = view;
  s.p = source;
  view_proj_pre(view, &v.half_w);
  view_proj_pre(source, &s.half_w);
  DisplayDev d;
  d.scale = scale;
  for (int j = 0; j < 3; j++) {
    d.ray_color[j] = ray_color[j];
    d.background[j] = background[j];
  }
  const uint32_t tiles_x = (static_cast<uint32_t>(view.img_w) + kViewTile - 1u) / kViewTile, tiles_y = (static_cast<uint32_t>(view.img_h) + kViewTile - 1u) / kViewTile;
  const uint32_t n_tiles = tiles_x * tiles_y;
  const uint32_t grid = n_tiles < static_cast<uint32_t>(blocks) ? n_tiles : static_cast<uint32_t>(blocks);
  const bool dual_src = view_family(source.proj_type) == kViewDual;
  const int bi = bilinear ? 1 : 0, bl = blend ? 1 : 0;
  switch (view_family(view.proj_type)) {
    case kViewSingle: launch_view_filtered_family<kViewSingle>(dual_src, grid, stream, sum, comp, v, s, d, bi, bl, rgb_out, xyz_out, map_out, dir_out, tap_out, tiles_x, n_tiles); break;
    case kViewDual: launch_view_filtered_family<kViewDual>(dual_src, grid, stream, sum, comp, v, s, d, bi, bl, rgb_out, xyz_out, map_out, dir_out, tap_out, tiles_x, n_tiles); break;
    case kViewRect: launch_view_filtered_family<kViewRect>(dual_src, grid, stream, sum, comp, v, s, d, bi, bl, rgb_out, xyz_out, map_out, dir_out, tap_out, tiles_x, n_tiles); break;
    default: launch_view_filtered_family<kViewGlobe>(dual_src, grid, stream, sum, comp, v, s, d, bi, bl, rgb_out, xyz_out, map_out, dir_out, tap_out, tiles_x, n_tiles); break;
  }
  return hipGetLastError();
}

hipError_t launch_view(const float* sum, const float* comp, const ProjDev& view, const ProjDev& source, float scale, const float ray_color[3], const float background[3],
                       uint8_t* rgb_out, float* xyz_out, int32_t* map_out, float* dir_out, int blocks, hipStream_t stream) {
  ProjLds v, s;
  v.p = view;
  s.p = source;
  view_proj_pre(view, &v.half_w);
  view_proj_pre(source, &s.half_w);
  DisplayDev d;
  d.scale = scale;
  for (int j = 0; j < 3; j++) {
    d.ray_color[j] = ray_color[j];
    d.background[j] = background[j];
  }
  const uint32_t tiles_x = (static_cast<uint32_t>(view.img_w) + kViewTile - 1u) / kViewTile, tiles_y = (static_cast<uint32_t>(view.img_h) + kViewTile - 1u) / kViewTile;
  const uint32_t n_tiles = tiles_x * tiles_y;   // (at most 2^25 pixels: below 2^32 whatever the aspect — a 1 x 2^25 view has 2^21 tiles)
  const uint32_t grid = n_tiles < static_cast<uint32_t>(blocks) ? n_tiles : static_cast<uint32_t>(blocks);
  switch (view_family(view.proj_type)) {
    case kViewSingle: hipLaunchKernelGGL(halo_view_kernel<kViewSingle>, dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, rgb_out, xyz_out, map_out, dir_out, tiles_x, n_tiles); break;
    case kViewDual: hipLaunchKernelGGL(halo_view_kernel<kViewDual>, dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, rgb_out, xyz_out, map_out, dir_out, tiles_x, n_tiles); break;
    case kViewRect: hipLaunchKernelGGL(halo_view_kernel<kViewRect>, dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, rgb_out, xyz_out, map_out, dir_out, tiles_x, n_tiles); break;
    default: hipLaunchKernelGGL(halo_view_kernel<kViewGlobe>, dim3(grid), dim3(kBlock), 0, stream, sum, comp, v, s, d, rgb_out, xyz_out, map_out, dir_out, tiles_x, n_tiles); break;
  }
  return hipGetLastError();
}

}  // namespace halo
