// halo_view_overlay.hip — the auxiliary lines of the view stage (halo_consumer_view_overlay, halo_consumer_view_composite_overlay): one pass behind
// the gather, on its stream, over the gather's own device buffers.  Per view pixel it reads the direction the gather wrote (`dir`, 12 bytes) and the
// pixel's bytes (`rgb`, 3 bytes), computes the sky coordinates and the pixel footprints, draws the layers by the rule of halo_overlay.h and writes the
// bytes back in place (3 bytes); sky_out (6 floats) and value_out (3 floats) are optional.
// The siblings' geometry: one thread per view pixel, 16 x 16-pixel tiles, the grid strides over the tiles, no LDS, no atomics; the overlay record is a
// kernel argument and every switch test a scalar branch.  A wave holds four rows of sixteen pixels and the tile origins are even, so the 2 x 2 quad
// partners of a pixel — (x ^ 1, y) and (x, y ^ 1) — are the lanes lane ^ 1 and lane ^ 16: the sky coordinates are computed once per pixel and the
// partners' come by __shfl_xor.  EVERY lane of a wave takes part in the exchange, those outside the view included (they hold "no direction"): nothing
// leaves the tile loop before it.  The fallback neighbour — the other side of the pixel, taken where the partner lies outside the view or has no
// direction — may lie in another wave or another tile: it is recomputed from the `dir` buffer, by the few lanes that need it.
// halo_view_dir_kernel writes the view's directions alone, for the composite call, whose gather has no dir output.
#include "halo_trace.inl"
#include "halo_launch.h"
#include "halo_overlay.h"
#include "halo_view.h"
#include "halo_view_sample.h"

namespace halo {

namespace {

// the sky coordinates of view pixel (x, y), inside the view, from the dir buffer: false where the pixel has no direction
__device__ __forceinline__ bool overlay_sky_at(const float* __restrict__ dir, uint32_t vw, uint32_t x, uint32_t y, const float sun[3], float sky[3]) {
  const size_t p = static_cast<size_t>(y) * vw + x;
  const float w[3] = {dir[3u * p], dir[3u * p + 1u], dir[3u * p + 2u]};
  sky[0] = sky[1] = sky[2] = 0.0f;
  if (!overlay_has_dir(w)) return false;
  overlay_sky(w, sun, sky);
  return true;
}

}  // namespace

__global__ void __launch_bounds__(kBlock) halo_view_overlay_kernel(const float* __restrict__ dir, OverlayDev ov, uint32_t vw, uint32_t vh, uint8_t* __restrict__ rgb,
                                                                    float* __restrict__ value_out, float* __restrict__ sky_out, uint32_t tiles_x, uint32_t n_tiles) {
#pragma clang fp contract(off)
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    const bool inside = x < vw && y < vh;
    float sky[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const bool has = inside && overlay_sky_at(dir, vw, x, y, ov.o.sun_dir, sky);
    // the quad exchange: every lane of the wave, whatever it holds
    float qx[3], qy[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      qx[j] = __shfl_xor(sky[j], 1);
      qy[j] = __shfl_xor(sky[j], 16);
    }
    const bool has_x = __shfl_xor(has ? 1 : 0, 1) != 0, has_y = __shfl_xor(has ? 1 : 0, 16) != 0;
    if (!inside) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    if (has) {
      bool ok_x = has_x, ok_y = has_y;
      if (!ok_x) {   // the other neighbour in the row: x - 1 for even x, x + 1 for odd x (unsigned: x - 1 of 0 wraps past vw)
        const uint32_t xo = (x & 1u) ? x + 1u : x - 1u;
        ok_x = xo < vw && overlay_sky_at(dir, vw, xo, y, ov.o.sun_dir, qx);
      }
      if (!ok_y) {
        const uint32_t yo = (y & 1u) ? y + 1u : y - 1u;
        ok_y = yo < vh && overlay_sky_at(dir, vw, x, yo, ov.o.sun_dir, qy);
      }
      float fx[3] = {0.0f, 0.0f, 0.0f}, fy[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < 3; j++) {
        if (ok_x) fx[j] = overlay_fw_term(qx[j], sky[j], j == 1);
        if (ok_y) fy[j] = overlay_fw_term(qy[j], sky[j], j == 1);
      }
      overlay_footprint(fx, fy, sky + 3);
    }
    if (sky_out) {
#pragma unroll
      for (int j = 0; j < 6; j++) sky_out[6u * p + j] = sky[j];
    }
    if (rgb == nullptr) continue;   // (the sky coordinates alone)
    const float base[3] = {static_cast<float>(rgb[3u * p]), static_cast<float>(rgb[3u * p + 1u]), static_cast<float>(rgb[3u * p + 2u])};
    float v[3] = {base[0], base[1], base[2]};
    if (has) overlay_pixel(base, sky, static_cast<float>(x), static_cast<float>(y), ov.marks, ov.o, v);
    if (value_out) {
#pragma unroll
      for (int j = 0; j < 3; j++) value_out[3u * p + j] = v[j];
    }
    if (has) {   // (a pixel without a direction keeps its bytes)
#pragma unroll
      for (int j = 0; j < 3; j++) rgb[3u * p + j] = overlay_byte(v[j]);
    }
  }
}

// dir_out of halo_view_kernel, alone: view_direction of every pixel of the view
template <int FAM>
__global__ void __launch_bounds__(kBlock) halo_view_dir_kernel(ProjLds view, float* __restrict__ dir_out, uint32_t tiles_x, uint32_t n_tiles) {
  const uint32_t tx = threadIdx.x & (kViewTile - 1u), ty = threadIdx.x / kViewTile;
  const uint32_t vw = static_cast<uint32_t>(view.p.img_w), vh = static_cast<uint32_t>(view.p.img_h);
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {   // (workgroup-uniform)
    const uint32_t x = (tile % tiles_x) * kViewTile + tx, y = (tile / tiles_x) * kViewTile + ty;
    if (x >= vw || y >= vh) continue;
    const size_t p = static_cast<size_t>(y) * vw + x;
    float w[3];
    view_direction(view.p, &view.half_w, static_cast<int>(x), static_cast<int>(y), w, FAM);
#pragma unroll
    for (int j = 0; j < 3; j++) dir_out[3u * p + j] = w[j];
  }
}

namespace {

struct TileGrid {
  uint32_t tiles_x, n_tiles, grid;
};
TileGrid tile_grid(int vw, int vh, int blocks) {
  TileGrid g;
  g.tiles_x = (static_cast<uint32_t>(vw) + kViewTile - 1u) / kViewTile;
  g.n_tiles = g.tiles_x * ((static_cast<uint32_t>(vh) + kViewTile - 1u) / kViewTile);   // (at most 2^25 pixels: below 2^32 whatever the aspect)
  g.grid = g.n_tiles < static_cast<uint32_t>(blocks) ? g.n_tiles : static_cast<uint32_t>(blocks);
  return g;
}

}  // namespace

hipError_t launch_view_overlay(const float* dir, const HaloViewOverlay& overlay, const float marks[9], int view_w, int view_h, uint8_t* rgb, float* value_out, float* sky_out,
                               int blocks, hipStream_t stream) {
  OverlayDev ov;
  ov.o = overlay;
  for (int j = 0; j < 9; j++) ov.marks[j] = marks[j];
  const TileGrid g = tile_grid(view_w, view_h, blocks);
  hipLaunchKernelGGL(halo_view_overlay_kernel, dim3(g.grid), dim3(kBlock), 0, stream, dir, ov, static_cast<uint32_t>(view_w), static_cast<uint32_t>(view_h), rgb, value_out,
                     sky_out, g.tiles_x, g.n_tiles);
  return hipGetLastError();
}

hipError_t launch_view_dir(const ProjDev& view, float* dir_out, int blocks, hipStream_t stream) {
  ProjLds v;
  v.p = view;
  view_proj_pre(view, &v.half_w);
  const TileGrid g = tile_grid(view.img_w, view.img_h, blocks);
  switch (view_family(view.proj_type)) {
    case kViewSingle: hipLaunchKernelGGL(halo_view_dir_kernel<kViewSingle>, dim3(g.grid), dim3(kBlock), 0, stream, v, dir_out, g.tiles_x, g.n_tiles); break;
    case kViewDual: hipLaunchKernelGGL(halo_view_dir_kernel<kViewDual>, dim3(g.grid), dim3(kBlock), 0, stream, v, dir_out, g.tiles_x, g.n_tiles); break;
    case kViewRect: hipLaunchKernelGGL(halo_view_dir_kernel<kViewRect>, dim3(g.grid), dim3(kBlock), 0, stream, v, dir_out, g.tiles_x, g.n_tiles); break;
    default: hipLaunchKernelGGL(halo_view_dir_kernel<kViewGlobe>, dim3(g.grid), dim3(kBlock), 0, stream, v, dir_out, g.tiles_x, g.n_tiles); break;
  }
  return hipGetLastError();
}

}  // namespace halo
