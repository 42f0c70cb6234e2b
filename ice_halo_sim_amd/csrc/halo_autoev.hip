// halo_autoev.hip — the auto-exposure stage of the device consumer: the reference GUI's Adaptive Brightness anchor (gui/gui_ev_auto.hpp
// DownsampleBoxSumY + ComputeP99Y) on the consumer image where it lies.  Two steps, both on the caller's stream with no host wait between them:
//   1. a value kernel writes the candidate values — the box sums of Y over f x f pixels (coarse path) or Y itself (fine path);
//   2. an exact radix select over the float bit patterns of the positive values (positive floats order like their patterns), 11 + 11 + 10
//      bits: one workgroup doing its three passes back to back out of an LDS histogram for up to kAevSmallMax values, multi-block histogram
//      kernels with a one-workgroup "pick the bin" kernel between them above that.  The picked prefix and the rank wanted inside it travel
//      from kernel to kernel in device memory (AevRecord); the host reads the record once, at the end.
// Every count is an integer, so the record does not depend on the order of the atomic adds: the stage is bit-reproducible.
#include "halo_launch.h"
#include "halo_radix.h"

namespace halo {

namespace {

constexpr uint32_t kAevPeel = 4u;          // rounds of wave-level aggregation before the plain LDS add (the digits themselves: halo_radix.h)

// One wave's adds of 1 to h[bin].  A halo image piles into a handful of exponents, so on the first digit most lanes of a wave name the same
// bin.  The plain form (AGG = false, the product) leaves that to the LDS: measured on images whose first digit lands in a dozen bins, ds_add_u32
// takes it well and any bookkeeping in front of it costs more than it saves (4-25 us per call); only an image of ONE value — every lane of every
// wave in one bin on all three digits — is faster aggregated (profiles/auto_ev_cost.txt).  AGG (option auto_ev_hist = 1, kept for that
// A/B): the wave peels off up to kAevPeel bins — the bin of its first pending lane, a ballot of the lanes that share it, one add of their number
// by that lane — and whatever is left adds for itself.  `valid` may differ per lane; every lane of the wave calls.
template <bool AGG>
__device__ __forceinline__ void aev_wave_add(uint32_t* h, uint32_t bin, bool valid) {
  if constexpr (AGG) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll 1
    for (uint32_t r = 0; r < kAevPeel; r++) {
      const unsigned long long todo = __ballot(valid);
      if (todo == 0ull) return;
      const uint32_t lead = static_cast<uint32_t>(__ffsll(todo)) - 1u;
      const uint32_t b = static_cast<uint32_t>(__shfl(static_cast<int>(bin), static_cast<int>(lead)));
      const bool mine = valid && bin == b;
      const unsigned long long same = __ballot(mine);
      if (lane == lead) atomicAdd(&h[b], static_cast<uint32_t>(__popcll(same)));
      if (mine) valid = false;
    }
  }
  if (valid) atomicAdd(&h[bin], 1u);
}

// Histogram of digit `pass` of the positive values among vals[first], vals[first + stride], ... whose higher digits equal `prefix`.
template <bool AGG>
__device__ __forceinline__ void aev_hist_pass(const float* __restrict__ vals, uint32_t n, uint32_t first, uint32_t stride, uint32_t pass, uint32_t prefix,
                                              uint32_t* h) {
  const uint32_t shift = aev_shift(pass), mask = (1u << aev_width(pass)) - 1u, hi = shift + aev_width(pass);
  // whole waves stay in the loop together (the aggregation's ballots need every lane of the wave): the bound is rounded up per wave
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t base = first - lane; base < n; base += stride) {
    const uint32_t i = base + lane;
    bool valid = i < n;
    uint32_t u = 0u;
    if (valid) {
      const float v = vals[i];
      u = __float_as_uint(v);
      valid = v > 0.0f && (hi >= 32u || (u >> hi) == prefix);
    }
    aev_wave_add<AGG>(h, (u >> shift) & mask, valid);
  }
}

// The bin of the `rank`-th smallest counted value (0-based) in h[0 .. nb), by the whole workgroup (kAevBlock threads, every one calls):
// thread t owns bins 2t and 2t + 1, an inclusive scan inside each wave, the waves' totals through LDS.  first: the histogram is the first
// digit's — its total is the count of positive values, and the rank wanted is the reference's index rule, idx = (size_t)((float)count * 0.99f)
// clamped to count - 1, with the product rounded once in fp32 (__fmul_rn: bit-identical to the host's).  Returns false when nothing was
// counted.  The picked bin and the rank inside it come back in sel[0], sel[1]; the total in *total.
__device__ __forceinline__ bool aev_pick(const uint32_t* h, uint32_t nb, bool first, uint32_t rank, uint32_t* wave_tot, uint32_t* sel, uint32_t* total,
                                         uint32_t* idx_out) {
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint32_t a0 = 2u * t < nb ? h[2u * t] : 0u, a1 = 2u * t + 1u < nb ? h[2u * t + 1u] : 0u, s = a0 + a1;
  uint32_t inc = s;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t v = static_cast<uint32_t>(__shfl_up(static_cast<int>(inc), d));
    if (lane >= d) inc += v;
  }
  if (lane == 63u) wave_tot[w] = inc;
  __syncthreads();
  uint32_t before = 0u, all = 0u;
  for (uint32_t k = 0; k < kAevBlock / 64; k++) {
    const uint32_t x = wave_tot[k];
    if (k < w) before += x;
    all += x;
  }
  *total = all;
  if (all == 0u) return false;
  if (first) {
    uint32_t idx = static_cast<uint32_t>(__fmul_rn(__uint2float_rn(all), 0.99f));
    if (idx >= all) idx = all - 1u;
    rank = idx;
    *idx_out = idx;
  }
  const uint32_t excl = before + inc - s;
  if (rank >= excl && rank < excl + a0) {
    sel[0] = 2u * t;
    sel[1] = rank - excl;
  } else if (rank >= excl + a0 && rank < excl + s) {
    sel[0] = 2u * t + 1u;
    sel[1] = rank - excl - a0;
  }
  __syncthreads();
  return true;
}

}  // namespace

// DownsampleBoxSumY (gui_ev_auto.hpp:31-57) over Y = sum + comp (what halo_post_snapshot_kernel hands out): one thread per coarse bin, the
// f x f pixels added one after another, rows outside, columns inside, from 0.0f — each add rounded on its own, in the reference's order.
// Bins cover [0, wc * f) x [0, hc * f): trailing rows and columns that do not fill a bin are never read.
__global__ void __launch_bounds__(256) halo_aev_coarse_kernel(const float* __restrict__ sum, const float* __restrict__ comp, uint32_t width, uint32_t f,
                                                              uint32_t wc, uint32_t n_bins, float* __restrict__ vals) {
  const uint32_t bin = blockIdx.x * 256u + threadIdx.x;
  if (bin >= n_bins) return;
  const uint32_t rc = bin / wc, cc = bin - rc * wc;
  float acc = 0.0f;
  for (uint32_t dr = 0; dr < f; dr++) {
    const size_t row = (static_cast<size_t>(rc) * f + dr) * width + static_cast<size_t>(cc) * f;
    for (uint32_t dc = 0; dc < f; dc++) {
      const size_t i = 3u * (row + dc) + 1u;
      acc = __fadd_rn(acc, __fadd_rn(sum[i], comp[i]));
    }
  }
  vals[bin] = acc;
}

// The fine path's values: Y of every pixel.
__global__ void __launch_bounds__(256) halo_aev_fine_kernel(const float* __restrict__ sum, const float* __restrict__ comp, uint32_t n_pix, float* __restrict__ vals) {
  const uint32_t stride = gridDim.x * 256u;
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n_pix; p += stride) {
    const size_t i = 3u * static_cast<size_t>(p) + 1u;
    vals[p] = __fadd_rn(sum[i], comp[i]);
  }
}

// The whole select by one workgroup: three histogram passes over vals[0 .. n) and the pick after each, out of one LDS histogram.
template <bool AGG>
__global__ void __launch_bounds__(kAevBlock) halo_aev_select_small_kernel(const float* __restrict__ vals, uint32_t n, AevRecord* __restrict__ rec) {
  __shared__ uint32_t h[kAevBins];
  __shared__ uint32_t wave_tot[kAevBlock / 64];
  __shared__ uint32_t sel[2];
  uint32_t prefix = 0u, rank = 0u, count = 0u, idx = 0u;
  for (uint32_t pass = 0; pass < 3u; pass++) {
    for (uint32_t i = threadIdx.x; i < kAevBins; i += kAevBlock) h[i] = 0u;
    __syncthreads();
    aev_hist_pass<AGG>(vals, n, threadIdx.x, kAevBlock, pass, prefix, h);
    __syncthreads();
    uint32_t total = 0u;
    const bool any = aev_pick(h, 1u << aev_width(pass), pass == 0u, rank, wave_tot, sel, &total, &idx);
    if (pass == 0u) count = total;
    if (!any) break;   // (workgroup-uniform: nothing positive, or — impossible with values that do not change — nothing under the prefix)
    prefix = (prefix << aev_width(pass)) | sel[0];
    rank = sel[1];
    __syncthreads();   // sel and wave_tot are rewritten by the next pass
  }
  if (threadIdx.x == 0u) {
    rec->count = count;
    rec->idx = idx;
    rec->p99_bits = count ? prefix : 0u;
    rec->prefix = prefix;
    rec->rank = rank;
  }
}

// Large value sets: one histogram pass by many workgroups into hist[pass] (zeroed by the launcher), reading the prefix the previous pick left.
template <bool AGG>
__global__ void __launch_bounds__(kAevBlock) halo_aev_hist_kernel(const float* __restrict__ vals, uint32_t n, uint32_t pass, const AevRecord* __restrict__ rec,
                                                                  uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kAevBins];
  if (pass > 0u && rec->count == 0u) return;   // nothing positive: the first pick said so
  const uint32_t prefix = pass ? rec->prefix : 0u;
  for (uint32_t i = threadIdx.x; i < kAevBins; i += kAevBlock) h[i] = 0u;
  __syncthreads();
  aev_hist_pass<AGG>(vals, n, blockIdx.x * kAevBlock + threadIdx.x, gridDim.x * kAevBlock, pass, prefix, h);
  __syncthreads();
  uint32_t* out = hist + pass * kAevBins;
  for (uint32_t i = threadIdx.x; i < (1u << aev_width(pass)); i += kAevBlock)
    if (h[i]) atomicAdd(&out[i], h[i]);
}

// ... and the one workgroup between two of them: picks the bin of hist[pass], extends the prefix, leaves the rank inside the bin.
__global__ void __launch_bounds__(kAevBlock) halo_aev_pick_kernel(uint32_t pass, AevRecord* __restrict__ rec, const uint32_t* __restrict__ hist) {
  __shared__ uint32_t wave_tot[kAevBlock / 64];
  __shared__ uint32_t sel[2];
  if (pass > 0u && rec->count == 0u) return;
  const uint32_t prefix = pass ? rec->prefix : 0u, rank = pass ? rec->rank : 0u;
  uint32_t total = 0u, idx = 0u;
  const bool any = aev_pick(hist + pass * kAevBins, 1u << aev_width(pass), pass == 0u, rank, wave_tot, sel, &total, &idx);
  if (threadIdx.x != 0u) return;
  if (pass == 0u) {
    rec->count = total;
    rec->idx = idx;
    rec->p99_bits = 0u;
  }
  if (!any) return;
  const uint32_t np = (prefix << aev_width(pass)) | sel[0];
  rec->prefix = np;
  rec->rank = sel[1];
  if (pass == 2u) rec->p99_bits = np;
}

hipError_t launch_aev_values(const float* sum, const float* comp, uint32_t width, uint32_t height, uint32_t f, uint32_t wc, uint32_t hc, float* vals, int blocks,
                             hipStream_t stream) {
  if (wc > 0u && hc > 0u) {
    const uint32_t n_bins = wc * hc;
    hipLaunchKernelGGL(halo_aev_coarse_kernel, dim3((n_bins + 255u) / 256u), dim3(256), 0, stream, sum, comp, width, f, wc, n_bins, vals);
  } else {
    const uint32_t n_pix = width * height;
    const uint32_t need = (n_pix + 255u) / 256u;
    hipLaunchKernelGGL(halo_aev_fine_kernel, dim3(need < static_cast<uint32_t>(blocks) ? need : static_cast<uint32_t>(blocks)), dim3(256), 0, stream, sum, comp,
                       n_pix, vals);
  }
  return hipGetLastError();
}

hipError_t launch_aev_select(const float* vals, uint32_t n, AevRecord* rec, uint32_t* hist, bool one_workgroup, bool aggregate, int blocks, hipStream_t stream) {
  if (one_workgroup) {
    if (aggregate) hipLaunchKernelGGL(halo_aev_select_small_kernel<true>, dim3(1), dim3(kAevBlock), 0, stream, vals, n, rec);
    else hipLaunchKernelGGL(halo_aev_select_small_kernel<false>, dim3(1), dim3(kAevBlock), 0, stream, vals, n, rec);
    return hipGetLastError();
  }
  hipError_t e = hipMemsetAsync(hist, 0, 3u * kAevBins * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const uint32_t need = (n + 4u * kAevBlock - 1u) / (4u * kAevBlock);   // at least four values per thread
  const uint32_t grid = need < static_cast<uint32_t>(blocks) ? (need ? need : 1u) : static_cast<uint32_t>(blocks);
  for (uint32_t pass = 0; pass < 3u; pass++) {
    if (aggregate) hipLaunchKernelGGL(halo_aev_hist_kernel<true>, dim3(grid), dim3(kAevBlock), 0, stream, vals, n, pass, rec, hist);
    else hipLaunchKernelGGL(halo_aev_hist_kernel<false>, dim3(grid), dim3(kAevBlock), 0, stream, vals, n, pass, rec, hist);
    hipLaunchKernelGGL(halo_aev_pick_kernel, dim3(1), dim3(kAevBlock), 0, stream, pass, rec, hist);
  }
  return hipGetLastError();
}

}  // namespace halo
