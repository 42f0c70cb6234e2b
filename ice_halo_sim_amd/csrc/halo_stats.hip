// halo_stats.hip — the image-statistics stage of the device consumer (halo_consumer_stats): exact percentiles and moments of the positive values
// of the consumer's Y (or of one class lane), the numbers the reference's doc/xyz-stats-tool.md tabulates, where the image lies.
//   1. The first sweep writes the values (Y = sum + comp, one float add: what halo_post_snapshot_kernel hands out), histograms their first radix
//      digit and gathers the moments as INTEGERS: a count of the values with v / norm > 1, an unsigned max of the bit patterns, and per exponent
//      field e the sums of the 24-bit significand m and of the two 24-bit halves of m * m, in 64-bit LDS bins (2^25 values x 2^24 < 2^49).  No
//      sum depends on the order of its adds; the host turns the bins into the exact sums rounded once (halo_host.cpp BinnedSum).
//   2. A radix select (11 + 11 + 10 bits, halo_radix.h) of up to 32 ranks at once.  The first-digit histogram serves every rank; after a digit,
//      ranks that share a prefix share a histogram (a "group"; r and r + 1 almost always do).  One sweep over the values fills the histograms of
//      kStBatch groups (2048 bins each; twice as many of the last digit's 1024), so a digit takes ceil(G / batch) sweeps for G groups.  The pick
//      after a digit turns each group's histogram into running sums (one wave per group), finds every rank's bin by bisection (one thread per
//      rank) and regroups the ranks, which stay sorted: equal prefixes are neighbours.
// Two forms, as in halo_autoev.hip: one workgroup doing everything back to back out of LDS for small inputs; above that many workgroups per
// sweep, adding their LDS histograms to global ones, with a one-workgroup pick kernel between digits.  The state (StatsSel) travels in device
// memory; the host reads one record, at the end.  Every count is an integer: the record is bit-reproducible.
#include "halo_launch.h"
#include "halo_radix.h"

namespace halo {

namespace {

constexpr uint32_t kStBatch = 7u;                                       // 2048-bin histograms one sweep fills: 56 KB of LDS, two workgroups per CU
__host__ __device__ constexpr uint32_t st_batch(uint32_t pass) { return pass == 2u ? 2u * kStBatch : kStBatch; }
constexpr uint32_t kStLdsWords = kStBatch * kAevBins;
constexpr uint32_t kStFirstWords = kAevBins + 2u * 3u * kStatsExpBins;   // the first sweep's LDS: first-digit histogram, then the 64-bit moment bins
constexpr uint32_t kStSelWords = sizeof(StatsSel) / sizeof(uint32_t);
static_assert(kStFirstWords <= kStLdsWords && 2u * kStBatch <= kStatsMaxRanks, "the first sweep fits the select's histograms");

__device__ __forceinline__ uint32_t st_wave_incl(uint32_t x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t v = static_cast<uint32_t>(__shfl_up(static_cast<int>(x), d));
    if (lane >= d) x += v;
  }
  return x;
}

// The first sweep over pixels first, first + stride, ...: see 1. above.  h: kAevBins words, bins: 3 x 256 64-bit words, both zeroed LDS; tot[0]
// counts the saturated values, tot[1] takes the max pattern.  A thread keeps the sums of a run of values with one exponent in registers.
template <bool LANE>
__device__ __forceinline__ void st_first_sweep(const float* __restrict__ sum, const float* __restrict__ comp, const double* __restrict__ lane, uint32_t n_pix,
                                               uint32_t first, uint32_t stride, float norm, float* __restrict__ vals, uint32_t* h, unsigned long long* bins,
                                               uint32_t* tot) {
  uint32_t sat = 0u, mx = 0u, ce = 0u;
  unsigned long long am = 0ull, al = 0ull, ah = 0ull;
  for (uint32_t p = first; p < n_pix; p += stride) {
    float v;
    if constexpr (LANE) {
      v = static_cast<float>(lane[p]);
    } else {
      const size_t i = 3u * static_cast<size_t>(p) + 1u;
      v = __fadd_rn(sum[i], comp[i]);
    }
    vals[p] = v;
    if (!(v > 0.0f)) continue;   // (NaN too)
    const uint32_t u = __float_as_uint(v);
    atomicAdd(&h[u >> aev_shift(0u)], 1u);
    mx = u > mx ? u : mx;
    if (__fdiv_rn(v, norm) > 1.0f) sat++;
    const uint32_t e = (u >> 23) & 255u, m = (u & 0x7FFFFFu) | (e ? 0x800000u : 0u);
    if (e != ce) {
      if (am) {
        atomicAdd(&bins[ce], am);
        atomicAdd(&bins[kStatsExpBins + ce], al);
        atomicAdd(&bins[2u * kStatsExpBins + ce], ah);
      }
      ce = e;
      am = al = ah = 0ull;
    }
    const unsigned long long q = static_cast<unsigned long long>(m) * m;
    am += m;
    al += q & 0xFFFFFFull;
    ah += q >> 24;
  }
  if (am) {
    atomicAdd(&bins[ce], am);
    atomicAdd(&bins[kStatsExpBins + ce], al);
    atomicAdd(&bins[2u * kStatsExpBins + ce], ah);
  }
  if (sat) atomicAdd(&tot[0], sat);
  if (mx) atomicMax(&tot[1], mx);
}

// A later digit's sweep: the values whose higher digits equal one of the ng (ascending) prefixes gp[] count in that group's histogram, nb bins each.
__device__ __forceinline__ void st_sweep(const float* __restrict__ vals, uint32_t n, uint32_t first, uint32_t stride, uint32_t pass, const uint32_t* gp, uint32_t ng,
                                         uint32_t* h) {
  const uint32_t shift = aev_shift(pass), width = aev_width(pass), mask = (1u << width) - 1u, hi = shift + width;
  const uint32_t gmin = gp[0], gmax = gp[ng - 1u];
  for (uint32_t i = first; i < n; i += stride) {
    const float v = vals[i];
    if (!(v > 0.0f)) continue;
    const uint32_t u = __float_as_uint(v), key = u >> hi;
    if (key < gmin || key > gmax) continue;
    for (uint32_t k = 0; k < ng; k++)
      if (gp[k] == key) {
        atomicAdd(&h[(k << width) + ((u >> shift) & mask)], 1u);
        break;
      }
  }
}

// Histograms -> exclusive running sums, in place: ng histograms of nb bins (a multiple of 64) at hist, one wave each.  *total0 (may be null)
// receives the total of histogram 0.  Every thread of the workgroup calls.
template <uint32_t NB>
__device__ __forceinline__ void st_cumulate_n(uint32_t* hist, uint32_t ng, uint32_t* total0) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  for (uint32_t g = w; g < ng; g += kAevBlock / 64) {   // (wave-uniform)
    uint32_t* hg = hist + g * NB;
    uint32_t x[NB / 64u];
#pragma unroll
    for (uint32_t k = 0; k < NB / 64u; k++) x[k] = hg[64u * k + lane];   // (all loads in flight before the first scan)
    uint32_t carry = 0u;
#pragma unroll
    for (uint32_t k = 0; k < NB / 64u; k++) {
      const uint32_t inc = st_wave_incl(x[k]);
      hg[64u * k + lane] = carry + inc - x[k];
      carry += static_cast<uint32_t>(__shfl(static_cast<int>(inc), 63));
    }
    if (total0 && g == 0u && lane == 0u) *total0 = carry;
  }
}
__device__ __forceinline__ void st_cumulate(uint32_t* hist, uint32_t ng, uint32_t nb, uint32_t* total0) {
  if (nb == kAevBins) st_cumulate_n<kAevBins>(hist, ng, total0);
  else st_cumulate_n<kAevBins / 2u>(hist, ng, total0);
}

// After the first digit's running sums gave n = sel->n > 0: the ranks.  numpy's default rule — vi = q (n - 1), ONE float64 product of the quotient
// the host made (q = percentile / 100), rank = floor(vi), frac = vi - rank, upper rank min(rank + 1, n - 1) — then the up to 2 P ranks sorted,
// without repeats, into sel->rank[0 .. K), each percentile keeping the places of its two.  Every thread of the workgroup calls.
__device__ __forceinline__ void st_setup(const StatsAsk& ask, StatsSel* sel, StatsRecord* rec, uint32_t* want, uint32_t* fresh) {
  const uint32_t t = threadIdx.x, P = ask.count, n = sel->n;
  if (t < P) {
    // (the product and the subtraction round on their own — fused, frac would keep bits the host's vi has lost: this file is built without contraction)
    double q = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < kStatsMaxQ; j++)
      if (j == t) q = ask.q[j];
    const double vi = __dmul_rn(q, static_cast<double>(n - 1u)), fl = floor(vi);
    const uint32_t r = static_cast<uint32_t>(fl);
    want[2u * t] = r;
    want[2u * t + 1u] = r + 1u < n ? r + 1u : n - 1u;
    rec->rank[t] = r;
    rec->frac[t] = __dsub_rn(vi, fl);
  }
  __syncthreads();
  if (t < 2u * P) {
    uint32_t f = 1u;
    for (uint32_t i = 0; i < t; i++)
      if (want[i] == want[t]) f = 0u;
    fresh[t] = f;
  }
  __syncthreads();
  if (t < 2u * P) {
    uint32_t pos = 0u;
    for (uint32_t i = 0; i < 2u * P; i++)
      if (fresh[i] && want[i] < want[t]) pos++;
    if (fresh[t]) {
      sel->rank[pos] = want[t];
      sel->pref[pos] = 0u;
      sel->group[pos] = 0u;
    }
    if (t & 1u) rec->idx_hi[t >> 1] = pos;
    else rec->idx_lo[t >> 1] = pos;
  }
  if (t == 0u) {
    uint32_t K = 0u;
    for (uint32_t i = 0; i < 2u * P; i++) K += fresh[i];
    sel->K = K;
    sel->G = 1u;
    sel->gpref[0] = 0u;
  }
  __syncthreads();
}

// Each rank of groups [g0, g0 + ng), whose running sums lie at hist: the last bin whose running sum is <= the rank (it is not empty, because the
// next one's exceeds the rank) extends the rank's prefix, and the rank becomes the rank inside that bin.  Every thread of the workgroup calls.
__device__ __forceinline__ void st_locate(uint32_t pass, const uint32_t* hist, uint32_t g0, uint32_t ng, StatsSel* sel) {
  const uint32_t t = threadIdx.x, width = aev_width(pass), nb = 1u << width;
  if (t < sel->K) {
    const uint32_t g = sel->group[t];
    if (g >= g0 && g < g0 + ng) {
      const uint32_t* hg = hist + (g - g0) * nb;
      const uint32_t r = sel->rank[t];
      uint32_t lo = 0u, hi = nb - 1u;
      while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (hg[mid] <= r) lo = mid;
        else hi = mid - 1u;
      }
      sel->pref[t] = (sel->pref[t] << width) | lo;
      sel->rank[t] = r - hg[lo];
    }
  }
  __syncthreads();
}

// The groups of the next digit: the distinct prefixes, in order (the ranks ascend, so do their prefixes).  Every thread of the workgroup calls.
__device__ __forceinline__ void st_regroup(StatsSel* sel) {
  const uint32_t t = threadIdx.x, K = sel->K;
  if (t < K) {
    uint32_t gid = 0u;
    for (uint32_t i = 1; i <= t; i++) gid += sel->pref[i] != sel->pref[i - 1u] ? 1u : 0u;
    sel->group[t] = gid;
    sel->gpref[gid] = sel->pref[t];
    if (t == K - 1u) sel->G = gid + 1u;
  }
  __syncthreads();
}

// After the last digit a rank's prefix is its order statistic's bit pattern.
__device__ __forceinline__ void st_finish(const StatsSel* sel, StatsRecord* rec, uint32_t P) {
  const uint32_t t = threadIdx.x;
  if (t < P) {
    rec->lo_bits[t] = sel->pref[rec->idx_lo[t]];
    rec->hi_bits[t] = sel->pref[rec->idx_hi[t]];
  }
}

__device__ __forceinline__ void st_store_sel(const StatsSel* sel, StatsRecord* rec) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(sel);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&rec->sel);
  for (uint32_t i = threadIdx.x; i < kStSelWords; i += kAevBlock) dst[i] = src[i];
}

}  // namespace

// The whole call by one workgroup: the first sweep, then per digit the sweeps of its batches of groups and the pick after each, out of LDS.
template <bool LANE>
__global__ void __launch_bounds__(kAevBlock) halo_stats_small_kernel(const float* __restrict__ sum, const float* __restrict__ comp, const double* __restrict__ lane,
                                                                     uint32_t n_pix, float norm, StatsAsk ask, float* vals, StatsRecord* rec) {
  __shared__ __attribute__((aligned(16))) uint32_t h[kStLdsWords];
  __shared__ StatsSel sel;
  __shared__ uint32_t want[kStatsMaxRanks], fresh[kStatsMaxRanks], tot[2];
  const uint32_t t = threadIdx.x;
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(h + kAevBins);
  for (uint32_t i = t; i < kStFirstWords; i += kAevBlock) h[i] = 0u;
  for (uint32_t i = t; i < kStSelWords; i += kAevBlock) reinterpret_cast<uint32_t*>(&sel)[i] = 0u;
  if (t < 2u) tot[t] = 0u;
  __syncthreads();
  st_first_sweep<LANE>(sum, comp, lane, n_pix, t, kAevBlock, norm, vals, h, bins, tot);
  __syncthreads();   // (also: this workgroup's vals are visible to all of it)
  for (uint32_t i = t; i < 3u * kStatsExpBins; i += kAevBlock) rec->bins[i] = bins[i];
  if (t == 0u) {
    rec->sat = tot[0];
    rec->max_bits = tot[1];
  }
  st_cumulate(h, 1u, kAevBins, &sel.n);
  __syncthreads();
  if (sel.n != 0u && ask.count != 0u) {   // (workgroup-uniform)
    st_setup(ask, &sel, rec, want, fresh);
    st_locate(0u, h, 0u, 1u, &sel);
    st_regroup(&sel);
    for (uint32_t pass = 1; pass < 3u; pass++) {
      const uint32_t nb = 1u << aev_width(pass), G = sel.G;
      for (uint32_t g0 = 0; g0 < G; g0 += st_batch(pass)) {
        const uint32_t ng = G - g0 < st_batch(pass) ? G - g0 : st_batch(pass);
        for (uint32_t i = t; i < ng * nb; i += kAevBlock) h[i] = 0u;
        __syncthreads();
        st_sweep(vals, n_pix, t, kAevBlock, pass, sel.gpref + g0, ng, h);
        __syncthreads();
        st_cumulate(h, ng, nb, nullptr);
        __syncthreads();
        st_locate(pass, h, g0, ng, &sel);
      }
      if (pass == 1u) st_regroup(&sel);
    }
    st_finish(&sel, rec, ask.count);
  }
  st_store_sel(&sel, rec);
}

// Large images.  The first sweep by many workgroups: LDS histogram and bins, then one add of what is not empty to the global ones (zeroed by the launcher).
template <bool LANE>
__global__ void __launch_bounds__(kAevBlock) halo_stats_first_kernel(const float* __restrict__ sum, const float* __restrict__ comp, const double* __restrict__ lane,
                                                                     uint32_t n_pix, float norm, float* __restrict__ vals, StatsRecord* rec, uint32_t* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) uint32_t h[kStFirstWords];
  __shared__ uint32_t tot[2];
  const uint32_t t = threadIdx.x;
  unsigned long long* bins = reinterpret_cast<unsigned long long*>(h + kAevBins);
  for (uint32_t i = t; i < kStFirstWords; i += kAevBlock) h[i] = 0u;
  if (t < 2u) tot[t] = 0u;
  __syncthreads();
  st_first_sweep<LANE>(sum, comp, lane, n_pix, blockIdx.x * kAevBlock + t, gridDim.x * kAevBlock, norm, vals, h, bins, tot);
  __syncthreads();
  for (uint32_t i = t; i < kAevBins; i += kAevBlock)
    if (h[i]) atomicAdd(&hist[i], h[i]);
  for (uint32_t i = t; i < 3u * kStatsExpBins; i += kAevBlock)
    if (bins[i]) atomicAdd(&rec->bins[i], bins[i]);
  if (t == 0u) {
    if (tot[0]) atomicAdd(&rec->sat, tot[0]);
    if (tot[1]) atomicMax(&rec->max_bits, tot[1]);
  }
}

// A later digit's sweep for batch `batch` of the groups the previous pick left, into hist[group][bin] of this digit (zeroed by the launcher).
__global__ void __launch_bounds__(kAevBlock) halo_stats_hist_kernel(const float* __restrict__ vals, uint32_t n, uint32_t pass, uint32_t batch, const StatsRecord* rec,
                                                                    uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[kStLdsWords];
  __shared__ uint32_t gp[2u * kStBatch];
  const uint32_t t = threadIdx.x, G = rec->sel.G, g0 = batch * st_batch(pass), nb = 1u << aev_width(pass);
  if (rec->sel.n == 0u || rec->sel.K == 0u || g0 >= G) return;   // nothing positive, nothing asked, or fewer groups than the launcher provided for
  const uint32_t ng = G - g0 < st_batch(pass) ? G - g0 : st_batch(pass);
  if (t < ng) gp[t] = rec->sel.gpref[g0 + t];
  for (uint32_t i = t; i < ng * nb; i += kAevBlock) h[i] = 0u;
  __syncthreads();
  st_sweep(vals, n, blockIdx.x * kAevBlock + t, gridDim.x * kAevBlock, pass, gp, ng, h);
  __syncthreads();
  for (uint32_t i = t; i < ng * nb; i += kAevBlock)
    if (h[i]) atomicAdd(&hist[g0 * nb + i], h[i]);
}

// ... and the one workgroup after a digit's sweeps: running sums, every rank's bin, the next digit's groups (or, after the last, the results).
__global__ void __launch_bounds__(kAevBlock) halo_stats_pick_kernel(uint32_t pass, StatsAsk ask, StatsRecord* rec, uint32_t* hist) {
  __shared__ StatsSel sel;
  __shared__ uint32_t want[kStatsMaxRanks], fresh[kStatsMaxRanks];
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < kStSelWords; i += kAevBlock)
    reinterpret_cast<uint32_t*>(&sel)[i] = pass ? reinterpret_cast<const uint32_t*>(&rec->sel)[i] : 0u;
  __syncthreads();
  if (pass == 0u) {
    st_cumulate(hist, 1u, kAevBins, &sel.n);
    __syncthreads();
    if (sel.n != 0u && ask.count != 0u) {
      st_setup(ask, &sel, rec, want, fresh);
      st_locate(0u, hist, 0u, 1u, &sel);
      st_regroup(&sel);
    }
  } else {
    if (sel.n == 0u || sel.K == 0u) return;
    st_cumulate(hist, sel.G, 1u << aev_width(pass), nullptr);
    __syncthreads();
    st_locate(pass, hist, 0u, sel.G, &sel);
    if (pass == 1u) st_regroup(&sel);
    else st_finish(&sel, rec, ask.count);
  }
  st_store_sel(&sel, rec);
}

hipError_t launch_stats(const float* sum, const float* comp, const double* lane, uint32_t n_pix, float norm, const StatsAsk& ask, float* vals, uint32_t* ws,
                        bool one_workgroup, int blocks, hipStream_t stream) {
  StatsRecord* rec = reinterpret_cast<StatsRecord*>(ws);
  uint32_t* hist = ws + kStatsRecWords;
  if (one_workgroup) {   // (the kernel writes every word of the record that the host reads)
    if (lane) hipLaunchKernelGGL(halo_stats_small_kernel<true>, dim3(1), dim3(kAevBlock), 0, stream, sum, comp, lane, n_pix, norm, ask, vals, rec);
    else hipLaunchKernelGGL(halo_stats_small_kernel<false>, dim3(1), dim3(kAevBlock), 0, stream, sum, comp, lane, n_pix, norm, ask, vals, rec);
    return hipGetLastError();
  }
  const uint32_t kmax = 2u * ask.count < kStatsMaxRanks ? 2u * ask.count : kStatsMaxRanks;   // the ranks, hence the groups, at most
  uint32_t* hist_of[3] = {hist, hist + kAevBins, hist + kAevBins + kmax * kAevBins};
  const size_t words = kStatsRecWords + kAevBins + static_cast<size_t>(kmax) * (kAevBins + (1u << aev_width(2u)));
  hipError_t e = hipMemsetAsync(ws, 0, words * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const uint32_t need = (n_pix + 4u * kAevBlock - 1u) / (4u * kAevBlock);   // at least four values per thread
  const uint32_t grid = need < static_cast<uint32_t>(blocks) ? (need ? need : 1u) : static_cast<uint32_t>(blocks);
  if (lane) hipLaunchKernelGGL(halo_stats_first_kernel<true>, dim3(grid), dim3(kAevBlock), 0, stream, sum, comp, lane, n_pix, norm, vals, rec, hist);
  else hipLaunchKernelGGL(halo_stats_first_kernel<false>, dim3(grid), dim3(kAevBlock), 0, stream, sum, comp, lane, n_pix, norm, vals, rec, hist);
  hipLaunchKernelGGL(halo_stats_pick_kernel, dim3(1), dim3(kAevBlock), 0, stream, 0u, ask, rec, hist);
  for (uint32_t pass = 1; pass < 3u && kmax > 0u; pass++) {
    const uint32_t batches = (kmax + st_batch(pass) - 1u) / st_batch(pass);
    for (uint32_t b = 0; b < batches; b++)
      hipLaunchKernelGGL(halo_stats_hist_kernel, dim3(grid), dim3(kAevBlock), 0, stream, vals, n_pix, pass, b, rec, hist_of[pass]);
    hipLaunchKernelGGL(halo_stats_pick_kernel, dim3(1), dim3(kAevBlock), 0, stream, pass, ask, rec, hist_of[pass]);
  }
  return hipGetLastError();
}

}  // namespace halo
