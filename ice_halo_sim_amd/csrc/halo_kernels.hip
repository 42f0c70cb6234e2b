// halo_kernels.hip — the kernels around the trace kernel (the hit log's split and per-tile passes, binned-accumulation passes,
// plane fold, device consumer) and the launch dispatcher.  The trace kernel itself is a template in halo_trace.inl, instantiated per MODE in
// halo_trace_m{0,1,2}.hip.
#include "halo_trace.inl"
#include "halo_display.h"
#include "halo_launch.h"

namespace halo {

// Tile sums in 64-bit fixed point.  An fp64 LDS add is the slow kind here (tools/lds_atomic_bench.hip: ds_add_f64 1.5 T adds/s, ds_add_u64
// 2.9 T), and these passes are LDS-bound (the index unit ~70 % busy, profiles/r03_bench4_pmc_lds.txt) — so a record's weight becomes a
// 64-bit integer, weight x 2^F rounded to nearest, and integer sums do not depend on the order of the adds.  F comes with the launch
// (halo_backend.cpp fix_frac_bits): the largest F <= 32 for which 4 x (largest ray weight of the session) x (rays of the launch) x 2^F
// stays below 2^62 — no slot can sum to more than that bound (a ray's exits never outweigh the ray; x2 for the dual-fisheye overlap, x2
// for the CMF rows of the X/Y/Z pass), so the unsigned sums cannot wrap.  F = 32 (resolution 2.3e-10) for every launch of unit-weight
// rays up to 2^28; an illuminant session (spd weights ~100) of 2^26 rays runs F = 28.  (Round 3 had F fixed at 32 on the assumption
// "weight <= 1" and a signed read-out: 4e9 of weight in one slot wrapped negative — ADVICE r3.)  A NaN or negative weight adds nothing.
// A tile list is read once, by one workgroup, a moment after the split pass wrote it: loaded non-temporally (four dword loads the compiler merges
// into one `global_load_dwordx4 ... nt`) the per-tile pass of configs[1] takes 108 us instead of 137 — the same pass launched a second time on the
// same lists takes 107 (round 6, rocprofv3 per-kernel minima on one box; non-temporal STORES in the split pass cost it more than they save here).
// Short lists (a small session's: they sit in the caches whole) keep the ordinary load — `--config 4d` lost 0.8 % with the other; `once` is
// workgroup-uniform (the tile's record count).
constexpr uint32_t kListOnceMin = 1u << 16;
template <bool ONCE>   // (a run-time choice inside one loop comes out as ordinary loads on both sides: the loop exists twice instead)
__device__ __forceinline__ uint4 load_list_u4(const uint4* p) {
  if constexpr (!ONCE) return *p;
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
  return make_uint4(__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2), __builtin_nontemporal_load(q + 3));
}

// (struct FixQ: halo_trace.inl, beside the deterministic route's cache, which sums by the same rule)

// kBinSplit workgroups per image tile: each sums its share of the tile's hit list in a 64 KB LDS tile (8 independent
// loads in flight per thread — the loop is load-latency-bound otherwise) and adds the non-zero slots to the plane.
constexpr int kBinBlock = 1024;
constexpr uint32_t kBinSplit = 2u;
__global__ void __launch_bounds__(kBinBlock) halo_bin_accumulate_kernel(float* __restrict__ plane, const uint2* __restrict__ list, uint32_t cap,
                                                                         const uint32_t* __restrict__ cnt, uint32_t tiles_log2, uint32_t frac_bits) {
  const FixQ fq(frac_bits);
  // fp64 sums, and not for precision: on gfx950 ds_add_f32 retires ~0.3 lanes per clock per CU (200 G adds/s chip-wide) while
  // ds_add_f64 runs at 1500 G/s and ds_add_u32 at 4600 G/s (tools/lds_atomic_bench.hip) — the fp32 LDS atomic is the slow one,
  // and this pass is one LDS add per hit.  128 KB of the CU's 160 KB: one workgroup of 16 waves per CU.
  __shared__ unsigned long long acc[1u << kBinTileLog2];   // fixed point (FixQ)
  const uint32_t tile = blockIdx.x / kBinSplit, part = blockIdx.x % kBinSplit;
  const uint32_t n = min(cnt[tile * kBinCntStride], cap);
  const uint32_t lo = static_cast<uint32_t>(static_cast<uint64_t>(n) * part / kBinSplit);
  const uint32_t hi = static_cast<uint32_t>(static_cast<uint64_t>(n) * (part + 1u) / kBinSplit);
  if (hi <= lo) return;
  for (uint32_t j = threadIdx.x; j < (1u << kBinTileLog2); j += kBinBlock) acc[j] = 0ull;
  __syncthreads();
  const uint2* src = list + static_cast<size_t>(tile) * cap;
  constexpr uint32_t kU = 8u;
  uint32_t i = lo + threadIdx.x;
  for (; i + (kU - 1u) * kBinBlock < hi; i += kU * kBinBlock) {
    uint2 h[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) h[u] = src[i + u * kBinBlock];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) atomicAdd(&acc[h[u].x >> tiles_log2], fq.fix(__uint_as_float(h[u].y)));
  }
  for (; i < hi; i += kBinBlock) {
    const uint2 h = src[i];
    atomicAdd(&acc[h.x >> tiles_log2], fq.fix(__uint_as_float(h.y)));
  }
  __syncthreads();
  for (uint32_t j = threadIdx.x; j < (1u << kBinTileLog2); j += kBinBlock) {
    const float v = fq.unfix(acc[j]);
    if (v != 0.0f) atomic_add_f32(plane + ((static_cast<size_t>(j) << tiles_log2) | tile), v);
  }
}

hipError_t launch_bin_accumulate(float* plane, const HitRec* list, uint32_t cap, uint32_t* cnt, uint32_t tiles, uint32_t frac_bits, hipStream_t stream) {
  hipLaunchKernelGGL(halo_bin_accumulate_kernel, dim3(tiles * kBinSplit), dim3(kBinBlock), 0, stream, plane, reinterpret_cast<const uint2*>(list), cap, cnt, static_cast<uint32_t>(__builtin_ctz(tiles)), frac_bits);
  return hipGetLastError();
}

// Interleaved tiles of one accumulation plane (the hit log's full-sky and X/Y/Z routes).  A slot is row << s | column (MonoSlot:
// row = pixel mod 1024 — for the usual image widths the image column mod 1024 — and column = a hash of pixel / 1024, i.e. of the
// image row).  Contiguous slot ranges are bands of image columns and run 6x uneven on a full-sky render, whose light sits
// around the sun's azimuth; the column alone is just as uneven (the sun's elevation).  So a tile takes both: with T = 2^t tiles
// and S = 2^s columns, tile = (column + row) mod T for T <= S, else (row mod T/S) * S + (column + row / (T/S)) mod S; `local` is
// what is left of the slot.  1024 * S / T slots per tile, a bijection (slot_of inverts it).
struct TileMap {
  uint32_t s, t;
  __device__ __forceinline__ void split(uint32_t slot, uint32_t& tile, uint32_t& local) const {
    const uint32_t row = slot >> s, col = slot & ((1u << s) - 1u);
    if (t <= s) {
      tile = (col + row) & ((1u << t) - 1u);
      local = (row << (s - t)) | (col >> t);
    } else {
      const uint32_t d = t - s;
      tile = ((row & ((1u << d) - 1u)) << s) | ((col + (row >> d)) & ((1u << s) - 1u));
      local = row >> d;
    }
  }
  __device__ __forceinline__ uint32_t slot_of(uint32_t tile, uint32_t local) const {
    if (t <= s) {
      const uint32_t row = local >> (s - t), chi = local & ((1u << (s - t)) - 1u);
      return (row << s) | (chi << t) | ((tile - row) & ((1u << t) - 1u));
    }
    const uint32_t d = t - s, r_hi = local;
    return ((((r_hi << d) | (tile >> s))) << s) | (((tile & ((1u << s) - 1u)) - r_hi) & ((1u << s) - 1u));
  }
};

// ---- the split pass: hit records of a source list dealt out to per-tile lists ----
// Two callers.  (1) Two-level binning, accumulators of more than 512 tiles (per-wavelength planes: 64 planes x 2 Mi slots = 8192
// tiles): the trace kernel can feed at most 512 lists from its 1536-record LDS buffer (fewer than ~3 records per list and flush
// and the appends stop coalescing), so its lists are COARSE — list l1 holds the hits of `fan` consecutive tiles (bin_shift = 14 +
// fan_log2) — and this kernel deals each coarse list out to its `fan` tile lists, kSplitParts workgroups per list.  (2) The hit
// log (halo_trace.inl log_hit): one UNSORTED region per trace workgroup, every region may hold every tile of an accumulator of
// at most kSplitFanMax tiles; one workgroup per region.
// A workgroup takes 4096 records per step.  Scattered 8-byte stores run at ~90 G/s on this part whatever their locality
// (tools/atomic_rate_bench.hip), so the records of a step are first SORTED by tile in LDS — rank from an LDS counter per tile,
// run offsets from a scan of the counters — and then written by consecutive lanes: a wave's store covers a few runs of
// consecutive addresses instead of 64 lists (the log split went from 0.67 to 0.37 ms per 68 M records with that).  One returning
// global atomic per tile and step reserves the run's place in the tile list; a tile list that overflows falls back to direct
// atomics on the plane.
constexpr uint32_t kSplitParts = 8u;
#ifndef HALO_SPLIT_THREADS
#define HALO_SPLIT_THREADS 1024
#endif
#ifndef HALO_SPLIT_PER
#define HALO_SPLIT_PER 16
#endif
// the hit log's split: records per step = threads x per.  Round 4 tried the shapes that put two workgroups on a CU (the kernel waits 61 % of its
// wave cycles, profiles/r04_ref_bench_light_single_ms_pmc_wait.txt): 512 x 16 and 1024 x 8 (8 Ki records, 70 KB) and 512 x 32 (16 Ki, eight waves)
// are 3-4 %, 4-5 % and 1.5-3 % SLOWER on the whole step of bench_light_single_ms / configs[1] / ms_multi_crystal — the length of the runs a step
// writes (32 records = 256 B per list at 512 lists) matters more than a second workgroup to hide the latencies behind
constexpr uint32_t kLogSplitThreads = HALO_SPLIT_THREADS, kLogSplitPer = HALO_SPLIT_PER;
// Step sizes (threads x records per thread).  The hit log has 128..256 destinations per step, and its stores only coalesce
// when a step is large: 16384 records (a region is read in one or two steps; 128 KB of LDS, one workgroup per CU) runs
// at 0.23 ms per 58 M records where 4096 takes 0.36 and 1024 takes 1.1.  The coarse lists of the two-level route have <= 32
// destinations per step, whose runs are long anyway, and ~1000 long chains that want many workgroups resident: 256 x 16.
// Tile of a record: ((slot & slot_mask) >> tile_log2) & (fan - 1) — contiguous 16 Ki-slot tiles of the plane array (tile_log2 14),
// or, X/Y/Z hit log, interleaved tiles of one plane (tile_log2 0, mix_log2 = log2 of the plane's columns; the wavelength-pool
// entry above the slot is cut off by slot_mask).  kSplitFanMax = destination tiles per source list.
struct SplitXyz {              // what a record that finds its tile list full is added to
  const WlEntryDev* pool;      // X/Y/Z hit log; nullptr = scalar planes: plane[slot] += w
  uint32_t pool_size;          // CMF codes: pool entries, then pool_size + c = "the weight is channel c already"
  uint32_t plane_stride;
  double* ovf;                 // the planes' fp64 twin (DispatchParams::ovf); nullptr = the fp32 plane itself
  uint32_t* ovf_flag;
  uint32_t plane_log2;         // log2 of a plane copy's floats, and of the privatised copies per plane: the twin has no copies (TwinOffset)
  uint32_t copies_log2;
};
__device__ __forceinline__ void split_overflow(float* plane, const SplitXyz& x, size_t off, float v) {
  if (x.ovf != nullptr) {
    atomicAdd(x.ovf + TwinOffset(off, x.plane_log2, x.copies_log2), static_cast<double>(v));
    *x.ovf_flag = 1u;
  } else {
    atomic_add_f32(plane + off, v);
  }
}
// The deterministic route's log (kFix instantiations: halo_split_fixed_kernel) differs in the fallback alone: a record that finds its tile list
// full is quantised with the session's F — X/Y/Z: the three fp32 products first — and added to the integer planes with integer atomics.
struct SplitFix {
  unsigned long long* planes;  // DispatchParams::fix
  uint32_t frac_bits;          // the session's F
};
template <uint32_t kSplitBlock, uint32_t kSplitPer, uint32_t kSplitFanMax, bool kXyz, bool kMix, bool kFix>
__device__ __forceinline__ void split_body(float* __restrict__ plane, const uint2* __restrict__ list1, uint32_t cap1,
                                           const uint32_t* __restrict__ cnt1, uint32_t cnt1_stride, uint32_t parts,
                                           uint2* __restrict__ list2, uint32_t cap2, uint32_t* __restrict__ cnt2, uint32_t fan_log2,
                                           uint32_t coarse, uint32_t slot_mask, uint32_t tile_log2, uint32_t mix_log2, const SplitXyz& xyz, const SplitFix& fix) {
  __shared__ __attribute__((aligned(16))) uint32_t s_cnt[kSplitFanMax];
  __shared__ __attribute__((aligned(16))) uint32_t s_off[kSplitFanMax];
  __shared__ uint32_t s_base[kSplitFanMax];
  __shared__ uint2 s_rec[kSplitBlock * kSplitPer];
  static_assert(kSplitBlock >= kSplitFanMax && kSplitFanMax % 256u == 0u, "one thread per tile counter; the scan takes 4 per lane and round");
  const uint32_t l1 = blockIdx.x / parts, part = blockIdx.x % parts;
  const uint32_t n = min(cnt1[static_cast<size_t>(l1) * cnt1_stride], cap1);
  const uint32_t lo = static_cast<uint32_t>(static_cast<uint64_t>(n) * part / parts);
  const uint32_t hi = static_cast<uint32_t>(static_cast<uint64_t>(n) * (part + 1u) / parts);
  const uint32_t fmask = (1u << fan_log2) - 1u;
  // kMix: interleaved tiles (TileMap, s = mix_log2, t = fan_log2); else contiguous ranges of 2^tile_log2 slots
  auto tile_of = [&](uint32_t x) {
    const uint32_t sl = x & slot_mask;
    if (kMix) {   // interleaved tiles of ONE plane; the planes of a per-entry-plane session lie back to back, each with its own 2^fan_log2 tiles
      uint32_t tile, local;
      TileMap{mix_log2, fan_log2}.split(sl & ((1u << (mix_log2 + 10u)) - 1u), tile, local);
      return ((sl >> (mix_log2 + 10u)) << fan_log2) | tile;
    }
    return (sl >> tile_log2) & fmask;
  };
  const uint32_t tile0 = coarse ? (l1 << fan_log2) : 0u;   // the first destination tile of this source list
  const uint2* src = list1 + static_cast<size_t>(l1) * cap1;
  // The steps of a workgroup are a chain of dependent latencies (loads, LDS ranks, the reserving atomic, stores), so the next
  // step's records are loaded while this step's are written out, and the reserving atomic flies during the LDS scatter.
  uint2 h[kSplitPer];
  uint32_t rank[kSplitPer];
#pragma unroll
  for (uint32_t u = 0; u < kSplitPer; ++u) {
    const uint32_t i = lo + u * kSplitBlock + threadIdx.x;
    h[u] = i < hi ? src[i] : make_uint2(0xFFFFFFFFu, 0u);
  }
  if (threadIdx.x < kSplitFanMax) s_cnt[threadIdx.x] = 0u;
  __syncthreads();
  for (uint32_t b0 = lo; b0 < hi; b0 += kSplitBlock * kSplitPer) {   // workgroup-uniform trip count
#pragma unroll
    for (uint32_t u = 0; u < kSplitPer; ++u)
      rank[u] = h[u].x != 0xFFFFFFFFu ? atomicAdd(&s_cnt[tile_of(h[u].x)], 1u) : 0u;
    __syncthreads();
    if (threadIdx.x < 64u) {   // exclusive scan of the counters by one wave: 4 per lane and round
      uint32_t carry = 0u;
#pragma unroll
      for (uint32_t g = 0; g < kSplitFanMax; g += 256u) {
        const uint4 c = *reinterpret_cast<const uint4*>(&s_cnt[g + threadIdx.x * 4u]);
        const uint32_t own = c.x + c.y + c.z + c.w;
        uint32_t incl = own;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t up = __shfl_up(incl, d);
          if (static_cast<int>(threadIdx.x) >= d) incl += up;
        }
        const uint32_t ex = carry + incl - own;
        *reinterpret_cast<uint4*>(&s_off[g + threadIdx.x * 4u]) = make_uint4(ex, ex + c.x, ex + c.x + c.y, ex + c.x + c.y + c.z);
        carry += __shfl(incl, 63);
      }
    }
    const uint32_t c_own = threadIdx.x < kSplitFanMax ? s_cnt[threadIdx.x] : 0u;
    const uint32_t base = c_own ? atomicAdd(&cnt2[static_cast<size_t>(tile0 + threadIdx.x) * kBinCntStride], c_own) : 0u;
    __syncthreads();
    if (threadIdx.x < kSplitFanMax) s_cnt[threadIdx.x] = 0u;   // for the next step (ranked after the barrier that ends this one)
#pragma unroll
    for (uint32_t u = 0; u < kSplitPer; ++u)
      if (h[u].x != 0xFFFFFFFFu) s_rec[s_off[tile_of(h[u].x)] + rank[u]] = h[u];
    const uint32_t nb = b0 + kSplitBlock * kSplitPer;
#pragma unroll
    for (uint32_t u = 0; u < kSplitPer; ++u) {
      const uint32_t i = nb + u * kSplitBlock + threadIdx.x;
      h[u] = i < hi ? src[i] : make_uint2(0xFFFFFFFFu, 0u);
    }
    if (threadIdx.x < kSplitFanMax) s_base[threadIdx.x] = base;
    __syncthreads();
    const uint32_t n_step = min(kSplitBlock * kSplitPer, hi - b0);
#pragma unroll
    for (uint32_t u = 0; u < kSplitPer; ++u) {
      const uint32_t i = u * kSplitBlock + threadIdx.x;
      if (i >= n_step) continue;
      const uint2 r = s_rec[i];
      const uint32_t t = tile_of(r.x);
      const uint32_t pos = s_base[t] + (i - s_off[t]);
      if (pos < cap2) {
        list2[static_cast<size_t>(tile0 + t) * cap2 + pos] = r;
      } else if constexpr (kFix) {
        const FixQ fq(fix.frac_bits);
        const float w = __uint_as_float(r.y);
        if constexpr (kXyz) {
          const uint32_t code = r.x >> kLogWlShift;
          if (code < xyz.pool_size) {   // (a deterministic launch logs pool entries only: no unit rows)
            const WlEntryDev e = xyz.pool[code];
            unsigned long long* at = fix.planes + (r.x & slot_mask);
            atomicAdd(at, fq.fix(e.cmf_x * w));
            atomicAdd(at + xyz.plane_stride, fq.fix(e.cmf_y * w));
            atomicAdd(at + 2u * static_cast<size_t>(xyz.plane_stride), fq.fix(e.cmf_z * w));
          }
        } else {
          atomicAdd(fix.planes + r.x, fq.fix(w));
        }
      } else if (kXyz) {
        const uint32_t code = r.x >> kLogWlShift;
        float c[3];
        if (code < xyz.pool_size) {
          const WlEntryDev e = xyz.pool[code];
          c[0] = e.cmf_x, c[1] = e.cmf_y, c[2] = e.cmf_z;
        } else {
          for (uint32_t k = 0; k < 3u; ++k) c[k] = code == xyz.pool_size + k ? 1.0f : 0.0f;
        }
        const size_t at = r.x & slot_mask;
        for (uint32_t k = 0; k < 3u; ++k)
          if (c[k] != 0.0f) split_overflow(plane, xyz, at + static_cast<size_t>(k) * xyz.plane_stride, c[k] * __uint_as_float(r.y));
      } else {
        split_overflow(plane, xyz, r.x, __uint_as_float(r.y));
      }
    }
    __syncthreads();
  }
}
template <uint32_t kSplitBlock, uint32_t kSplitPer, uint32_t kSplitFanMax, bool kXyz, bool kMix>
__global__ void __launch_bounds__(kSplitBlock) halo_split_kernel(float* __restrict__ plane, const uint2* __restrict__ list1, uint32_t cap1,
                                                                 const uint32_t* __restrict__ cnt1, uint32_t cnt1_stride, uint32_t parts,
                                                                 uint2* __restrict__ list2, uint32_t cap2, uint32_t* __restrict__ cnt2, uint32_t fan_log2,
                                                                 uint32_t coarse, uint32_t slot_mask, uint32_t tile_log2, uint32_t mix_log2, SplitXyz xyz) {
  split_body<kSplitBlock, kSplitPer, kSplitFanMax, kXyz, kMix, false>(plane, list1, cap1, cnt1, cnt1_stride, parts, list2, cap2, cnt2, fan_log2, coarse, slot_mask, tile_log2,
                                                                      mix_log2, xyz, SplitFix{nullptr, 0u});
}
template <uint32_t kSplitBlock, uint32_t kSplitPer, uint32_t kSplitFanMax, bool kXyz, bool kMix>
__global__ void __launch_bounds__(kSplitBlock) halo_split_fixed_kernel(const uint2* __restrict__ list1, uint32_t cap1, const uint32_t* __restrict__ cnt1,
                                                                       uint2* __restrict__ list2, uint32_t cap2, uint32_t* __restrict__ cnt2, uint32_t fan_log2,
                                                                       uint32_t slot_mask, uint32_t tile_log2, uint32_t mix_log2, SplitXyz xyz, SplitFix fix) {
  split_body<kSplitBlock, kSplitPer, kSplitFanMax, kXyz, kMix, true>(nullptr, list1, cap1, cnt1, 1u, 1u, list2, cap2, cnt2, fan_log2, 0u, slot_mask, tile_log2, mix_log2, xyz, fix);
}

// One workgroup per tile of 16 Ki CONSECUTIVE slots: sums the tile's list in LDS and adds the tile to the plane with plain
// coalesced float4 read-modify-writes — the workgroup is the only writer of those slots while this kernel runs (direct
// atomics of the trace / split kernels are ordered before it on the stream).
// (kFix, the deterministic route's integer twin: `plane` is the integer plane, frac_bits the session's F, and the write-out ADDS the LDS integers
// to it — no-return 64-bit atomics for the non-zero slots, so it needs no ordering against any other writer.  The float instantiation's code is
// what it was.)
// (kClose, the float route's closing form, for a launch that is its whole session — DESIGN.md 3.2: the plane is zero before this pass, so the tile's
// sums ARE the plane, and the workgroup, the only writer of its tile, adds coef x sum to the XYZ image itself — what the closing fold would do
// with the plane it read back, value for value: the twin taken in and zeroed when its flag is up, the slot mapped back to its pixel, the product
// and the add rounded separately.  `plane` and `cnt` are not used (null): the plane is neither read nor written, and the tile's count is read and
// ZEROED through CloseArgs::cnt — the next split pass on this list set, later on the same stream, finds its counters clear.  The twin's flag is
// read by every workgroup, so no workgroup may clear it: a 4-byte memset follows the kernel on its stream (an end-of-grid ticket — the last
// workgroup to finish clears the flag — measured no better than the memset, profiles/direct_close_ab.txt, and is not kept).)
template <bool kClose>
struct CloseArgsOf {};
template <>
struct CloseArgsOf<true> {
  float* xyz;         // the image: 3 floats per pixel
  uint32_t n_pix;
  uint32_t s_log2;    // columns per plane row (MonoSlot)
  float coef[3];      // the session's CMF
  uint32_t* cnt;      // the tile lists' counters (read, then zeroed)
  double* twin;       // the plane's fp64 twin and its flag (DispatchParams::ovf, ovf_flag)
  const uint32_t* flag;
};
// image += coef x sum as the fold makes it: the product rounded, then the add (the fold's product goes through LDS before it meets the image;
// written as one expression here, the two would contract into one fma and round once)
__device__ __forceinline__ float close_add(float q, float c, float v) {
#pragma clang fp contract(off)
  const float p = c * v;
  return q + p;
}
// a workgroup's last step in the closing form: its counter cleared
__device__ __forceinline__ void close_done(const CloseArgsOf<true>& cl, uint32_t tile) {
  __syncthreads();   // every thread has the count it loaded
  if (threadIdx.x == 0u) cl.cnt[static_cast<size_t>(tile) * kBinCntStride] = 0u;
}
// The closing form's write-out, shared by the pass over tile lists (halo_bin_accumulate_range_kernel<false, true>) and the pass over per-tile chunks
// (halo_tile_close_kernel): `acc` holds the tile's fixed-point sums, every thread of the workgroup is behind the barrier that completes them.
template <typename Acc>   // (the LDS array itself, not a pointer to it: the sums are read with LDS instructions)
__device__ __forceinline__ void close_write_out(const Acc& acc, const FixQ fq, const uint32_t tile, const uint32_t tile_log2, const uint32_t slots, const bool take_twin,
                                                const CloseArgsOf<true> cl) {
  // Consecutive lanes take consecutive ROWS of one column — consecutive pixels — in runs of up to eight (96 bytes of XYZ; the fold's own runs are
  // 48 bytes and more), then the next column.  A tile-local slot is row bits above `cb` column bits.
  const uint32_t s_mask = (1u << cl.s_log2) - 1u;
  const uint32_t cb = min(cl.s_log2, tile_log2), rl = min(tile_log2 - cb, 3u);
  const uint32_t base = tile << tile_log2;
  for (uint32_t i = threadIdx.x; i < slots; i += kBinBlock) {
    const uint32_t rest = i >> rl;
    const uint32_t j = (((((rest >> cb) << rl) | (i & ((1u << rl) - 1u))) << cb) | (rest & ((1u << cb) - 1u)));
    const uint32_t slot = base | j;
    float v = fq.unfix(acc[j]);
    if (take_twin) {
      const double o = cl.twin[slot];
      if (o != 0.0) {
        cl.twin[slot] = 0.0;
        v = static_cast<float>(static_cast<double>(v) + o);
      }
    }
    if (v == 0.0f) continue;
    const uint32_t pix = (((slot & s_mask) * kMonoMulInv) & s_mask) * kMonoRows + (slot >> cl.s_log2);   // MonoSlot inverted, as the fold does
    if (pix >= cl.n_pix) continue;
    float* q = cl.xyz + 3u * static_cast<size_t>(pix);
#pragma unroll
    for (uint32_t c = 0; c < 3u; ++c) q[c] = close_add(q[c], cl.coef[c], v);
  }
}
template <bool kFix>
using PlaneOf = typename std::conditional<kFix, unsigned long long, float>::type;
template <bool kFix = false, bool kClose = false>
__global__ void __launch_bounds__(kBinBlock) halo_bin_accumulate_range_kernel(PlaneOf<kFix>* __restrict__ plane, const uint2* __restrict__ list, uint32_t cap,
                                                                               const uint32_t* __restrict__ cnt, uint32_t tile_log2, uint32_t frac_bits,
                                                                               const CloseArgsOf<kClose> cl) {
  static_assert(!(kFix && kClose), "the closing form exists on the float route only");
  __shared__ __attribute__((aligned(16))) unsigned long long acc[1u << kBinTileLog2];   // fixed point (FixQ); tile_log2 <= kBinTileLog2
  const FixQ fq(frac_bits);
  const uint32_t tile = blockIdx.x;
  uint32_t n;
  bool take_twin = false;   // workgroup-uniform, like n
  if constexpr (kClose) {
    n = min(cl.cnt[static_cast<size_t>(tile) * kBinCntStride], cap);
    take_twin = *cl.flag != 0u;
    if (n == 0u && !take_twin) {
      close_done(cl, tile);
      return;
    }
  } else {
    n = min(cnt[static_cast<size_t>(tile) * kBinCntStride], cap);
    if (n == 0u) return;
  }
  const uint32_t slots = 1u << tile_log2, mask = slots - 1u;
  for (uint32_t j = threadIdx.x; j < slots; j += kBinBlock) acc[j] = 0ull;
  __syncthreads();
  const uint2* src = list + static_cast<size_t>(tile) * cap;
#ifndef HALO_ACC_U
#define HALO_ACC_U 4
#endif
  constexpr uint32_t kU = HALO_ACC_U;
  uint32_t i = threadIdx.x;
#ifndef HALO_ACC_NARROW
  // two records per 16-byte load (the lists start on whole 128-byte lines): configs[1]'s pass 164 -> 137 us; eight or sixteen 8-byte loads in
  // flight instead of four gave 152 / 149
  const uint4* src4 = reinterpret_cast<const uint4*>(src);
  const uint32_t n2 = n / 2u;
  auto stream = [&](auto once) {
    for (; i + (kU - 1u) * kBinBlock < n2; i += kU * kBinBlock) {
      uint4 h[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) h[u] = load_list_u4<decltype(once)::value>(&src4[i + u * kBinBlock]);
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        atomicAdd(&acc[h[u].x & mask], fq.fix(__uint_as_float(h[u].y)));
        atomicAdd(&acc[h[u].z & mask], fq.fix(__uint_as_float(h[u].w)));
      }
    }
  };
  if (n >= kListOnceMin) stream(std::true_type{});
  else stream(std::false_type{});
  for (uint32_t r = 2u * i; r < n; r += 2u * kBinBlock) {   // what is left of this thread's pairs, and the odd last record
    for (uint32_t q = r; q < min(r + 2u, n); ++q) {
      const uint2 h = src[q];
      atomicAdd(&acc[h.x & mask], fq.fix(__uint_as_float(h.y)));
    }
  }
  i = n;
#else
  for (; i + (kU - 1u) * kBinBlock < n; i += kU * kBinBlock) {
    uint2 h[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) h[u] = src[i + u * kBinBlock];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) atomicAdd(&acc[h[u].x & mask], fq.fix(__uint_as_float(h[u].y)));
  }
#endif
  for (; i < n; i += kBinBlock) {
    const uint2 h = src[i];
    atomicAdd(&acc[h.x & mask], fq.fix(__uint_as_float(h.y)));
  }
  __syncthreads();
  if constexpr (kClose) {
    close_write_out(acc, fq, tile, tile_log2, slots, take_twin, cl);
    close_done(cl, tile);
  } else if constexpr (kFix) {
    unsigned long long* dst = plane + (static_cast<size_t>(tile) << tile_log2);
    for (uint32_t j = threadIdx.x; j < slots; j += kBinBlock) {
      const unsigned long long v = acc[j];
      if (v != 0ull) atomicAdd(&dst[j], v);
    }
  } else {
  float4* dst = reinterpret_cast<float4*>(plane + (static_cast<size_t>(tile) << tile_log2));
  for (uint32_t j = threadIdx.x; j < slots / 4u; j += kBinBlock) {
    const float4 v = make_float4(fq.unfix(acc[4u * j]), fq.unfix(acc[4u * j + 1u]), fq.unfix(acc[4u * j + 2u]), fq.unfix(acc[4u * j + 3u]));
    if (v.x != 0.0f || v.y != 0.0f || v.z != 0.0f || v.w != 0.0f) {
      float4 q = dst[j];
      q.x += v.x;
      q.y += v.y;
      q.z += v.z;
      q.w += v.w;
      dst[j] = q;
    }
  }
  }
}

// The hit log's per-tile pass.  CH = 1: one scalar plane (discrete wavelength), records {slot, w}, tiles of 16 Ki slots.
// CH = 3: an illuminant session on X, Y, Z planes, records {slot in ONE plane | CMF code << kLogWlShift, w}, tiles of 4 Ki slots:
// the code picks the CMF row (pool entries, then three unit rows for a cached pixel's X, Y, Z records; staged in LDS) and the
// record goes into X, Y and Z tiles with three fp64 LDS adds.  This is where an illuminant session's colour is made: no plane
// per pool entry (31 x 128 tiles at configs[4], a two-level split) and a fold over 3 planes instead of 31.
// Tiles are interleaved over the plane (TileMap) and as many as the split pass can feed (256 / 512), whatever the image size:
// the pass has one workgroup per tile, and a 512 x 256 image cut into 16 Ki-slot tiles would leave it 8 workgroups.  A tile's
// slots are scattered, so its write-out is plain 4-byte read-modify-writes (the workgroup is the only writer of its slots
// while this kernel runs).
// (kFix, the deterministic route's integer twins: as in halo_bin_accumulate_range_kernel.)
template <uint32_t CH, bool kFix = false>
__global__ void __launch_bounds__(kBinBlock) halo_log_accumulate_kernel(PlaneOf<kFix>* __restrict__ planes, uint32_t plane_stride, const uint2* __restrict__ list, uint32_t cap,
                                                                        const uint32_t* __restrict__ cnt, const WlEntryDev* __restrict__ pool, uint32_t pool_size,
                                                                        uint32_t tiles_log2, uint32_t s_log2, uint32_t frac_bits) {
  constexpr uint32_t kTileLog2 = CH == 3u ? 12u : 14u;
  __shared__ __attribute__((aligned(16))) unsigned long long acc[CH][1u << kTileLog2];   // fixed point (FixQ)
  const FixQ fq(frac_bits);
  __shared__ __attribute__((aligned(16))) float s_cmf[CH == 3u ? HALO_WL_POOL_MAX + 3 : 1][4];   // rows of 16 bytes: one LDS read per record
  const uint32_t tile = blockIdx.x;   // plane << tiles_log2 | tile of that plane (CH = 1: the scalar planes of a per-entry-plane session lie back to back)
  const uint32_t n = min(cnt[static_cast<size_t>(tile) * kBinCntStride], cap);
  if (n == 0u) return;
  const TileMap map{s_log2, tiles_log2};
  const uint32_t tile_in = tile & ((1u << tiles_log2) - 1u), plane_of_tile = tile >> tiles_log2, in_plane = (1u << (s_log2 + 10u)) - 1u;
  const uint32_t slots = 1u << (s_log2 + 10u - tiles_log2);   // <= 1 << kTileLog2
  for (uint32_t c = 0; c < CH; ++c)
    for (uint32_t j = threadIdx.x; j < slots; j += kBinBlock) acc[c][j] = 0ull;
  if constexpr (CH == 3u) {
    for (uint32_t j = threadIdx.x; j < pool_size + 3u; j += kBinBlock) {
      const bool unit = j >= pool_size;
      s_cmf[j][0] = unit ? (j == pool_size ? 1.0f : 0.0f) : pool[j].cmf_x;
      s_cmf[j][1] = unit ? (j == pool_size + 1u ? 1.0f : 0.0f) : pool[j].cmf_y;
      s_cmf[j][2] = unit ? (j == pool_size + 2u ? 1.0f : 0.0f) : pool[j].cmf_z;
      s_cmf[j][3] = 0.0f;
    }
  }
  __syncthreads();
  const uint2* src = list + static_cast<size_t>(tile) * cap;
  constexpr uint32_t kU = CH == 3u ? 8u : 4u, kSlotMask = CH == 3u ? (1u << kLogWlShift) - 1u : 0xFFFFFFFFu;
  auto add = [&](uint2 h) {
    uint32_t t_unused, s;
    map.split(h.x & kSlotMask & in_plane, t_unused, s);
    const float w = __uint_as_float(h.y);
    if constexpr (CH == 3u) {
      const uint32_t code = h.x >> kLogWlShift;
      const float4 c4 = *reinterpret_cast<const float4*>(s_cmf[code]);
      if (c4.x != 0.0f) atomicAdd(&acc[0][s], fq.fix(c4.x * w));
      if (c4.y != 0.0f) atomicAdd(&acc[1][s], fq.fix(c4.y * w));
      if (c4.z != 0.0f) atomicAdd(&acc[2][s], fq.fix(c4.z * w));
    } else {
      atomicAdd(&acc[0][s], fq.fix(w));
    }
  };
  // Where the time goes (configs[4], 137 M records, 1.00 ms): without the adds the pass takes 0.27 ms, without the write-out 0.94 — the
  // three fp64 LDS adds per record are 0.67 ms, 41 % of the rate tools/lds_atomic_bench.hip reaches, with the LDS index unit busy 13 % of the
  // time (SQ_LDS_IDX_ACTIVE / SQ_BUSY_CYCLES, profiles/r03_bench4_pmc_lds.txt): a latency chain, not a throughput limit.  One workgroup per
  // CU (96 KB of tiles) is four waves per SIMD, and each record was its own chain: CMF row read from LDS -> wait -> three adds.  So a batch's
  // rows are all requested first, then its adds issued back to back.  (Requesting the next batch's global loads early changes nothing.)
  // (two records per 16-byte load, as in halo_bin_accumulate_range_kernel: the lists start on whole 128-byte lines, and the order in which
  // records reach the fixed-point sums changes nothing)
  const uint4* src4 = reinterpret_cast<const uint4*>(src);
  const uint32_t n2 = n / 2u;
  constexpr uint32_t kU2 = kU / 2u;
  uint32_t i = threadIdx.x;
  auto stream = [&](auto once) {
  for (; i + (kU2 - 1u) * kBinBlock < n2; i += kU2 * kBinBlock) {
    uint2 h[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU2; ++u) {
      const uint4 q = load_list_u4<decltype(once)::value>(&src4[i + u * kBinBlock]);
      h[2u * u] = make_uint2(q.x, q.y);
      h[2u * u + 1u] = make_uint2(q.z, q.w);
    }
    if constexpr (CH == 3u) {
      float4 c4[kU];
      uint32_t sl[kU];
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        uint32_t t_unused;
        map.split(h[u].x & kSlotMask & in_plane, t_unused, sl[u]);
        c4[u] = *reinterpret_cast<const float4*>(s_cmf[h[u].x >> kLogWlShift]);
      }
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        const float w = __uint_as_float(h[u].y);
        if (c4[u].x != 0.0f) atomicAdd(&acc[0][sl[u]], fq.fix(c4[u].x * w));
        if (c4[u].y != 0.0f) atomicAdd(&acc[1][sl[u]], fq.fix(c4[u].y * w));
        if (c4[u].z != 0.0f) atomicAdd(&acc[2][sl[u]], fq.fix(c4[u].z * w));
      }
    } else {
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) add(h[u]);
    }
  }
  };
  if (n >= kListOnceMin) stream(std::true_type{});
  else stream(std::false_type{});
  for (uint32_t r = 2u * i; r < n; r += 2u * kBinBlock) {   // what is left of this thread's pairs, and the odd last record
    add(src[r]);
    if (r + 1u < n) add(src[r + 1u]);
  }
  __syncthreads();
  for (uint32_t c = 0; c < CH; ++c) {
    PlaneOf<kFix>* dst = planes + static_cast<size_t>(c) * plane_stride + (static_cast<size_t>(plane_of_tile) << (s_log2 + 10u));
    for (uint32_t j = threadIdx.x; j < slots; j += kBinBlock) {
      if constexpr (kFix) {
        const unsigned long long v = acc[c][j];
        if (v != 0ull) atomicAdd(&dst[map.slot_of(tile_in, j)], v);
      } else {
      const float v = fq.unfix(acc[c][j]);
      if (v != 0.0f) dst[map.slot_of(tile_in, j)] += v;
      }
    }
  }
}

// (`before_sums`, all three routes below: the per-tile sums end in PLAIN read-modify-writes of the planes, so they may not run beside another
// launch that adds to the same planes; the event, when given, is waited for between the split pass and the sums — see halo_backend.cpp.)
// hit-log route, one scalar plane: regions -> `tiles` (a power of two <= 256) tiles -> the plane.  Contiguous tiles (plain float4
// write-out, 3-5 % faster at configs[1] / [2]) where the lists have room for an uneven image — renders that cull most exits,
// ~1.2 records per ray against room for 8 — interleaved tiles (halo_log_accumulate_kernel) for full-sky renders.
// `planes` > 1: the scalar planes of a per-entry-plane illuminant session (back to back), `tiles` interleaved tiles EACH, planes x tiles <= 512.
hipError_t launch_log_route(float* plane, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2, uint32_t cap2, uint32_t* cnt2,
                            uint32_t tiles, uint32_t planes, uint32_t s_log2, bool interleaved, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, uint32_t copies_log2, hipStream_t stream,
                            hipEvent_t before_sums) {
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles)), tile_log2 = s_log2 + 10u - tiles_log2;   // slots per tile <= 16 Ki
  // more than 256 lists — several planes, or ONE plane of an 8 Mi-pixel image cut into 512 tiles (an illuminant pool of one entry on 4096 x 2048:
  // found by tests/test_gpu_fuzz.py, the 256-list kernel below wrote past its counters) — take the 512-list split kernel
  if (planes > 1u || tiles > 256u) {
    hipLaunchKernelGGL((halo_split_kernel<kLogSplitThreads, kLogSplitPer, 512u, false, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, plane, reinterpret_cast<const uint2*>(log), cap1, cnt1, 1u,
                       1u, reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, 0u, 0xFFFFFFFFu, 0u, s_log2, SplitXyz{nullptr, 0u, 0u, ovf, ovf_flag, s_log2 + 10u, copies_log2});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL((halo_log_accumulate_kernel<1u>), dim3(tiles * planes), dim3(kBinBlock), 0, stream, plane, 0u, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                       static_cast<const WlEntryDev*>(nullptr), 0u, tiles_log2, s_log2, frac_bits);
    return hipGetLastError();
  }
  if (interleaved)
    hipLaunchKernelGGL((halo_split_kernel<kLogSplitThreads, kLogSplitPer, 256u, false, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, plane, reinterpret_cast<const uint2*>(log), cap1, cnt1, 1u,
                       1u, reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, 0u, 0xFFFFFFFFu, 0u, s_log2, SplitXyz{nullptr, 0u, 0u, ovf, ovf_flag, s_log2 + 10u, copies_log2});
  else
    hipLaunchKernelGGL((halo_split_kernel<kLogSplitThreads, kLogSplitPer, 256u, false, false>), dim3(regions), dim3(kLogSplitThreads), 0, stream, plane, reinterpret_cast<const uint2*>(log), cap1, cnt1, 1u,
                       1u, reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, 0u, 0xFFFFFFFFu, tile_log2, 0u, SplitXyz{nullptr, 0u, 0u, ovf, ovf_flag, s_log2 + 10u, copies_log2});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
  if (interleaved)
    hipLaunchKernelGGL((halo_log_accumulate_kernel<1u>), dim3(tiles), dim3(kBinBlock), 0, stream, plane, 0u, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                       static_cast<const WlEntryDev*>(nullptr), 0u, tiles_log2, s_log2, frac_bits);
  else hipLaunchKernelGGL((halo_bin_accumulate_range_kernel<false>), dim3(tiles), dim3(kBinBlock), 0, stream, plane, reinterpret_cast<const uint2*>(list2), cap2, cnt2, tile_log2, frac_bits, CloseArgsOf<false>{});
  return hipGetLastError();
}

// The scalar route's closing form (halo_bin_accumulate_range_kernel<false, true>): regions -> `tiles` CONTIGUOUS tiles -> coef x sum added to the
// XYZ image, for a launch that is its whole session.  The plane is not touched; what the lists cannot hold goes to the twin, which must be there.
// The pass leaves cnt2 zeroed; a 4-byte memset behind it clears the twin's flag.
hipError_t launch_log_route_close(float* xyz, uint32_t n_pix, const float* coef, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                  uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag,
                                  hipStream_t stream, hipEvent_t before_sums) {
  if (tiles == 0u || (tiles & (tiles - 1u)) != 0u || tiles > 256u || xyz == nullptr || coef == nullptr || ovf == nullptr || ovf_flag == nullptr) return hipErrorInvalidValue;
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles));
  if (s_log2 + 10u < tiles_log2 || s_log2 + 10u - tiles_log2 > kBinTileLog2) return hipErrorInvalidValue;
  const uint32_t tile_log2 = s_log2 + 10u - tiles_log2;
  hipLaunchKernelGGL((halo_split_kernel<kLogSplitThreads, kLogSplitPer, 256u, false, false>), dim3(regions), dim3(kLogSplitThreads), 0, stream, static_cast<float*>(nullptr),
                     reinterpret_cast<const uint2*>(log), cap1, cnt1, 1u, 1u, reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, 0u, 0xFFFFFFFFu, tile_log2, 0u,
                     SplitXyz{nullptr, 0u, 0u, ovf, ovf_flag, s_log2 + 10u, 0u});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
  const CloseArgsOf<true> cl{xyz, n_pix, s_log2, {coef[0], coef[1], coef[2]}, cnt2, ovf, ovf_flag};
  hipLaunchKernelGGL((halo_bin_accumulate_range_kernel<false, true>), dim3(tiles), dim3(kBinBlock), 0, stream, static_cast<float*>(nullptr), reinterpret_cast<const uint2*>(list2), cap2,
                     static_cast<const uint32_t*>(nullptr), tile_log2, frac_bits, cl);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipMemsetAsync(ovf_flag, 0, sizeof(uint32_t), stream);   // every workgroup has seen it; the pass zeroed what it took
}

// ---- the closing per-tile pass over per-tile CHUNKS (option "tile_append": a kAccTileFinal trace kernel wrote them, halo_trace.inl log_hit_tile) ----
// One workgroup per tile of 2^tile_log2 consecutive slots, as in the closing form above; the tile's records lie in one chunk per trace workgroup,
// chunk[tile][wg][cap] with cnt[tile][wg] records met (clamped to cap here: what a chunk could not hold went to the twin).  A chunk is short — the
// headline's 781 184 chunks hold 74 - 76 records each, the longest 560 (profiles/resident_grid_traffic.txt; the "~160" this comment used to give was
// wrong) — so ONE WAVE takes a chunk.  A wave holds the counts of kCloseBatch chunks at a time, one per lane, each read ONCE (the pre-pass that asks
// whether the tile is empty keeps what it loaded), and walks the batch in STEPS: kLoads 16-byte loads per lane — 64 x kLoads pairs of records —
// of each of kChunksInFlight chunks, in one of two register sets; the next step's loads are issued before this step's ds_add_u64, so the memory
// system always holds a whole step of the wave while it adds (the form before this one requested 16 chunks, waited, added, and then walked what
// was left of each chunk in a serial loop of load, wait, add).  Two records per 16-byte load (a chunk starts on 16 bytes: cap is even), an odd last
// record in the chunk's last pair, non-temporal — the chunks are read once, a moment after they were written — and the same fixed-point LDS sums,
// whose order does not matter.  The write-out is the closing form's own (close_write_out).  Nothing is reset: the trace kernel writes every count
// of every launch, and the twin's flag is cleared by the memset behind the pass, as above.
// (Measured on configs[1], passes per launch, chunks in flight x loads per lane and chunk, profiles/resident_grid_ab.txt: the form before 246 us;
// 8 x 1 177 [kept: 84 VGPRs, no scratch], 4 x 1 181, 4 x 2 203, 2 x 3 256, 2 x 4 278, 4 x 3 307; 8 x 2 and 16 x 1 need more than the 128 VGPRs a
// 1024-thread workgroup may have and spill, 306 / 313.  On chunks four times as long — a grid of six workgroups per CU — 2 x 4, 2 x 3 and 4 x 2 lead
// at 141 - 144 and 8 x 1 takes 155, but the trace kernel loses 210 us on that grid: blocks_of.  Batches of 16 / 32 / 64 counts: level.)
#ifndef HALO_TILE_CHUNKS   // (the sweep's builds set these; the committed values are the defaults)
#define HALO_TILE_CHUNKS 8
#endif
#ifndef HALO_TILE_LOADS
#define HALO_TILE_LOADS 1
#endif
#ifndef HALO_TILE_BATCH
#define HALO_TILE_BATCH 32
#endif
constexpr uint32_t kChunksInFlight = HALO_TILE_CHUNKS, kLoads = HALO_TILE_LOADS;
constexpr uint32_t kCloseBatch = HALO_TILE_BATCH;   // chunks whose counts one wave holds at a time, one per lane (lanes 0 .. kCloseBatch - 1): 32 spreads a
                                                    // small grid's chunks evenly over the 16 waves (1536 chunks: three batches each, not two or one of 64)
constexpr uint32_t kCloseKeep = 4u;     // batches per wave whose counts stay in registers from the `any` pre-pass on (16 waves x 32 x 4 = 2048 chunks)
static_assert(kCloseBatch % kChunksInFlight == 0u && kCloseBatch <= 64u, "a batch is whole groups of chunks, one count per lane");
__global__ void __launch_bounds__(kBinBlock) halo_tile_close_kernel(const uint2* __restrict__ chunk, uint32_t cap, const uint32_t* __restrict__ cnt, uint32_t wgs,
                                                                    uint32_t tile_log2, uint32_t frac_bits, const CloseArgsOf<true> cl, uint32_t* __restrict__ ticket) {
  __shared__ __attribute__((aligned(16))) unsigned long long acc[1u << kBinTileLog2];   // fixed point (FixQ); tile_log2 <= kBinTileLog2
  // the ticket counters of the trace kernel in front of this pass (wave tickets: nullptr without them) goes back to zero here — no stream operation
  // of its own; the log set's next user waits for this pass (set_free)
  if (ticket != nullptr && blockIdx.x == 0u && threadIdx.x < kTicketGroups) ticket[threadIdx.x * kTicketStride] = 0u;
  const FixQ fq(frac_bits);
  const uint32_t tile = blockIdx.x;
  const uint32_t* tcnt = cnt + static_cast<size_t>(tile) * wgs;
  const bool take_twin = *cl.flag != 0u;   // workgroup-uniform
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  constexpr uint32_t kRound = (kBinBlock / 64u) * kCloseBatch;   // chunks the workgroup's waves take per round: wave w the batch at r x kRound + w x kCloseBatch
  // the count of this lane's chunk in round r, clamped (what a chunk could not hold went to the twin); 0 past the last chunk and on lanes >= kCloseBatch
  auto count_at = [&](uint32_t r) -> uint32_t {
    const uint32_t c = r * kRound + wave * kCloseBatch + lane;
    return (lane < kCloseBatch && c < wgs) ? min(tcnt[c], cap) : 0u;
  };
  // every count is read once: the pre-pass keeps the first kCloseKeep rounds' (a resident grid's all), later rounds are read when their turn comes —
  // a tile of a grid that large is not asked whether it is empty (an empty one adds zeros and writes nothing out)
  const uint32_t rounds = (wgs + kRound - 1u) / kRound;
  uint32_t kept[kCloseKeep], any = rounds > kCloseKeep ? 1u : 0u;
#pragma unroll
  for (uint32_t r = 0; r < kCloseKeep; ++r) any |= kept[r] = count_at(r);
  if (!__syncthreads_or(static_cast<int>(any != 0u)) && !take_twin) return;
  const uint32_t slots = 1u << tile_log2, mask = slots - 1u;
  for (uint32_t j = threadIdx.x; j < slots; j += kBinBlock) acc[j] = 0ull;
  __syncthreads();
  const uint2* tsrc = chunk + static_cast<size_t>(tile) * wgs * cap;
  auto add = [&](uint32_t slot, uint32_t w_bits) { atomicAdd(&acc[slot & mask], fq.fix(__uint_as_float(w_bits))); };
  // One batch: chunks c0 .. c0 + kCloseBatch - 1, their counts in `mine` of lanes 0 .. kCloseBatch - 1.  The unit of work is a STEP: kLoads 16-byte
  // loads per lane (64 x kLoads pairs of records) of each of the kChunksInFlight chunks of one group; a group has as many steps as its longest chunk
  // needs, and the steps of the batch are walked in order, the next step's loads issued before this step's adds (two register sets, taken in turn).
  // An odd last record rides in the chunk's last pair: cap is even, so the 16 bytes are the chunk's own, and its second half is not added.
  auto batch = [&](uint32_t c0, uint32_t mine) {   // wave-uniform c0
    if (__ballot(mine != 0u) == 0ull) return;
    auto count_of = [&](uint32_t j) { return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(mine), static_cast<int>(j))); };
    auto steps_of = [&](uint32_t g) {
      uint32_t most = 0u;
#pragma unroll
      for (uint32_t k = 0; k < kChunksInFlight; ++k) most = max(most, count_of(g + k));
      return (most + 128u * kLoads - 1u) / (128u * kLoads);
    };
    uint32_t g = 0u, it = 0u, steps = 0u;   // the cursor: step `it` of the group at chunk g
    auto seek = [&]() {
      while (g < kCloseBatch && (steps = steps_of(g)) == 0u) g += kChunksInFlight;
      return g < kCloseBatch;
    };
    auto advance = [&]() {
      if (++it < steps) return true;
      it = 0u, g += kChunksInFlight;
      return seek();
    };
    auto issue = [&](uint32_t sg, uint32_t si, uint4 (&h)[kChunksInFlight][kLoads]) {
#pragma unroll
      for (uint32_t k = 0; k < kChunksInFlight; ++k) {
        const uint32_t n = count_of(sg + k);
        const uint4* src4 = reinterpret_cast<const uint4*>(tsrc + static_cast<size_t>(c0 + sg + k) * cap);
#pragma unroll
        for (uint32_t u = 0; u < kLoads; ++u) {
          const uint32_t i = (si * kLoads + u) * 64u + lane;
          if (2u * i < n) h[k][u] = load_list_u4<true>(&src4[i]);
        }
      }
    };
    auto take = [&](uint32_t sg, uint32_t si, const uint4 (&h)[kChunksInFlight][kLoads]) {
#pragma unroll
      for (uint32_t k = 0; k < kChunksInFlight; ++k) {
        const uint32_t n = count_of(sg + k);
#pragma unroll
        for (uint32_t u = 0; u < kLoads; ++u) {
          const uint32_t i = (si * kLoads + u) * 64u + lane;
          if (2u * i < n) add(h[k][u].x, h[k][u].y);
          if (2u * i + 1u < n) add(h[k][u].z, h[k][u].w);
        }
      }
    };
    if (!seek()) return;
    uint4 ha[kChunksInFlight][kLoads], hb[kChunksInFlight][kLoads];
    issue(g, it, ha);
    for (;;) {
      uint32_t tg = g, ti = it;
      bool more = advance();
      if (more) issue(g, it, hb);
      take(tg, ti, ha);
      if (!more) break;
      tg = g, ti = it;
      more = advance();
      if (more) issue(g, it, ha);
      take(tg, ti, hb);
      if (!more) break;
    }
  };
#pragma unroll
  for (uint32_t r = 0; r < kCloseKeep; ++r)
    if (r < rounds) batch(r * kRound + wave * kCloseBatch, kept[r]);
  for (uint32_t r = kCloseKeep; r < rounds; ++r) batch(r * kRound + wave * kCloseBatch, count_at(r));
  __syncthreads();
  close_write_out(acc, fq, tile, tile_log2, slots, take_twin, cl);
}

// The closing form over per-tile chunks: chunk[tiles][wgs][cap] and cnt[tiles][wgs] as a kAccTileFinal trace kernel of `wgs` workgroups left them ->
// coef x sum added to the XYZ image.  No split pass, no tile lists, no counter to reset; the 4-byte memset of the twin's flag behind the pass stays.
hipError_t launch_tile_route_close(float* xyz, uint32_t n_pix, const float* coef, const HitRec* chunk, uint32_t cap, const uint32_t* cnt, uint32_t wgs, uint32_t tiles,
                                   uint32_t s_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, hipStream_t stream, hipEvent_t before_sums, uint32_t* ticket) {
  if (tiles == 0u || (tiles & (tiles - 1u)) != 0u || tiles > kTileAppendMax || wgs == 0u || cap == 0u || (cap & 1u) != 0u) return hipErrorInvalidValue;
  if (xyz == nullptr || coef == nullptr || chunk == nullptr || cnt == nullptr || ovf == nullptr || ovf_flag == nullptr) return hipErrorInvalidValue;
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles));
  if (s_log2 + 10u < tiles_log2 || s_log2 + 10u - tiles_log2 > kBinTileLog2) return hipErrorInvalidValue;
  if (static_cast<uint64_t>(tiles) * wgs * cap > (1ull << 30)) return hipErrorInvalidValue;   // (the trace kernel's 32-bit record index)
  hipError_t e = hipSuccess;
  if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
  const CloseArgsOf<true> cl{xyz, n_pix, s_log2, {coef[0], coef[1], coef[2]}, nullptr, ovf, ovf_flag};
  hipLaunchKernelGGL(halo_tile_close_kernel, dim3(tiles), dim3(kBinBlock), 0, stream, reinterpret_cast<const uint2*>(chunk), cap, cnt, wgs, s_log2 + 10u - tiles_log2, frac_bits, cl, ticket);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return hipMemsetAsync(ovf_flag, 0, sizeof(uint32_t), stream);   // every workgroup has seen it; the pass zeroed what it took
}

// the same for an illuminant session on X, Y, Z planes: `tiles` (a power of two <= 512) interleaved tiles of <= 4 Ki slots of one plane
hipError_t launch_log_route_xyz(float* planes, uint32_t plane_stride, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, const WlEntryDev* pool, uint32_t pool_size, uint32_t frac_bits,
                                double* ovf, uint32_t* ovf_flag, uint32_t copies_log2, hipStream_t stream, hipEvent_t before_sums) {
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles));
  hipLaunchKernelGGL((halo_split_kernel<kLogSplitThreads, kLogSplitPer, 512u, true, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, planes, reinterpret_cast<const uint2*>(log), cap1, cnt1, 1u, 1u,
                     reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, 0u, (1u << kLogWlShift) - 1u, 0u, s_log2, SplitXyz{pool, pool_size, plane_stride, ovf, ovf_flag, s_log2 + 10u, copies_log2});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
  hipLaunchKernelGGL((halo_log_accumulate_kernel<3u>), dim3(tiles), dim3(kBinBlock), 0, stream, planes, plane_stride, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                     pool, pool_size, tiles_log2, s_log2, frac_bits);
  return hipGetLastError();
}

// The deterministic route's log (halo_backend.cpp: a kAccFixedLog trace kernel wrote the regions): the same split — only its full-list fallback
// differs — and the integer twins of the per-tile sums, with the SESSION's F.  Every write to the integer planes is an atomic add of integers, so the
// passes need no ordering against another stream's cache flushes, overflow adds or sums (no `before_sums`), and the planes hold the same integers
// whatever ran when.  One scalar plane, `tiles` (a power of two <= 512) tiles: contiguous ones unless `interleaved`.
hipError_t launch_log_route_fixed(unsigned long long* fix, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2, uint32_t cap2,
                                  uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, bool interleaved, uint32_t frac_bits, hipStream_t stream) {
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles)), tile_log2 = s_log2 + 10u - tiles_log2;   // slots per tile <= 16 Ki
  if (tiles > 512u || tile_log2 > kBinTileLog2) return hipErrorInvalidValue;
  const uint2* l1 = reinterpret_cast<const uint2*>(log);
  uint2* l2 = reinterpret_cast<uint2*>(list2);
  const SplitXyz none{nullptr, 0u, 0u, nullptr, nullptr, 0u, 0u};
  const SplitFix sf{fix, frac_bits};
  const bool mix = interleaved || tiles > 256u;
  if (tiles > 256u)
    hipLaunchKernelGGL((halo_split_fixed_kernel<kLogSplitThreads, kLogSplitPer, 512u, false, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, l1, cap1, cnt1, l2, cap2, cnt2,
                       tiles_log2, 0xFFFFFFFFu, 0u, s_log2, none, sf);
  else if (mix)
    hipLaunchKernelGGL((halo_split_fixed_kernel<kLogSplitThreads, kLogSplitPer, 256u, false, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, l1, cap1, cnt1, l2, cap2, cnt2,
                       tiles_log2, 0xFFFFFFFFu, 0u, s_log2, none, sf);
  else
    hipLaunchKernelGGL((halo_split_fixed_kernel<kLogSplitThreads, kLogSplitPer, 256u, false, false>), dim3(regions), dim3(kLogSplitThreads), 0, stream, l1, cap1, cnt1, l2, cap2, cnt2,
                       tiles_log2, 0xFFFFFFFFu, tile_log2, 0u, none, sf);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (mix)
    hipLaunchKernelGGL((halo_log_accumulate_kernel<1u, true>), dim3(tiles), dim3(kBinBlock), 0, stream, fix, 0u, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                       static_cast<const WlEntryDev*>(nullptr), 0u, tiles_log2, s_log2, frac_bits);
  else hipLaunchKernelGGL((halo_bin_accumulate_range_kernel<true>), dim3(tiles), dim3(kBinBlock), 0, stream, fix, reinterpret_cast<const uint2*>(list2), cap2, cnt2, tile_log2, frac_bits, CloseArgsOf<false>{});
  return hipGetLastError();
}

// ... and for X, Y, Z planes: `tiles` (a power of two <= 512) interleaved tiles of <= 4 Ki slots of one plane
hipError_t launch_log_route_xyz_fixed(unsigned long long* fix, uint32_t plane_stride, const HitRec* log, uint32_t cap1, const uint32_t* cnt1, uint32_t regions, HitRec* list2,
                                      uint32_t cap2, uint32_t* cnt2, uint32_t tiles, uint32_t s_log2, const WlEntryDev* pool, uint32_t pool_size, uint32_t frac_bits,
                                      hipStream_t stream) {
  const uint32_t tiles_log2 = static_cast<uint32_t>(__builtin_ctz(tiles));
  if (tiles > 512u || s_log2 + 10u - tiles_log2 > 12u || pool_size > HALO_WL_POOL_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL((halo_split_fixed_kernel<kLogSplitThreads, kLogSplitPer, 512u, true, true>), dim3(regions), dim3(kLogSplitThreads), 0, stream, reinterpret_cast<const uint2*>(log), cap1, cnt1,
                     reinterpret_cast<uint2*>(list2), cap2, cnt2, tiles_log2, (1u << kLogWlShift) - 1u, 0u, s_log2, SplitXyz{pool, pool_size, plane_stride, nullptr, nullptr, 0u, 0u},
                     SplitFix{fix, frac_bits});
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((halo_log_accumulate_kernel<3u, true>), dim3(tiles), dim3(kBinBlock), 0, stream, fix, plane_stride, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                     pool, pool_size, tiles_log2, s_log2, frac_bits);
  return hipGetLastError();
}

hipError_t launch_bin_two_level(float* plane, const HitRec* list1, uint32_t cap1, uint32_t* cnt1, uint32_t lists1, HitRec* list2, uint32_t cap2,
                                uint32_t* cnt2, uint32_t tiles, uint32_t fan_log2, uint32_t frac_bits, double* ovf, uint32_t* ovf_flag, hipStream_t stream, hipEvent_t before_sums) {
  hipLaunchKernelGGL((halo_split_kernel<256u, 16u, 256u, false, false>), dim3(lists1 * kSplitParts), dim3(256u), 0, stream, plane, reinterpret_cast<const uint2*>(list1), cap1,
                     cnt1, static_cast<uint32_t>(kBinCntStride), kSplitParts, reinterpret_cast<uint2*>(list2), cap2, cnt2, fan_log2, 1u, 0xFFFFFFFFu,
                     static_cast<uint32_t>(kBinTileLog2), 0u, SplitXyz{nullptr, 0u, 0u, ovf, ovf_flag, 0u, 0u});   // (per-entry planes have no privatised copies: the twin's offsets are the planes')
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (before_sums && (e = hipStreamWaitEvent(stream, before_sums, 0)) != hipSuccess) return e;
  hipLaunchKernelGGL((halo_bin_accumulate_range_kernel<false>), dim3(tiles), dim3(kBinBlock), 0, stream, plane, reinterpret_cast<const uint2*>(list2), cap2, cnt2,
                     static_cast<uint32_t>(kBinTileLog2), frac_bits, CloseArgsOf<false>{});
  return hipGetLastError();
}

// xyz[pix] += sum over planes of coef[plane] * (sum over copies of plane[MonoSlot(pix)]); the slots are zeroed — closes a
// session.  Planes: 1 (discrete wavelength, coef = CMF), 3 (X, Y, Z; unit coefs) or one per wavelength-pool entry
// (coef = that entry's CMF), at most kFoldGroup per launch.  Tiled transpose through LDS: a block reads a R-row x
// 64-column tile of every plane copy along the columns (coalesced), then walks it along the rows, where consecutive
// rows are consecutive pixels (coalesced xyz RMW).
// Round 4.  The first form (R = 64 only) ran 436 us on the reference's own benchmark scene (512 x 256, 64 planes): 32 workgroups on
// a 256-CU part, and per thread 16 rows x 64 planes of load -> compare -> store-zero round trips in sequence (the zeroing store may
// alias the next load as far as the compiler knows, so nothing overlapped).  Now (1) the tile height R is 64, 16 or 4 rows, whichever
// gives the launch >= 512 workgroups (the write runs stay >= 48 bytes, and an image that small is cache-resident anyway), and (2) a
// thread requests kFoldBatch plane values before it looks at any of them or zeroes anything.
constexpr uint32_t kFoldTile = 64u;
constexpr uint32_t kFoldBatch = 8u;
// The second half of a fold: the workgroup's R-row x 64-column tile of X, Y, Z sums, walked along the rows — consecutive rows are consecutive
// pixels — and added to the image.
template <uint32_t R>
__device__ __forceinline__ void fold_store_tile(const float (&tile)[3][R][kFoldTile + 1], float* __restrict__ xyz, uint32_t n_pix, uint32_t s_log2, uint32_t row0, uint32_t col0) {
  const uint32_t s_mask = (1u << s_log2) - 1u;
  const uint32_t wr = threadIdx.x % R;   // row of the tile = consecutive pixels
  for (uint32_t c = threadIdx.x / R; c < kFoldTile; c += kBlock / R) {
    const float x = tile[0][wr][c], y = tile[1][wr][c], z = tile[2][wr][c];
    if (x == 0.0f && y == 0.0f && z == 0.0f) continue;
    const uint32_t a = ((col0 + c) * kMonoMulInv) & s_mask;   // column hash inverted
    const uint32_t pix = a * kMonoRows + row0 + wr;
    if (pix < n_pix) {
      xyz[3u * pix + 0u] += x;
      xyz[3u * pix + 1u] += y;
      xyz[3u * pix + 2u] += z;
    }
  }
}
template <uint32_t R>
__global__ void __launch_bounds__(kBlock) halo_fold_kernel(float* __restrict__ xyz, float* __restrict__ planes, uint32_t n_pix,
                                                            uint32_t s_log2, uint32_t copies, uint32_t n_planes, const FoldCoef coef,
                                                            double* __restrict__ ovf, const uint32_t* __restrict__ ovf_flag) {
  __shared__ float tile[3][R][kFoldTile + 1];
  // the planes' fp64 twin (copy 0: what log regions and tile lists could not hold, DispatchParams::ovf) comes in only when something was written
  // to it — one uniform load — and `ovf` already points at this group's first plane
  const bool take_ovf = ovf != nullptr && *ovf_flag != 0u;
  const uint32_t tiles_c = (1u << s_log2) / kFoldTile;  // columns per row / tile width (s_log2 >= 6)
  const uint32_t row0 = (blockIdx.x / tiles_c) * R, col0 = (blockIdx.x % tiles_c) * kFoldTile;
  const size_t plane = static_cast<size_t>(kMonoRows) << s_log2;
  const uint32_t lo = threadIdx.x & (kFoldTile - 1u), hi = threadIdx.x / kFoldTile;  // hi in [0, 4)
  for (uint32_t r = hi; r < R; r += kBlock / kFoldTile) {
    float* q = planes + (static_cast<size_t>(row0 + r) << s_log2) + col0 + lo;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (copies == 1u) {   // per-entry planes, or a session whose launches all went through the hit log: batches of planes
      for (uint32_t p0 = 0; p0 < n_planes; p0 += kFoldBatch) {
        float t[kFoldBatch];
#pragma unroll
        for (uint32_t u = 0; u < kFoldBatch; ++u) t[u] = p0 + u < n_planes ? q[static_cast<size_t>(p0 + u) * plane] : 0.0f;
        if (take_ovf) {
          double* qo = ovf + (q - planes);
#pragma unroll
          for (uint32_t u = 0; u < kFoldBatch; ++u) {
            if (p0 + u >= n_planes) continue;
            const double o = qo[static_cast<size_t>(p0 + u) * plane];
            if (o != 0.0) {
              qo[static_cast<size_t>(p0 + u) * plane] = 0.0;
              const float sum = static_cast<float>(static_cast<double>(t[u]) + o);
              t[u] = sum;
            }
          }
        }
#pragma unroll
        for (uint32_t u = 0; u < kFoldBatch; ++u) {
          if (t[u] == 0.0f) continue;
          q[static_cast<size_t>(p0 + u) * plane] = 0.0f;
          x += coef.c[p0 + u][0] * t[u];
          y += coef.c[p0 + u][1] * t[u];
          z += coef.c[p0 + u][2] * t[u];
        }
      }
    } else {              // privatised copies of few planes: batches of copies, the plane's coefficient applied to their sum
      for (uint32_t pl = 0; pl < n_planes; ++pl) {
        float v = 0.0f;
        float* qp = q + static_cast<size_t>(pl) * copies * plane;
        for (uint32_t c0 = 0; c0 < copies; c0 += kFoldBatch) {
          float t[kFoldBatch];
#pragma unroll
          for (uint32_t u = 0; u < kFoldBatch; ++u) t[u] = c0 + u < copies ? qp[static_cast<size_t>(c0 + u) * plane] : 0.0f;
#pragma unroll
          for (uint32_t u = 0; u < kFoldBatch; ++u) {
            if (t[u] == 0.0f) continue;
            qp[static_cast<size_t>(c0 + u) * plane] = 0.0f;
            v += t[u];
          }
        }
        if (take_ovf) {   // the twin shadows copy 0
          double* qo = ovf + (q - planes) + static_cast<size_t>(pl) * plane;   // the twin has no copies: plane pl's twin starts at pl * plane
          const double o = *qo;
          if (o != 0.0) {
            *qo = 0.0;
            v = static_cast<float>(static_cast<double>(v) + o);
          }
        }
        x += coef.c[pl][0] * v;
        y += coef.c[pl][1] * v;
        z += coef.c[pl][2] * v;
      }
    }
    tile[0][r][lo] = x;
    tile[1][r][lo] = y;
    tile[2][r][lo] = z;
  }
  __syncthreads();
  fold_store_tile<R>(tile, xyz, n_pix, s_log2, row0, col0);
}

// The same fold over the 64-bit fixed-point planes of a deterministic session (DispatchParams::fix: [plane][slot], one copy, no twin): a slot's
// value is float(double(S) * 2^-F), exact in the integer and rounded once; coefficients, the add to XYZ and the zeroing of what was read are
// the float fold's.  One or three planes (a discrete wavelength's scalar plane, or X, Y, Z).
constexpr uint32_t kFixPlanesMax = 3u;
template <uint32_t R>
__global__ void __launch_bounds__(kBlock) halo_fold_fixed_kernel(float* __restrict__ xyz, unsigned long long* __restrict__ planes, uint32_t n_pix,
                                                                  uint32_t s_log2, uint32_t n_planes, const FoldCoef coef, uint32_t frac_bits) {
  __shared__ float tile[3][R][kFoldTile + 1];
  const FixQ fq(frac_bits);
  const uint32_t tiles_c = (1u << s_log2) / kFoldTile;
  const uint32_t row0 = (blockIdx.x / tiles_c) * R, col0 = (blockIdx.x % tiles_c) * kFoldTile;
  const size_t plane = static_cast<size_t>(kMonoRows) << s_log2;
  const uint32_t lo = threadIdx.x & (kFoldTile - 1u), hi = threadIdx.x / kFoldTile;
  for (uint32_t r = hi; r < R; r += kBlock / kFoldTile) {
    unsigned long long* q = planes + (static_cast<size_t>(row0 + r) << s_log2) + col0 + lo;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    unsigned long long t[kFixPlanesMax];
#pragma unroll
    for (uint32_t u = 0; u < kFixPlanesMax; ++u) t[u] = u < n_planes ? q[static_cast<size_t>(u) * plane] : 0ull;
#pragma unroll
    for (uint32_t u = 0; u < kFixPlanesMax; ++u) {
      if (t[u] == 0ull) continue;
      q[static_cast<size_t>(u) * plane] = 0ull;
      const float v = fq.unfix(t[u]);
      x += coef.c[u][0] * v;
      y += coef.c[u][1] * v;
      z += coef.c[u][2] * v;
    }
    tile[0][r][lo] = x;
    tile[1][r][lo] = y;
    tile[2][r][lo] = z;
  }
  __syncthreads();
  fold_store_tile<R>(tile, xyz, n_pix, s_log2, row0, col0);
}

// Moving the fixed-point planes between handles (halo_export_fixed / halo_import_fixed): `words` is pixel order, plane p at [p * n_pix, (p + 1) * n_pix);
// the planes lie [plane][MonoSlot(pix)].  A thread takes V consecutive words (V = 2: one 16-byte access on the pixel-order side, when `words` is
// 16-byte aligned), so that side is coalesced; the plane side is a gather / scatter of 8-byte words through the slot hash — consecutive pixels are a
// plane row apart, by design (halo_device.h MonoSlot).  Grid-stride; word indices are 64-bit (3 planes of 2^25 pixels stay below 2^32, the products do not).
template <uint32_t V>
__global__ void __launch_bounds__(kBlock) halo_export_fixed_kernel(unsigned long long* __restrict__ planes, unsigned long long* __restrict__ words, uint32_t n_pix,
                                                                    uint32_t s_log2, uint32_t n_planes, unsigned long long landed) {
  const uint64_t total = static_cast<uint64_t>(n_pix) * n_planes;
  const size_t plane = static_cast<size_t>(kMonoRows) << s_log2;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock * V;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) * V; i < total; i += stride) {
    unsigned long long v[V];
#pragma unroll
    for (uint32_t u = 0; u < V; ++u) {
      v[u] = 0ull;
      if (i + u < total) {
        const uint32_t pl = static_cast<uint32_t>((i + u) / n_pix), pix = static_cast<uint32_t>((i + u) - static_cast<uint64_t>(pl) * n_pix);
        unsigned long long* q = planes + static_cast<size_t>(pl) * plane + MonoSlot(pix, s_log2);
        v[u] = *q;
        if (v[u] != 0ull) *q = 0ull;   // moved out: the planes are all-zero afterwards, as after a fold
      }
    }
    if (V == 2u && i + 1u < total) {
      *reinterpret_cast<ulonglong2*>(words + i) = make_ulonglong2(v[0], v[V - 1u]);
    } else {
#pragma unroll
      for (uint32_t u = 0; u < V; ++u)
        if (i + u < total) words[i + u] = v[u];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) words[total] = landed;   // the landed integer nobody has taken yet, behind the planes
}
// ... and back in: planes[plane][MonoSlot(pix)] += words[plane * n_pix + pix], modulo 2^64.  Plain read-modify-writes: every slot has one word, and
// the launch is ordered behind everything that adds to the planes (halo_import_fixed).
template <uint32_t V>
__global__ void __launch_bounds__(kBlock) halo_import_fixed_kernel(unsigned long long* __restrict__ planes, const unsigned long long* __restrict__ words, uint32_t n_pix,
                                                                    uint32_t s_log2, uint32_t n_planes) {
  const uint64_t total = static_cast<uint64_t>(n_pix) * n_planes;
  const size_t plane = static_cast<size_t>(kMonoRows) << s_log2;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock * V;
  for (uint64_t i = (static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x) * V; i < total; i += stride) {
    unsigned long long v[V];
    if (V == 2u && i + 1u < total) {
      const ulonglong2 t = *reinterpret_cast<const ulonglong2*>(words + i);
      v[0] = t.x, v[V - 1u] = t.y;
    } else {
#pragma unroll
      for (uint32_t u = 0; u < V; ++u) v[u] = i + u < total ? words[i + u] : 0ull;
    }
#pragma unroll
    for (uint32_t u = 0; u < V; ++u) {
      if (v[u] == 0ull) continue;   // (also every word past the end)
      const uint32_t pl = static_cast<uint32_t>((i + u) / n_pix), pix = static_cast<uint32_t>((i + u) - static_cast<uint64_t>(pl) * n_pix);
      planes[static_cast<size_t>(pl) * plane + MonoSlot(pix, s_log2)] += v[u];
    }
  }
}

// Consumer fold: running image += drained accumulator, Neumaier-compensated (accum_shared.h:70-74), accumulator zeroed.
__global__ void __launch_bounds__(kBlock) halo_consumer_fold_kernel(float* __restrict__ acc, float* __restrict__ sum,
                                                                     float* __restrict__ comp, uint32_t n) {
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const float delta = acc[i];
    if (delta == 0.0f) continue;
    acc[i] = 0.0f;
    const float s = sum[i];
    const float ns = s + delta;
    comp[i] += (fabsf(delta) < fabsf(s)) ? ((s - ns) + delta) : ((delta - ns) + s);
    sum[i] = ns;
  }
}

// PostSnapshot (render.cpp:508-578): the per-pixel display transform (halo_display.h display_pixel) of the snapshot.  Also writes the raw
// snapshot (sum + comp) when xyz_out is set.
__global__ void __launch_bounds__(kBlock) halo_post_snapshot_kernel(const float* __restrict__ sum, const float* __restrict__ comp,
                                                                     uint8_t* __restrict__ rgb_out, float* __restrict__ xyz_out,
                                                                     uint32_t n_pix, DisplayDev dsp) {
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_pix; i += stride) {
    float raw[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      raw[j] = sum[3u * i + j] + comp[3u * i + j];
      if (xyz_out) xyz_out[3u * i + j] = raw[j];
    }
    if (rgb_out == nullptr) continue;
    uint8_t px[3];
    display_pixel(raw, dsp, px);
#pragma unroll
    for (int j = 0; j < 3; j++) rgb_out[3u * i + j] = px[j];
  }
}

// ---- display-side composite of the raypath-colour class lanes (server/component_compositor.cpp) --------------------------------
// The lanes are fp64 on the device and are handed out as floats (halo_readback_class_lanes); the composite reads them the same way.

// One pass of the radix select behind ComputeParticipatingP99Y (component_compositor.cpp:138-163): a histogram of `bits` bits at `shift`
// of the float bit patterns of the positive lane values whose higher bits equal `prefix` (positive floats order like their patterns).
// shift + bits == 32 on the first pass (no prefix).
__global__ void __launch_bounds__(kBlock) halo_lane_hist_kernel(const double* __restrict__ lanes, uint32_t n_pix, CompositeDev cd, uint32_t shift, uint32_t bits,
                                                                 uint32_t prefix, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[2048];
  const uint32_t nb = 1u << bits;
  for (uint32_t i = threadIdx.x; i < nb; i += kBlock) h[i] = 0u;
  __syncthreads();
  const uint64_t total = static_cast<uint64_t>(n_pix) * cd.n_active;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  const uint32_t hi = shift + bits;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < total; i += stride) {
    const uint32_t k = static_cast<uint32_t>(i / n_pix), p = static_cast<uint32_t>(i - static_cast<uint64_t>(k) * n_pix);
    const float v = static_cast<float>(lanes[static_cast<size_t>(cd.lane[k]) * n_pix + p]);
    if (!(v > 0.0f)) continue;
    const uint32_t u = __float_as_uint(v);
    if (hi < 32u && (u >> hi) != prefix) continue;
    atomicAdd(&h[(u >> shift) & (nb - 1u)], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < nb; i += kBlock)
    if (h[i]) atomicAdd(&hist[i], h[i]);
}

// CompositeDominantPixel / CompositeAdditivePixel / CompositePainterPixel (component_compositor.cpp:56-114) + the painter's post-multiply and
// clamp (:268-274) + LinearRgbToSrgbU8 (:292-300).  Every product and sum is rounded on its own (mul_rn / add_rn: the backend fuses plain a * b + c whatever the source says), like the
// reference's host build.
__global__ void __launch_bounds__(kBlock) halo_composite_kernel(const double* __restrict__ lanes, uint32_t n_pix, CompositeDev cd, float* __restrict__ rgb_out,
                                                                 uint8_t* __restrict__ srgb_out) {
  const uint32_t stride = gridDim.x * kBlock;
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < n_pix; p += stride) {
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (cd.mode == HALO_COMPOSITE_DOMINANT) {
      int best = -1;
      float best_ey = 0.0f;
      for (uint32_t k = 0; k < cd.n_active; k++) {
        const float ey = mul_rn(static_cast<float>(lanes[static_cast<size_t>(cd.lane[k]) * n_pix + p]), cd.s);
        if (ey > best_ey) {
          best_ey = ey;
          best = static_cast<int>(k);
        }
      }
      if (best >= 0)
        for (int j = 0; j < 3; j++) out[j] = mul_rn(cd.color[best][j], best_ey);
    } else if (cd.mode == HALO_COMPOSITE_ADDITIVE) {
      for (uint32_t k = 0; k < cd.n_active; k++) {
        const float ey = mul_rn(static_cast<float>(lanes[static_cast<size_t>(cd.lane[k]) * n_pix + p]), cd.s);
        if (!(ey > 0.0f)) continue;
        for (int j = 0; j < 3; j++) out[j] = add_rn(out[j], mul_rn(cd.color[k][j], ey));
      }
      for (int j = 0; j < 3; j++) out[j] = fminf(fmaxf(out[j], 0.0f), 1.0f);
    } else {
      float T = 1.0f;
      for (uint32_t k = 0; k < cd.n_active && T > 0.0f; k++) {
        const float alpha = fminf(mul_rn(static_cast<float>(lanes[static_cast<size_t>(cd.lane[k]) * n_pix + p]), cd.a), 1.0f);
        if (!(alpha > 0.0f)) continue;
        const float ta = mul_rn(T, alpha);
        for (int j = 0; j < 3; j++) out[j] = add_rn(out[j], mul_rn(ta, cd.color[k][j]));
        T = mul_rn(T, add_rn(1.0f, -alpha));
      }
      for (int j = 0; j < 3; j++) out[j] = fminf(fmaxf(mul_rn(out[j], cd.display), 0.0f), 1.0f);
    }
    if (rgb_out)
      for (int j = 0; j < 3; j++) rgb_out[3u * p + j] = out[j];
    if (srgb_out)
      for (int j = 0; j < 3; j++) {
        const float v = fminf(fmaxf(out[j], 0.0f), 1.0f);
        const float g = (v < 0.0031308f) ? mul_rn(v, 12.92f) : add_rn(mul_rn(1.055f, powf(v, 1.0f / 2.4f)), -0.055f);   // LinearToSrgb color_space.cpp:47-52
        srgb_out[3u * p + j] = static_cast<uint8_t>(mul_rn(g, 255.0f));
      }
  }
}

__global__ void __launch_bounds__(kBlock) halo_lanes_load_kernel(const float* __restrict__ src, double* __restrict__ lanes, uint64_t n) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) lanes[i] = static_cast<double>(src[i]);
}

// ConsumeDeviceFused's lane half: lanes drained elsewhere are ADDED (render.cpp:176-185)
__global__ void __launch_bounds__(kBlock) halo_lanes_add_kernel(const float* __restrict__ src, double* __restrict__ lanes, uint64_t n) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) lanes[i] += static_cast<double>(src[i]);
}
// the inverse at the seam (TraceBackend::ReadbackClassLanes hands out floats and drains the device lanes): narrow into the staging buffer, zero the lane
__global__ void __launch_bounds__(kBlock) halo_lanes_drain_kernel(double* __restrict__ lanes, float* __restrict__ dst, uint64_t n) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlock;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x; i < n; i += stride) {
    dst[i] = static_cast<float>(lanes[i]);
    lanes[i] = 0.0;
  }
}

hipError_t launch_lane_hist(const double* lanes, uint32_t n_pix, const CompositeDev& cd, uint32_t shift, uint32_t bits, uint32_t prefix, uint32_t* hist, int blocks,
                            hipStream_t stream) {
  hipLaunchKernelGGL(halo_lane_hist_kernel, dim3(blocks), dim3(kBlock), 0, stream, lanes, n_pix, cd, shift, bits, prefix, hist);
  return hipGetLastError();
}
hipError_t launch_composite(const double* lanes, uint32_t n_pix, const CompositeDev& cd, float* rgb_out, uint8_t* srgb_out, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(halo_composite_kernel, dim3(blocks), dim3(kBlock), 0, stream, lanes, n_pix, cd, rgb_out, srgb_out);
  return hipGetLastError();
}
hipError_t launch_lanes_load(const float* src, double* lanes, uint64_t n, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(halo_lanes_load_kernel, dim3(blocks), dim3(kBlock), 0, stream, src, lanes, n);
  return hipGetLastError();
}

hipError_t launch_lanes_add(const float* src, double* lanes, uint64_t n, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(halo_lanes_add_kernel, dim3(blocks), dim3(kBlock), 0, stream, src, lanes, n);
  return hipGetLastError();
}
hipError_t launch_lanes_drain(double* lanes, float* dst, uint64_t n, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(halo_lanes_drain_kernel, dim3(blocks), dim3(kBlock), 0, stream, lanes, dst, n);
  return hipGetLastError();
}

hipError_t launch_consumer_fold(float* acc, float* sum, float* comp, uint32_t n, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL(halo_consumer_fold_kernel, dim3(blocks), dim3(kBlock), 0, stream, acc, sum, comp, n);
  return hipGetLastError();
}

hipError_t launch_post_snapshot(const float* sum, const float* comp, uint8_t* rgb_out, float* xyz_out, uint32_t n_pix, float scale,
                                const float ray_color[3], const float background[3], int blocks, hipStream_t stream) {
  DisplayDev d;
  d.scale = scale;
  for (int j = 0; j < 3; j++) {
    d.ray_color[j] = ray_color[j];
    d.background[j] = background[j];
  }
  hipLaunchKernelGGL(halo_post_snapshot_kernel, dim3(blocks), dim3(kBlock), 0, stream, sum, comp, rgb_out, xyz_out, n_pix, d);
  return hipGetLastError();
}

// `planes` points at the first plane of this group; coef holds n_planes (<= kFoldGroup) coefficient triples
hipError_t launch_fold(float* xyz, float* planes, uint32_t n_pix, uint32_t s_log2, uint32_t copies, uint32_t n_planes, const FoldCoef& coef,
                       double* ovf, const uint32_t* ovf_flag, hipStream_t stream) {
  const uint32_t tiles_c = (1u << s_log2) / kFoldTile;
  if (tiles_c * (kMonoRows / 64u) >= 512u)
    hipLaunchKernelGGL(halo_fold_kernel<64u>, dim3(tiles_c * (kMonoRows / 64u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, copies, n_planes, coef, ovf, ovf_flag);
  else if (tiles_c * (kMonoRows / 16u) >= 512u)
    hipLaunchKernelGGL(halo_fold_kernel<16u>, dim3(tiles_c * (kMonoRows / 16u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, copies, n_planes, coef, ovf, ovf_flag);
  else
    hipLaunchKernelGGL(halo_fold_kernel<4u>, dim3(tiles_c * (kMonoRows / 4u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, copies, n_planes, coef, ovf, ovf_flag);
  return hipGetLastError();
}

hipError_t launch_fold_fixed(float* xyz, unsigned long long* planes, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, const FoldCoef& coef, uint32_t frac_bits,
                             hipStream_t stream) {
  if (n_planes > kFixPlanesMax) return hipErrorInvalidValue;
  const uint32_t tiles_c = (1u << s_log2) / kFoldTile;
  if (tiles_c * (kMonoRows / 64u) >= 512u)
    hipLaunchKernelGGL(halo_fold_fixed_kernel<64u>, dim3(tiles_c * (kMonoRows / 64u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, n_planes, coef, frac_bits);
  else if (tiles_c * (kMonoRows / 16u) >= 512u)
    hipLaunchKernelGGL(halo_fold_fixed_kernel<16u>, dim3(tiles_c * (kMonoRows / 16u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, n_planes, coef, frac_bits);
  else
    hipLaunchKernelGGL(halo_fold_fixed_kernel<4u>, dim3(tiles_c * (kMonoRows / 4u)), dim3(kBlock), 0, stream, xyz, planes, n_pix, s_log2, n_planes, coef, frac_bits);
  return hipGetLastError();
}

// (memory-bound copies: one workgroup per kBlock * V words up to eight per CU, the rest by the grid stride)
static uint32_t fixed_copy_blocks(uint64_t total, uint32_t v) {
  const uint64_t want = (total + static_cast<uint64_t>(kBlock) * v - 1u) / (static_cast<uint64_t>(kBlock) * v);
  return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(want, 1u), 2048u));
}
hipError_t launch_export_fixed(unsigned long long* planes, unsigned long long* words, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, unsigned long long landed,
                               hipStream_t stream) {
  if (n_planes == 0u || n_planes > kFixPlanesMax || n_pix == 0u || (static_cast<uint64_t>(kMonoRows) << s_log2) < n_pix) return hipErrorInvalidValue;
  const uint64_t total = static_cast<uint64_t>(n_pix) * n_planes;
  if ((reinterpret_cast<uintptr_t>(words) & 15u) == 0u)
    hipLaunchKernelGGL(halo_export_fixed_kernel<2u>, dim3(fixed_copy_blocks(total, 2u)), dim3(kBlock), 0, stream, planes, words, n_pix, s_log2, n_planes, landed);
  else
    hipLaunchKernelGGL(halo_export_fixed_kernel<1u>, dim3(fixed_copy_blocks(total, 1u)), dim3(kBlock), 0, stream, planes, words, n_pix, s_log2, n_planes, landed);
  return hipGetLastError();
}
hipError_t launch_import_fixed(unsigned long long* planes, const unsigned long long* words, uint32_t n_pix, uint32_t s_log2, uint32_t n_planes, hipStream_t stream) {
  if (n_planes == 0u || n_planes > kFixPlanesMax || n_pix == 0u || (static_cast<uint64_t>(kMonoRows) << s_log2) < n_pix) return hipErrorInvalidValue;
  const uint64_t total = static_cast<uint64_t>(n_pix) * n_planes;
  if ((reinterpret_cast<uintptr_t>(words) & 15u) == 0u)
    hipLaunchKernelGGL(halo_import_fixed_kernel<2u>, dim3(fixed_copy_blocks(total, 2u)), dim3(kBlock), 0, stream, planes, words, n_pix, s_log2, n_planes);
  else
    hipLaunchKernelGGL(halo_import_fixed_kernel<1u>, dim3(fixed_copy_blocks(total, 1u)), dim3(kBlock), 0, stream, planes, words, n_pix, s_log2, n_planes);
  return hipGetLastError();
}

// ---- canonical continuation order (option cont_order = 1) ----------------------------------------------------------------------------
// A layer before the last appends its continuations wherever its waves' atomics land (sharded pool, see kContShards); with the option on each
// record also carries (root, seq) and every root a 128-bit mask of the seqs that continued.  Recombine then sorts the pool into (root, seq)
// order — the order a one-thread run of the oracle builds — in O(roots + records): an exclusive scan of the masks' popcounts over the roots
// (reduce, scan of the tile sums, downsweep) gives each root its first slot, and a record's slot is that plus the number of its root's bits
// below its own.  Roots are in tiles of kScanTile, eight consecutive roots per thread.  Whatever breaks the invariant — a key outside the
// layer, a slot outside the pool, popcounts that do not add up to the pool's fill (a seq continued twice loses a bit) — sets a bit of the error
// word (kContErr*), which Recombine reads behind the scatter and turns into HALO_FATAL: a pool with holes is never traced.
constexpr uint32_t kScanBlock = 256u, kScanItems = 8u, kScanTile = kScanBlock * kScanItems;

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
  const uint32_t lane = __lane_id();
#pragma unroll
  for (uint32_t d = 1u; d < 64u; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}
// exclusive prefix of v over the workgroup (kScanBlock threads); `total` is the workgroup's sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t& total) {
  __shared__ uint32_t s_wave[kScanBlock / 64u];
  const uint32_t inc = wave_inclusive_scan(v);
  const uint32_t w = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) s_wave[w] = inc;
  __syncthreads();
  uint32_t before = 0u;
  total = 0u;
#pragma unroll
  for (uint32_t k = 0; k < kScanBlock / 64u; k++) {
    const uint32_t s = s_wave[k];
    before += (k < w) ? s : 0u;
    total += s;
  }
  __syncthreads();   // (s_wave is reused by the next call)
  return before + inc - v;
}
// a root's 128-bit mask as two 64-bit halves (kContMaskWords = 4 words)
struct Mask128 {
  unsigned long long lo, hi;
};
__device__ __forceinline__ Mask128 load_mask(const unsigned long long* __restrict__ mask, uint64_t r) { return Mask128{mask[2u * r], mask[2u * r + 1u]}; }
__device__ __forceinline__ uint32_t mask_count(Mask128 m) { return static_cast<uint32_t>(__popcll(m.lo) + __popcll(m.hi)); }
__device__ __forceinline__ uint32_t mask_below(Mask128 m, uint32_t seq) {   // bits of m below bit `seq` (< 128)
  return seq < 64u ? static_cast<uint32_t>(__popcll(m.lo & ((1ull << seq) - 1ull)))
                   : static_cast<uint32_t>(__popcll(m.lo) + __popcll(m.hi & ((1ull << (seq - 64u)) - 1ull)));
}
// the popcounts of one thread's eight masks (roots past n count 0)
__device__ __forceinline__ void tile_counts(const unsigned long long* __restrict__ mask, uint32_t n, uint32_t c[kScanItems]) {
  const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScanTile + static_cast<uint64_t>(threadIdx.x) * kScanItems;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; k++) c[k] = (r0 + k < n) ? mask_count(load_mask(mask, r0 + k)) : 0u;
}

__global__ void __launch_bounds__(kScanBlock) halo_cont_count_kernel(const unsigned long long* __restrict__ mask, uint32_t n, uint32_t* __restrict__ tile_sum) {
  uint32_t c[kScanItems];
  tile_counts(mask, n, c);
  uint32_t v = 0u;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; k++) v += c[k];
  uint32_t total;
  (void)block_exclusive_scan(v, total);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: the tile sums, exclusively scanned in place (kScanTile of them per pass, a carry between passes); the grand total must be the
// pool's fill, n_cont
__global__ void __launch_bounds__(kScanBlock) halo_cont_tiles_scan_kernel(uint32_t* __restrict__ tile_sum, uint32_t tiles, uint32_t n_cont, uint32_t* __restrict__ err) {
  uint64_t carry = 0u;
  for (uint32_t t0 = 0u; t0 < tiles; t0 += kScanTile) {
    const uint32_t i0 = t0 + threadIdx.x * kScanItems;
    uint32_t c[kScanItems], v = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; k++) {
      c[k] = (i0 + k < tiles) ? tile_sum[i0 + k] : 0u;
      v += c[k];
    }
    uint32_t total;
    uint32_t run = static_cast<uint32_t>(carry) + block_exclusive_scan(v, total);
#pragma unroll
    for (uint32_t k = 0; k < kScanItems; k++) {
      if (i0 + k < tiles) tile_sum[i0 + k] = run;
      run += c[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0 && carry != n_cont) atomicOr(err, kContErrSum);
}

__global__ void __launch_bounds__(kScanBlock) halo_cont_base_kernel(const unsigned long long* __restrict__ mask, uint32_t n, const uint32_t* __restrict__ tile_off,
                                                                    uint32_t* __restrict__ base) {
  uint32_t c[kScanItems];
  tile_counts(mask, n, c);
  uint32_t v = 0u;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; k++) v += c[k];
  uint32_t total;
  uint32_t run = tile_off[blockIdx.x] + block_exclusive_scan(v, total);
  const uint64_t r0 = static_cast<uint64_t>(blockIdx.x) * kScanTile + static_cast<uint64_t>(threadIdx.x) * kScanItems;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; k++) {
    if (r0 + k < n) base[r0 + k] = run;
    run += c[k];
  }
}

// every record of the sharded pool (shard blockIdx.y, its fill count from the trace kernels' own counter) to its canonical slot, all planes
__global__ void __launch_bounds__(kBlock) halo_cont_scatter_kernel(const uint32_t* __restrict__ in, uint32_t in_stride, uint32_t region, const uint32_t* __restrict__ cnt,
                                                                   const unsigned long long* __restrict__ mask, const uint32_t* __restrict__ base, uint32_t n_roots,
                                                                   uint32_t* __restrict__ out, uint32_t out_stride, uint32_t n_cont, uint32_t planes,
                                                                   uint32_t* __restrict__ err) {
  const uint32_t shard = blockIdx.y;
  const uint32_t fill = min(cnt[shard * kContCntStride], region);
  for (uint32_t off = blockIdx.x * kBlock + threadIdx.x; off < fill; off += gridDim.x * kBlock) {
    const uint32_t src = shard * region + off;
    const uint32_t root = in[kContPlaneRoot * in_stride + src], seq = in[kContPlaneSeq * in_stride + src];
    const Mask128 m = (root < n_roots) ? load_mask(mask, root) : Mask128{0ull, 0ull};
    const bool known = root < n_roots && seq < 32u * kContMaskWords && ((seq < 64u ? (m.lo >> seq) : (m.hi >> (seq - 64u))) & 1ull) != 0ull;
    const uint32_t dst = known ? base[root] + mask_below(m, seq) : n_cont;
    if (dst >= n_cont) {   // (cannot happen while the append and the scan hold their invariants — and if it does, the layer is refused)
      atomicOr(err, kContErrKey);
      continue;
    }
    for (uint32_t p = 0; p < planes; p++) out[p * out_stride + dst] = in[p * in_stride + src];
  }
}

hipError_t launch_cont_reorder(const float* in, uint32_t in_stride, uint32_t region, const uint32_t* cnt, uint32_t max_fill, const uint32_t* mask, uint32_t n_roots,
                               uint32_t* tile_sum, uint32_t* base, float* out, uint32_t out_stride, uint32_t n_cont, uint32_t planes, uint32_t* err, hipStream_t stream) {
  if (n_cont == 0u || n_roots == 0u) return hipSuccess;
  const uint32_t tiles = static_cast<uint32_t>((static_cast<uint64_t>(n_roots) + kScanTile - 1u) / kScanTile);
  const unsigned long long* m = reinterpret_cast<const unsigned long long*>(mask);
  hipLaunchKernelGGL(halo_cont_count_kernel, dim3(tiles), dim3(kScanBlock), 0, stream, m, n_roots, tile_sum);
  hipLaunchKernelGGL(halo_cont_tiles_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, tile_sum, tiles, n_cont, err);
  hipLaunchKernelGGL(halo_cont_base_kernel, dim3(tiles), dim3(kScanBlock), 0, stream, m, n_roots, tile_sum, base);
  const uint32_t gx = std::max<uint32_t>(1u, std::min<uint32_t>(static_cast<uint32_t>((static_cast<uint64_t>(max_fill) + kBlock - 1u) / kBlock), 64u));
  hipLaunchKernelGGL(halo_cont_scatter_kernel, dim3(gx, kContShards), dim3(kBlock), 0, stream, reinterpret_cast<const uint32_t*>(in), in_stride, region, cnt, m, base,
                     n_roots, reinterpret_cast<uint32_t*>(out), out_stride, n_cont, planes, err);
  return hipGetLastError();
}

// mode: halo_select.h kMode* — 0 plain, 1 filter (fast form), 2 capture (tests), 3 generic filter / colour, 4 filter + colour (fast form)
// geom: 0 = one shape per dispatch, 1 = shape pool, 2 = shape pool of prisms (compact LDS slots), 3 = one regular hexagonal prism
// The launch goes to the unit that instantiates the selected kernel's family (halo_select.h family_of); `launched`, if given, is that kernel.
hipError_t launch_trace(const DispatchParams& P, int blocks, hipStream_t stream, int mode, int geom, bool mono, KernelId* launched) {
  const Selection s = select_kernel(make_request(P, mode, geom, mono));
  if (s.err != 0) return static_cast<hipError_t>(s.err);
  if (launched != nullptr) *launched = s.id;
  switch (family_of(s.id)) {
    case kFamMode + kModePlain: return launch_trace_m0(P, blocks, stream, geom, mono);
    case kFamMode + kModeFilter: return launch_trace_m1(P, blocks, stream, geom, mono);
    case kFamMode + kModeCapture: return launch_trace_m2(P, blocks, stream, geom, mono);
    case kFamMode + kModeGeneric: return launch_trace_m3(P, blocks, stream, geom, mono);
    case kFamMode + kModeColor: return launch_trace_m4(P, blocks, stream, geom, mono);
    case kFamFixed + kModePlain: return launch_trace_fx0(P, blocks, stream, geom, mono);
    case kFamFixed + kModeFilter: return launch_trace_fx1(P, blocks, stream, geom, mono);
    case kFamFixedLog + kModePlain: return launch_trace_fxl0(P, blocks, stream, geom, mono);
    case kFamFixedLog + kModeFilter: return launch_trace_fxl1(P, blocks, stream, geom, mono);
    case kFamTile + kModePlain: return launch_trace_tl0(P, blocks, stream, geom, mono);
  }
  return hipErrorInvalidValue;
}

}  // namespace halo
