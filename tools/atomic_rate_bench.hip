// Micro-benchmark: what does gfx950 sustain for the accumulation traffic of the trace kernel — fp32 global atomics on
// random slots of an image plane — and what do the alternatives cost (plain 8-byte log stores, returning atomics)?
// Variants: footprint of the plane (MB), active lanes per instruction (the kernel's miss path runs with ~10 of 64), copies
// addressed by blockIdx & 7 (the kernel's privatised planes), some ALU work between atomics.
//   hipcc --offload-arch=gfx950 -O3 -munsafe-fp-atomics tools/atomic_rate_bench.hip -o tools/atomic_rate_bench.bin
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>

__device__ __forceinline__ uint32_t pcg(uint32_t x) {
  x = x * 747796405u + 2891336453u;
  x = ((x >> ((x >> 28) + 4u)) ^ x) * 277803737u;
  return (x >> 22) ^ x;
}

// MODE 0: non-returning fp32 atomic; 1: plain 4-byte store to the slot; 2: 8-byte store to a per-wave contiguous log;
// 3: returning u32 atomic on a per-workgroup counter + 8-byte store (the shard-log scheme); 4: nothing (ALU only);
// 5: non-returning 64-bit INTEGER atomic on 8-byte slots (the deterministic route's fixed-point planes: same slot counts, twice the bytes)
template <int MODE>
__global__ void __launch_bounds__(256, 5) k(float* plane, uint32_t slot_mask, uint32_t copy_shift, uint32_t iters, uint32_t lane_keep, uint32_t alu, uint2* log,
                                            uint32_t* cnt, float* sink) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  uint32_t s = pcg(t + 1u);
  float acc = 0.0f;
  const uint32_t copy = copy_shift < 31u ? (blockIdx.x & 7u) << copy_shift : 0u;
  const uint32_t wave = t >> 6;
  uint32_t cur = 0u;
  for (uint32_t i = 0; i < iters; i++) {
    s = pcg(s);
    float v = __uint_as_float(0x3f800000u | (s >> 9)) - 1.0f;
    for (uint32_t a = 0; a < alu; a++) v = fmaf(v, 0.999f, 1e-3f);   // stand-in for the trace between two hits
    acc += v;
    const bool on = (pcg(s ^ i) & 63u) < lane_keep;   // a random subset of the lanes takes the miss path
    if (on) {
      const uint32_t slot = (s & slot_mask) + copy;
      if (MODE == 0) {
        unsafeAtomicAdd(plane + slot, v);
      } else if (MODE == 5) {
        atomicAdd(reinterpret_cast<unsigned long long*>(plane) + slot, static_cast<unsigned long long>(v * 4294967296.0f));
      } else if (MODE == 1) {
        plane[slot] = v;
      } else if (MODE == 2) {
        const uint64_t m = __ballot(1);
        const uint32_t pos = cur + __popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull));
        log[static_cast<size_t>(wave) * iters * 64u + pos] = make_uint2(slot, __float_as_uint(v));
      } else if (MODE == 3) {
        const uint64_t m = __ballot(1);
        const uint32_t leader = __ffsll(static_cast<unsigned long long>(m)) - 1u;
        uint32_t base = 0u;
        if ((threadIdx.x & 63u) == leader) base = atomicAdd(&cnt[(blockIdx.x & 255u) * 16u], static_cast<uint32_t>(__popcll(m)));
        base = __shfl(base, static_cast<int>(leader));
        const uint32_t pos = base + __popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull));
        log[(static_cast<size_t>(blockIdx.x & 255u) << 21) + (pos & 0x1FFFFFu)] = make_uint2(slot, __float_as_uint(v));
      }
    }
    if (MODE == 2) cur += __popcll(__ballot(on));
  }
  if (acc == 12345.678f) sink[t] = acc;
}

template <int MODE>
static void run(const char* name, uint32_t foot_mb, uint32_t copies, uint32_t lane_keep, uint32_t alu, float* plane, uint2* log, uint32_t* cnt, float* sink) {
  const uint32_t blocks = 6104, iters = 512;
  const uint32_t slots = (foot_mb << 20) / (MODE == 5 ? 8u : 4u) / copies;   // (foot_mb <= 1024: inside the 1 GB plane either way)
  uint32_t shift = 0;
  while ((1u << shift) < slots) shift++;
  hipMemset(cnt, 0, 256 * 64);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  for (int rep = 0; rep < 2; rep++) {
    hipEventRecord(e0);
    hipLaunchKernelGGL(k<MODE>, dim3(blocks), dim3(256), 0, 0, plane, slots - 1u, copies > 1 ? shift : 31u, iters, lane_keep, alu, log, cnt, sink);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
  }
  float ms = 0;
  hipEventElapsedTime(&ms, e0, e1);
  const double n = double(blocks) * 256 * iters * lane_keep / 64.0;
  std::printf("%-26s foot %4u MB copies %u lanes %2u/64 alu %3u : %7.3f ms  %6.2f G ops/s\n", name, foot_mb, copies, lane_keep, alu, ms, n / ms * 1e-6);
  std::fflush(stdout);
}

// The per-tile append ("tile append"): would the trace kernel sustain the split's scatter itself?  256-thread workgroups, six per CU
// (the 22 960 B of the trace kernel's LDS stand in as s_pad), 128 tiles.  Each lane draws a tile, takes its position from a returning LDS add on
// that tile's counter and stores 8 bytes to the workgroup's own chunk of that tile; at the end the workgroup writes all 128 counts.
// LAYOUT 0: chunk[tile][wg][pos]; 1: chunk[wg][tile][pos]; 2: one region per workgroup with a wave-aggregated cursor (today's log, for scale);
// 3: the LDS add alone, no store.
template <int LAYOUT>
__global__ void __launch_bounds__(256, 6) tile_append(uint2* chunk, uint32_t* cnt, uint32_t* over, uint32_t cap, uint32_t tile_mask, uint32_t iters, uint32_t alu,
                                                      float* sink) {
  __shared__ uint32_t s_tile_n[128];
  __shared__ uint32_t s_pad[5740];
  const uint32_t wg = blockIdx.x, nwg = gridDim.x;
  const uint32_t t = wg * 256u + threadIdx.x;
  if (threadIdx.x < 128u) s_tile_n[threadIdx.x] = 0u;
  s_pad[threadIdx.x] = t;
  __syncthreads();
  uint32_t s = pcg(t + 1u);
  float acc = 0.0f;
  for (uint32_t i = 0; i < iters; i++) {
    s = pcg(s);
    float v = __uint_as_float(0x3f800000u | (s >> 9)) - 1.0f;
    for (uint32_t a = 0; a < alu; a++) v = fmaf(v, 0.999f, 1e-3f);
    acc += v;
    const uint32_t tile = pcg(s ^ 0x9e3779b9u) & tile_mask;
    const uint2 rec = make_uint2(s, __float_as_uint(v));
    if (LAYOUT == 2) {
      const uint64_t m = __ballot(1);
      const uint32_t leader = __ffsll(static_cast<unsigned long long>(m)) - 1u;
      uint32_t base = 0u;
      if ((threadIdx.x & 63u) == leader) base = atomicAdd(&s_tile_n[0], static_cast<uint32_t>(__popcll(m)));
      base = __shfl(base, static_cast<int>(leader));
      const uint32_t pos = base + __popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull));
      if (pos < 128u * cap) chunk[static_cast<size_t>(wg) * 128u * cap + pos] = rec;
      else atomicAdd(over, 1u);
    } else {
      const uint32_t pos = atomicAdd(&s_tile_n[tile], 1u);
      if (LAYOUT == 3) {
        acc += static_cast<float>(pos);
      } else if (pos < cap) {
        const size_t c = LAYOUT == 0 ? static_cast<size_t>(tile) * nwg + wg : static_cast<size_t>(wg) * 128u + tile;
        chunk[c * cap + pos] = rec;
      } else {
        atomicAdd(over, 1u);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 128u) cnt[static_cast<size_t>(threadIdx.x) * nwg + wg] = s_tile_n[threadIdx.x];
  if (acc == 12345.678f) sink[t] = acc + static_cast<float>(s_pad[(threadIdx.x * 7u) % 5740u]);
}

template <int LAYOUT>
static void run_tile(const char* name, uint32_t tiles_on, uint32_t alu, uint2* chunk, uint32_t* cnt, uint32_t* over, float* sink) {
  const uint32_t blocks = 6104, iters = 40, cap = 640;   // 10 240 records per workgroup, 80 per tile: cap = 8 x the even share
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  float best = 1e30f, all[5];
  for (int rep = 0; rep < 5; rep++) {
    hipMemset(over, 0, 4);
    hipEventRecord(e0);
    hipLaunchKernelGGL(tile_append<LAYOUT>, dim3(blocks), dim3(256), 0, 0, chunk, cnt, over, cap, tiles_on - 1u, iters, alu, sink);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    hipEventElapsedTime(&all[rep], e0, e1);
    if (all[rep] < best) best = all[rep];
  }
  for (int i = 1; i < 5; i++)
    for (int j = i; j > 0 && all[j] < all[j - 1]; j--) std::swap(all[j], all[j - 1]);
  // every record is counted, kept or not: the counts the reader would clamp
  static uint32_t h_cnt[128 * 6104];
  uint32_t h_over = 0;
  hipMemcpy(h_cnt, cnt, sizeof(h_cnt), hipMemcpyDeviceToHost);
  hipMemcpy(&h_over, over, 4, hipMemcpyDeviceToHost);
  uint64_t sum = 0;
  for (uint32_t c : h_cnt) sum += c;
  const double n = double(blocks) * 256 * iters;
  std::printf("%-26s tiles %3u/128 alu %3u : min %6.3f median %6.3f ms  %6.2f G records/s (median)  counted %llu of %.0f, past cap %u  [%s]\n", name, tiles_on, alu,
              best, all[2], n / all[2] * 1e-6, static_cast<unsigned long long>(sum), n, h_over, hipGetErrorString(hipGetLastError()));
  std::fflush(stdout);
}

static void tile_rows(float* sink) {
  uint2* chunk;
  uint32_t *cnt, *over;
  if (hipMalloc(&chunk, 6104ull * 128 * 640 * 8) != hipSuccess) {   // 4.0 GB
    std::printf("tile append: no memory for the chunks\n");
    return;
  }
  hipMalloc(&cnt, 6104ull * 128 * 4);
  hipMalloc(&over, 4);
  for (uint32_t alu : {0u, 200u}) {
    run_tile<3>("tile append: LDS add only", 128, alu, chunk, cnt, over, sink);
    run_tile<2>("tile append: one region/wg", 128, alu, chunk, cnt, over, sink);
    for (uint32_t tiles_on : {128u, 64u}) {   // (the fisheye disc fills about half the tiles)
      run_tile<0>("tile append: [tile][wg]", tiles_on, alu, chunk, cnt, over, sink);
      run_tile<1>("tile append: [wg][tile]", tiles_on, alu, chunk, cnt, over, sink);
    }
  }
  hipFree(chunk);
  hipFree(cnt);
  hipFree(over);
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "tile") {   // the per-tile append rows alone
    float* s;
    hipMalloc(&s, 6104ull * 256 * 4);
    tile_rows(s);
    return 0;
  }
  float *plane, *sink;
  uint2* log;
  uint32_t* cnt;
  hipMalloc(&plane, 1ull << 30);
  hipMemset(plane, 0, 1ull << 30);
  hipMalloc(&sink, 6104ull * 256 * 4);
  hipMalloc(&log, 6104ull * 4 * 512 * 64 * 8);   // 6.4 GB
  hipMalloc(&cnt, 256 * 64);
  for (uint32_t alu : {0u, 200u}) {
    run<4>("alu only", 8, 1, 64, alu, plane, log, cnt, sink);
    for (uint32_t lanes : {64u, 10u}) {
      run<0>("atomic_add_f32", 8, 1, lanes, alu, plane, log, cnt, sink);
      run<0>("atomic_add_f32", 64, 8, lanes, alu, plane, log, cnt, sink);
      run<0>("atomic_add_f32", 64, 1, lanes, alu, plane, log, cnt, sink);
      run<0>("atomic_add_f32", 1024, 1, lanes, alu, plane, log, cnt, sink);
      run<0>("atomic_add_f32", 1, 1, lanes, alu, plane, log, cnt, sink);
      run<5>("atomic_add_u64", 16, 1, lanes, alu, plane, log, cnt, sink);
      run<5>("atomic_add_u64", 128, 8, lanes, alu, plane, log, cnt, sink);
      run<5>("atomic_add_u64", 128, 1, lanes, alu, plane, log, cnt, sink);
      run<5>("atomic_add_u64", 1024, 1, lanes, alu, plane, log, cnt, sink);
      run<5>("atomic_add_u64", 2, 1, lanes, alu, plane, log, cnt, sink);
      run<1>("plain store", 64, 8, lanes, alu, plane, log, cnt, sink);
      run<2>("per-wave log store", 64, 8, lanes, alu, plane, log, cnt, sink);
      run<3>("shard log (ret. atomic)", 64, 8, lanes, alu, plane, log, cnt, sink);
    }
  }
  tile_rows(sink);
  return 0;
}
