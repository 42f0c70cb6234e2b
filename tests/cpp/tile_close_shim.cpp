// tile_close_shim.cpp — hands synthetic per-tile chunks to launch_tile_route_close (halo_launch.h), for tests/test_gpu_tile_route_exact.py.  Host code
// only, linked against libhalo_hip.so; no device code of its own.
//
// Buffers come as PtBuf, as in close_shim.cpp: `bytes` of host memory of which the launcher sees the part behind the first `lead` bytes; the rest is
// guard band.  tt_close allocates every buffer on the device, copies ALL of it in, queues the launcher on one stream of its own — once, or twice when
// a second chunk set is given, with nothing between the two but a copy of the image out (no reset of any buffer) — synchronises, copies ALL of every
// buffer back and returns the HIP status (0 = hipSuccess).
#include <cstddef>
#include <cstdint>
#include <vector>

#include "halo_launch.h"

using namespace halo;

extern "C" {
struct PtBuf {
  void* host;
  uint64_t bytes;
  uint64_t lead;   // multiple of 256: the launcher's pointer keeps hipMalloc's alignment
};
}

namespace {

struct Run {
  struct Dev {
    const PtBuf* b;
    char* d;
  };
  std::vector<Dev> devs;
  hipStream_t stream = nullptr;
  hipError_t err = hipSuccess;

  Run() {
    int n = 0;
    err = hipGetDeviceCount(&n);
    if (err == hipSuccess && n == 0) err = hipErrorNoDevice;
    if (err == hipSuccess) err = hipStreamCreate(&stream);
  }
  bool ok() const { return err == hipSuccess; }
  template <typename T>
  T* in(const PtBuf* b) {
    if (!ok() || b == nullptr || b->host == nullptr) return nullptr;
    char* d = nullptr;
    err = hipMalloc(reinterpret_cast<void**>(&d), b->bytes ? b->bytes : 1);
    if (!ok()) return nullptr;
    devs.push_back(Dev{b, d});
    err = hipMemcpy(d, b->host, b->bytes, hipMemcpyHostToDevice);
    return reinterpret_cast<T*>(d + b->lead);
  }
  int finish() {
    if (stream) {
      const hipError_t e = hipStreamSynchronize(stream);
      if (ok()) err = e;
    }
    for (const Dev& v : devs) {
      if (ok()) err = hipMemcpy(v.b->host, v.d, v.b->bytes, hipMemcpyDeviceToHost);
      (void)hipFree(v.d);
    }
    if (stream) (void)hipStreamDestroy(stream);
    return static_cast<int>(err);
  }
};

}  // namespace

extern "C" {

int tt_device_count() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

uint32_t tt_tiles_max() { return kTileAppendMax; }

// One closing pass over {chunk, cnt}, then — chunk_b given — a second one over {chunk_b, cnt_b} on the same twin, flag and image; xyz_mid (same
// size and lead as xyz) receives the whole image buffer as it stood between the two.
int tt_close(const PtBuf* xyz, uint32_t n_pix, const float* coef, const PtBuf* chunk, const PtBuf* cnt, const PtBuf* chunk_b, const PtBuf* cnt_b, uint32_t wgs,
             uint32_t cap, uint32_t tiles, uint32_t s_log2, uint32_t frac_bits, const PtBuf* twin, const PtBuf* flag, const PtBuf* xyz_mid) {
  Run r;
  float* d_xyz = r.in<float>(xyz);
  HitRec* d_chunk = r.in<HitRec>(chunk);
  uint32_t* d_cnt = r.in<uint32_t>(cnt);
  HitRec* d_chunk_b = r.in<HitRec>(chunk_b);
  uint32_t* d_cnt_b = r.in<uint32_t>(cnt_b);
  double* d_twin = r.in<double>(twin);
  uint32_t* d_flag = r.in<uint32_t>(flag);
  float* d_mid = r.in<float>(xyz_mid);
  if (r.ok()) r.err = launch_tile_route_close(d_xyz, n_pix, coef, d_chunk, cap, d_cnt, wgs, tiles, s_log2, frac_bits, d_twin, d_flag, r.stream, nullptr);
  if (r.ok() && d_chunk_b != nullptr) {
    if (d_mid != nullptr && xyz != nullptr && xyz_mid->bytes == xyz->bytes && xyz_mid->lead == xyz->lead)
      r.err = hipMemcpyAsync(reinterpret_cast<char*>(d_mid) - xyz_mid->lead, reinterpret_cast<char*>(d_xyz) - xyz->lead, xyz->bytes, hipMemcpyDeviceToDevice, r.stream);
    if (r.ok()) r.err = launch_tile_route_close(d_xyz, n_pix, coef, d_chunk_b, cap, d_cnt_b, wgs, tiles, s_log2, frac_bits, d_twin, d_flag, r.stream, nullptr);
  }
  return r.finish();
}

}  // extern "C"
