// passes_shim.cpp — hands synthetic records to the launchers of the accumulation and reorder passes (halo_launch.h), for
// tests/test_gpu_passes_exact.py.  Host code only, linked against libhalo_hip.so; no device code of its own.
//
// Every buffer comes as a PtBuf: `bytes` of host memory of which the launcher sees the part behind the first `lead` bytes — what lies before
// (and whatever the test leaves behind the part the kernels may touch) is a guard band.  An entry point allocates each buffer on the device, copies
// ALL of it in, calls one launcher on a stream of its own, synchronises, copies ALL of every buffer back and returns the HIP status (0 = hipSuccess).
// A PtBuf with host == nullptr (or a null PtBuf pointer) hands the launcher a null pointer.
#include <cstddef>
#include <cstdint>
#include <cstring>
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
  int finish(hipError_t launched) {
    if (ok()) err = launched;
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

int pt_device_count() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// constants of halo_device.h / halo_trace.h by name; -1 for an unknown name
int64_t pt_const(const char* name) {
  const struct {
    const char* k;
    int64_t v;
  } tab[] = {
      {"kBinCntStride", kBinCntStride},
      {"kBinTileLog2", kBinTileLog2},
      {"kLogWlShift", kLogWlShift},
      {"kMonoRows", kMonoRows},
      {"kFoldGroup", kFoldGroup},
      {"kContShards", kContShards},
      {"kContCntStride", kContCntStride},
      {"kContPlaneRoot", kContPlaneRoot},
      {"kContPlaneSeq", kContPlaneSeq},
      {"kContMaskWords", kContMaskWords},
      {"kContErrKey", kContErrKey},
      {"kContErrSum", kContErrSum},
      {"sizeof_WlEntryDev", static_cast<int64_t>(sizeof(WlEntryDev))},
      {"offsetof_cmf_x", static_cast<int64_t>(offsetof(WlEntryDev, cmf_x))},
      {"offsetof_cmf_y", static_cast<int64_t>(offsetof(WlEntryDev, cmf_y))},
      {"offsetof_cmf_z", static_cast<int64_t>(offsetof(WlEntryDev, cmf_z))},
      {"sizeof_HitRec", static_cast<int64_t>(sizeof(HitRec))},
      {"HALO_WL_POOL_MAX", HALO_WL_POOL_MAX},
  };
  for (const auto& e : tab)
    if (std::strcmp(e.k, name) == 0) return e.v;
  return -1;
}

uint32_t pt_mono_slot(uint32_t pix, uint32_t s_log2) { return MonoSlot(pix, s_log2); }
uint64_t pt_twin_offset(uint64_t off, uint32_t plane_log2, uint32_t copies_log2) { return TwinOffset(off, plane_log2, copies_log2); }

int pt_log_route(const PtBuf* plane, const PtBuf* log, uint32_t cap1, const PtBuf* cnt1, uint32_t regions, const PtBuf* list2, uint32_t cap2, const PtBuf* cnt2,
                 uint32_t tiles, uint32_t planes, uint32_t s_log2, int interleaved, uint32_t frac_bits, const PtBuf* ovf, const PtBuf* ovf_flag, uint32_t copies_log2) {
  Run r;
  float* d_plane = r.in<float>(plane);
  HitRec* d_log = r.in<HitRec>(log);
  uint32_t* d_cnt1 = r.in<uint32_t>(cnt1);
  HitRec* d_list2 = r.in<HitRec>(list2);
  uint32_t* d_cnt2 = r.in<uint32_t>(cnt2);
  double* d_ovf = r.in<double>(ovf);
  uint32_t* d_flag = r.in<uint32_t>(ovf_flag);
  return r.finish(r.ok() ? launch_log_route(d_plane, d_log, cap1, d_cnt1, regions, d_list2, cap2, d_cnt2, tiles, planes, s_log2, interleaved != 0, frac_bits, d_ovf, d_flag,
                                            copies_log2, r.stream, nullptr)
                         : r.err);
}

int pt_log_route_xyz(const PtBuf* planes, uint32_t plane_stride, const PtBuf* log, uint32_t cap1, const PtBuf* cnt1, uint32_t regions, const PtBuf* list2, uint32_t cap2,
                     const PtBuf* cnt2, uint32_t tiles, uint32_t s_log2, const PtBuf* pool, uint32_t pool_size, uint32_t frac_bits, const PtBuf* ovf, const PtBuf* ovf_flag,
                     uint32_t copies_log2) {
  Run r;
  float* d_planes = r.in<float>(planes);
  HitRec* d_log = r.in<HitRec>(log);
  uint32_t* d_cnt1 = r.in<uint32_t>(cnt1);
  HitRec* d_list2 = r.in<HitRec>(list2);
  uint32_t* d_cnt2 = r.in<uint32_t>(cnt2);
  WlEntryDev* d_pool = r.in<WlEntryDev>(pool);
  double* d_ovf = r.in<double>(ovf);
  uint32_t* d_flag = r.in<uint32_t>(ovf_flag);
  return r.finish(r.ok() ? launch_log_route_xyz(d_planes, plane_stride, d_log, cap1, d_cnt1, regions, d_list2, cap2, d_cnt2, tiles, s_log2, d_pool, pool_size, frac_bits, d_ovf,
                                                d_flag, copies_log2, r.stream, nullptr)
                         : r.err);
}

int pt_bin_accumulate(const PtBuf* plane, const PtBuf* list, uint32_t cap, const PtBuf* cnt, uint32_t tiles, uint32_t frac_bits) {
  Run r;
  float* d_plane = r.in<float>(plane);
  HitRec* d_list = r.in<HitRec>(list);
  uint32_t* d_cnt = r.in<uint32_t>(cnt);
  return r.finish(r.ok() ? launch_bin_accumulate(d_plane, d_list, cap, d_cnt, tiles, frac_bits, r.stream) : r.err);
}

int pt_bin_two_level(const PtBuf* plane, const PtBuf* list1, uint32_t cap1, const PtBuf* cnt1, uint32_t lists1, const PtBuf* list2, uint32_t cap2, const PtBuf* cnt2,
                     uint32_t tiles, uint32_t fan_log2, uint32_t frac_bits, const PtBuf* ovf, const PtBuf* ovf_flag) {
  Run r;
  float* d_plane = r.in<float>(plane);
  HitRec* d_list1 = r.in<HitRec>(list1);
  uint32_t* d_cnt1 = r.in<uint32_t>(cnt1);
  HitRec* d_list2 = r.in<HitRec>(list2);
  uint32_t* d_cnt2 = r.in<uint32_t>(cnt2);
  double* d_ovf = r.in<double>(ovf);
  uint32_t* d_flag = r.in<uint32_t>(ovf_flag);
  return r.finish(r.ok() ? launch_bin_two_level(d_plane, d_list1, cap1, d_cnt1, lists1, d_list2, cap2, d_cnt2, tiles, fan_log2, frac_bits, d_ovf, d_flag, r.stream, nullptr)
                         : r.err);
}

// coef: n_planes (<= kFoldGroup) triples
int pt_fold(const PtBuf* xyz, const PtBuf* planes, uint32_t n_pix, uint32_t s_log2, uint32_t copies, uint32_t n_planes, const float* coef, const PtBuf* ovf,
            const PtBuf* ovf_flag) {
  if (n_planes > kFoldGroup) return static_cast<int>(hipErrorInvalidValue);
  Run r;
  FoldCoef fc;
  std::memset(&fc, 0, sizeof(fc));
  std::memcpy(fc.c, coef, sizeof(float) * 3u * n_planes);
  float* d_xyz = r.in<float>(xyz);
  float* d_planes = r.in<float>(planes);
  double* d_ovf = r.in<double>(ovf);
  uint32_t* d_flag = r.in<uint32_t>(ovf_flag);
  return r.finish(r.ok() ? launch_fold(d_xyz, d_planes, n_pix, s_log2, copies, n_planes, fc, d_ovf, d_flag, r.stream) : r.err);
}

int pt_cont_reorder(const PtBuf* in, uint32_t in_stride, uint32_t region, const PtBuf* cnt, uint32_t max_fill, const PtBuf* mask, uint32_t n_roots, const PtBuf* tile_sum,
                    const PtBuf* base, const PtBuf* out, uint32_t out_stride, uint32_t n_cont, uint32_t planes, const PtBuf* err) {
  Run r;
  float* d_in = r.in<float>(in);
  uint32_t* d_cnt = r.in<uint32_t>(cnt);
  uint32_t* d_mask = r.in<uint32_t>(mask);
  uint32_t* d_tile_sum = r.in<uint32_t>(tile_sum);
  uint32_t* d_base = r.in<uint32_t>(base);
  float* d_out = r.in<float>(out);
  uint32_t* d_err = r.in<uint32_t>(err);
  return r.finish(r.ok() ? launch_cont_reorder(d_in, in_stride, region, d_cnt, max_fill, d_mask, n_roots, d_tile_sum, d_base, d_out, out_stride, n_cont, planes, d_err, r.stream)
                         : r.err);
}

}  // extern "C"
