// shapegen_shim.cpp — whole shape records of the device crystal generators (launch_shapegen, halo_launch.h) next to the host builder's
// (geom::MakeShapeDev, halo_geom.h), for tests/test_gpu_shapegen_records.py and tests/test_shapegen_model.py.  Host code only, linked against
// libhalo_hip.so; no device code of its own.
//
// sg_device takes `n_cases` crystals and runs each through launch_shapegen with the recipe production makes (host::MakeRecipe), every case into
// its own segment of ONE device buffer: kGuard records of poison, the pool of n records, kGuard records of poison.
//
// Prefill: NONE, which is what production does.  The backend's pools (halo_backend.cpp: shapes_s, reserved by reserve_idle; the DevBuf of
// halo_generate_shapes) come from hipMalloc and are reused from launch to launch without a memset — "every record gets its counts written ... so
// the pool needs no clearing" (halo_shapegen.hip) — so a record starts as whatever the memory held.  Here that is the poison byte, pool and guards
// alike: a row the generator should have written and did not shows as poison, not as a plausible zero.
//
// All launches go to one stream of the shim's own, then one copy of the whole buffer back (guards included) and one synchronise; the return value
// is the HIP status (0 = hipSuccess).  sg_host fills the same records on the host and needs no GPU.
#include <cstddef>
#include <cstdint>
#include <string>

#include "halo_geom.h"
#include "halo_host.hpp"
#include "halo_launch.h"

using namespace halo;

namespace {

constexpr uint32_t kGuard = 2u;

template <class S>
void fill_host(const HaloCrystal* crystals, uint32_t n_cases, uint32_t seed, uint64_t first_index, uint32_t n, void* out) {
  S* rec = static_cast<S*>(out);
  for (uint32_t c = 0; c < n_cases; c++) {
    const geom::CrystalRecipe rc = host::MakeRecipe(crystals[c]);
    for (uint32_t k = 0; k < n; k++) geom::MakeShapeDev(seed, rc, first_index + k, rec[static_cast<size_t>(c) * n + k]);
  }
}

#define SG_MEMBER(S, m) (text += std::string(#m) + ":" + std::to_string(offsetof(S, m)) + ":" + std::to_string(sizeof(S::m)) + ";")
template <class S>
std::string layout_common() {
  std::string text;
  SG_MEMBER(S, face_cnt);
  SG_MEMBER(S, tri_cnt);
  SG_MEMBER(S, slab_cnt);
  SG_MEMBER(S, single_cnt);
  SG_MEMBER(S, face);
  SG_MEMBER(S, slab);
  SG_MEMBER(S, tri_v);
  SG_MEMBER(S, tri_na);
  SG_MEMBER(S, tri_face);
  SG_MEMBER(S, face_number);
  SG_MEMBER(S, single);
  return text;
}

}  // namespace

extern "C" {

int sg_device_count() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

uint32_t sg_guard_records() { return kGuard; }

// "member:offset:size;...;sizeof:N;" of ShapeDev (prism_records = 0) or ShapePrism (1): every member, the trailing pad included
const char* sg_layout(int prism_records) {
  static std::string kept[2];
  std::string text;
  if (prism_records) {
    text = layout_common<ShapePrism>();
    SG_MEMBER(ShapePrism, pad);
    text += "sizeof:" + std::to_string(sizeof(ShapePrism)) + ";";
  } else {
    text = layout_common<ShapeDev>();
    SG_MEMBER(ShapeDev, pad2);
    text += "sizeof:" + std::to_string(sizeof(ShapeDev)) + ";";
  }
  kept[prism_records ? 1 : 0] = text;
  return kept[prism_records ? 1 : 0].c_str();
}

// n_cases * n records into `out`, case-major
int sg_host(const HaloCrystal* crystals, uint32_t n_cases, uint32_t seed, uint64_t first_index, uint32_t n, int prism_records, void* out) {
  if (!crystals || (!out && n_cases && n)) return -1;
  if (prism_records) fill_host<ShapePrism>(crystals, n_cases, seed, first_index, n, out);
  else fill_host<ShapeDev>(crystals, n_cases, seed, first_index, n, out);
  return 0;
}

// n_cases segments of (kGuard + n + kGuard) records into `out`, case-major, exactly as the device buffer stood after the last launch
int sg_device(const HaloCrystal* crystals, uint32_t n_cases, uint32_t seed, uint64_t first_index, uint32_t n, int prism_records, int serial, uint32_t poison_byte,
              void* out) {
  if (!crystals || !out) return -1;
  const size_t rec = prism_records ? sizeof(ShapePrism) : sizeof(ShapeDev);
  const size_t seg = (static_cast<size_t>(n) + 2u * kGuard) * rec, bytes = seg * n_cases;
  int devs = 0;
  hipError_t err = hipGetDeviceCount(&devs);
  if (err == hipSuccess && devs == 0) err = hipErrorNoDevice;
  hipStream_t stream = nullptr;
  char* d = nullptr;
  if (err == hipSuccess) err = hipStreamCreate(&stream);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d), bytes ? bytes : 1);
  if (err == hipSuccess && bytes) err = hipMemsetAsync(d, static_cast<int>(poison_byte & 0xFFu), bytes, stream);
  for (uint32_t c = 0; c < n_cases && err == hipSuccess; c++)
    err = launch_shapegen(d + c * seg + kGuard * rec, prism_records != 0, n, seed, host::MakeRecipe(crystals[c]), first_index, stream, serial != 0);
  if (err == hipSuccess && bytes) err = hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, stream);
  if (stream) {
    const hipError_t e = hipStreamSynchronize(stream);
    if (err == hipSuccess) err = e;
  }
  if (d) (void)hipFree(d);
  if (stream) (void)hipStreamDestroy(stream);
  return static_cast<int>(err);
}

}  // extern "C"
