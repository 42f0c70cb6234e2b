// halo_radix.h — the digits of the radix selects over float bit patterns (positive floats order like their patterns): 11 + 11 + 10 bits, the
// widest histogram 2048 bins, one workgroup of 1024 threads per histogram.  Shared by the auto-exposure select (halo_autoev.hip, one rank) and the
// image-statistics select (halo_stats.hip, up to 32 ranks at once).
#ifndef HALO_RADIX_H_
#define HALO_RADIX_H_

#include <cstdint>

#include <hip/hip_runtime.h>

namespace halo {

namespace {

constexpr int kAevBlock = 1024;            // 16 wave64: the pick scans 2048 bins two per thread
constexpr uint32_t kAevBins = 2048u;       // the widest digit (11 bits)
__host__ __device__ constexpr uint32_t aev_shift(uint32_t pass) { return pass == 0u ? 21u : (pass == 1u ? 10u : 0u); }
__host__ __device__ constexpr uint32_t aev_width(uint32_t pass) { return pass == 2u ? 10u : 11u; }

}  // namespace

}  // namespace halo

#endif
