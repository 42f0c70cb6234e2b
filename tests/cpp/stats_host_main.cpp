// stats_host_main.cpp — the host halves of halo_consumer_stats (halo_host.cpp PercentileRank, BinnedSum) on their edge inputs, as a stand-alone
// program: tests/test_cpp_stats_host.py builds it from the host sources alone with -fsanitize=address,undefined and runs it on the CPU.  No GPU,
// no HIP runtime, nothing loaded into Python.  Prints "ok" and returns 0, or says what was wrong and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../ice_halo_sim_amd/csrc/halo_host.hpp"

using halo::host::BinnedSum;
using halo::host::PercentileRank;

static int failures = 0;
#define EXPECT(c)                                       \
  do {                                                  \
    if (!(c)) {                                         \
      std::printf("line %d: %s\n", __LINE__, #c);       \
      failures++;                                       \
    }                                                   \
  } while (0)

int main() {
  uint64_t r = 0;
  double f = 0.0;
  // the rank rule at its ends and on the largest image
  EXPECT(PercentileRank(0.0, 1, &r, &f) && r == 0 && f == 0.0);
  EXPECT(PercentileRank(100.0, 1, &r, &f) && r == 0 && f == 0.0);
  EXPECT(PercentileRank(100.0, 1ull << 25, &r, &f) && r == (1ull << 25) - 1 && f == 0.0);
  EXPECT(PercentileRank(50.0, 101, &r, &f) && r == 50 && f == 0.0);
  EXPECT(PercentileRank(50.0, 2, &r, &f) && r == 0 && f == 0.5);
  EXPECT(PercentileRank(99.99, 1ull << 25, &r, &f) && r < (1ull << 25) - 1 && f >= 0.0 && f < 1.0);
  EXPECT(!PercentileRank(-1e-9, 10, &r, &f) && !PercentileRank(100.0000001, 10, &r, &f));
  EXPECT(!PercentileRank(std::numeric_limits<double>::quiet_NaN(), 10, &r, &f) && !PercentileRank(50.0, 0, &r, &f));
  EXPECT(!PercentileRank(50.0, 10, nullptr, &f) && !PercentileRank(50.0, 10, &r, nullptr));
  // the binned sums: empty, one denormal, the top finite exponent as full as 2^25 values make it (the widest integer), a tie, infinity
  std::vector<uint64_t> b(512, 0);
  EXPECT(BinnedSum(b.data(), false) == 0.0 && BinnedSum(b.data(), true) == 0.0);
  b[0] = 1;
  EXPECT(BinnedSum(b.data(), false) == std::ldexp(1.0, -149) && BinnedSum(b.data(), true) == std::ldexp(1.0, -298));
  b.assign(512, 0);
  for (int e = 0; e < 255; e++) b[e] = b[256 + e] = (1ull << 49) - 1;
  const double big = BinnedSum(b.data(), false), big2 = BinnedSum(b.data(), true);
  EXPECT(std::isfinite(big) && big > std::ldexp(1.0, 152) && big < std::ldexp(1.0, 154));
  EXPECT(std::isfinite(big2) && big2 > std::ldexp(1.0, 280) && big2 < std::ldexp(1.0, 282));
  b.assign(512, 0);
  b[60] = (1ull << 54) | (6ull << 2) | 2;   // 2^52 + 6 kept, guard set, nothing below: ties to even, down
  EXPECT(BinnedSum(b.data(), false) == std::ldexp(static_cast<double>((1ull << 52) + 6), 2 + 59 - 149));
  b[60] = (1ull << 54) | (7ull << 2) | 2;   // odd: up
  EXPECT(BinnedSum(b.data(), false) == std::ldexp(static_cast<double>((1ull << 52) + 8), 2 + 59 - 149));
  b[60] = ~0ull;                            // all ones: the round-up carries into a 54th bit
  EXPECT(BinnedSum(b.data(), false) == std::ldexp(1.0, 64 + 59 - 149));
  b.assign(512, 0);
  b[255] = 0x800000;
  EXPECT(std::isinf(BinnedSum(b.data(), false)));
  b.assign(512, 0);
  b[256 + 255] = 1ull << 22;
  EXPECT(std::isinf(BinnedSum(b.data(), true)));
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
