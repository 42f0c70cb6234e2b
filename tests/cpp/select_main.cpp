// select_main.cpp — halo_select.h on the host, without HIP (tests/test_cpp_select.py builds and runs it, and compares its output with
// tests/golden/kernel_selection.txt line by line):
//   1. select_kernel over every request of select_enum.h: per (mode, geom, mono), one line per chosen kernel and per error code with the number
//      of requests that chose it and a hash of their ordinal numbers;
//   2. expand_kernel's round trip: every id of every family's table, expanded to template constants and read back, is itself, exists, and
//      belongs to the family; an id of another family is refused.  Last line: "round trip <ids> of <ids>".
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../../ice_halo_sim_amd/csrc/halo_select.h"
#include "select_enum.h"

namespace {

struct ReadBack {
  halo::KernelId got;
  template <int MODE, int GEOM, bool MONO, int ACC, int LENS, int VIS, bool NOGATE, bool CANON, int ROOT>
  void operator()(halo::KernelConst<MODE, GEOM, MONO, ACC, LENS, VIS, NOGATE, CANON, ROOT>) {
    static_assert(halo::kernel_exists(halo::KernelId{MODE, GEOM, MONO, ACC, LENS, VIS, NOGATE, CANON, ROOT}), "the expander instantiates kernels of the set only");
    got = halo::KernelId{MODE, GEOM, MONO, ACC, LENS, VIS, NOGATE, CANON, ROOT};
  }
};

template <int FAMILY>
void round_trip(int& ids, int& good) {
  const auto& T = halo::FamilyTable<FAMILY>::ids;
  const auto& other = halo::FamilyTable<(FAMILY + 1) % halo::kFamilies>::ids;
  for (int i = 0; i < T.n; i++) {
    ReadBack rb{};
    rb.got.mode = -1;
    const bool ok = halo::expand_kernel<FAMILY>(T.id[i], rb) && rb.got == T.id[i] && halo::kernel_exists(T.id[i]) && halo::family_of(T.id[i]) == FAMILY;
    ids++, good += ok ? 1 : 0;
  }
  ReadBack rb{};
  if (other.n > 0 && halo::expand_kernel<FAMILY>(other.id[0], rb)) good = -1000000;   // another family's kernel
  if constexpr (FAMILY + 1 < halo::kFamilies) round_trip<FAMILY + 1>(ids, good);
}

}  // namespace

int main() {
  std::vector<std::string> out(select_enum::kGroups);
  std::vector<std::thread> pool;
  const int workers = 4;
  for (int w = 0; w < workers; w++)
    pool.emplace_back([&out, w, workers] {
      for (int g = w; g < select_enum::kGroups; g += workers) {
        select_enum::Tally tally;
        select_enum::for_each_request(g, [&](uint64_t ord, const halo::DispatchParams& P, int mode, int geom, bool mono) {
          const halo::Selection s = halo::select_kernel(halo::make_request(P, mode, geom, mono));
          const halo::KernelId& k = s.id;
          tally.add(s.err ? select_enum::error_choice(s.err) : select_enum::Choice{k.mode, k.geom, k.mono, k.acc, k.lens, k.vis, k.nogate, k.canon, k.root}, ord);
        });
        tally.print(g, [&](const char* line) { out[g] += line, out[g] += '\n'; });
      }
    });
  for (auto& t : pool) t.join();
  for (const auto& s : out) std::fputs(s.c_str(), stdout);
  int ids = 0, good = 0;
  round_trip<0>(ids, good);
  std::printf("round trip %d of %d\n", good, ids);
  return good == ids ? 0 : 1;
}
