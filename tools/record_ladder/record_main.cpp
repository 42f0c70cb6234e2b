// record_main.cpp — what the compiled launchers choose, for every request of tests/cpp/select_enum.h: the recorder behind
// tests/golden/kernel_selection.txt (built and run by record.sh, which see).
// CPU-ONLY TOOL: it links host-only objects that register dummy code objects with the HIP runtime.  Never part of a test, never run on a machine
// with a GPU.  It calls halo::launch_trace, whose launches prefix.h turns into halo_record_launch(kernel address); the address's symbol name,
// demangled, holds the instantiation's template arguments.  A call that launches nothing chose the error code it returns.
#include <cxxabi.h>
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "halo_launch.h"   // the recorded tree's (record.sh: -I TREE/ice_halo_sim_amd/csrc)

#include "../../tests/cpp/select_enum.h"

static thread_local const void* t_kernel = nullptr;
static thread_local int t_launches = 0;
extern "C" void halo_record_launch(const void* kernel) {
  t_kernel = kernel;
  t_launches++;
}

static select_enum::Choice choice_of_address(const void* kernel) {
  Dl_info info{};
  if (!dladdr(kernel, &info) || !info.dli_sname) {
    std::fprintf(stderr, "no symbol for %p\n", kernel);
    std::exit(2);
  }
  int status = 0;
  char* dm = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &status);
  const std::string name = dm ? dm : info.dli_sname;
  std::free(dm);
  const size_t at = name.find("halo_trace_kernel<");
  if (at == std::string::npos) {
    std::fprintf(stderr, "not a trace kernel: %s\n", name.c_str());
    std::exit(2);
  }
  int v[9], n = 0;
  const char* s = name.c_str() + at + std::strlen("halo_trace_kernel<");
  while (n < 9) {
    while (*s == ' ' || *s == ',') s++;
    if (!std::strncmp(s, "true", 4)) v[n++] = 1, s += 4;
    else if (!std::strncmp(s, "false", 5)) v[n++] = 0, s += 5;
    else {
      char* e = nullptr;
      v[n++] = static_cast<int>(std::strtol(s, &e, 10));
      if (e == s) break;
      s = e;
    }
  }
  if (n != 9 || *s != '>') {
    std::fprintf(stderr, "unparsed: %s\n", name.c_str());
    std::exit(2);
  }
  return select_enum::Choice{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
}

int main() {
  std::vector<std::string> out(select_enum::kGroups);
  std::mutex names_lock;   // (dladdr and the demangler, one thread at a time)
  std::vector<std::thread> pool;
  for (int w = 0; w < 8; w++)
    pool.emplace_back([&, w] {
      std::unordered_map<const void*, select_enum::Choice> seen;
      for (int g = w; g < select_enum::kGroups; g += 8) {
        select_enum::Tally tally;
        const void* last_k = nullptr;
        select_enum::Choice last_c{};
        select_enum::for_each_request(g, [&](uint64_t ord, const halo::DispatchParams& P, int mode, int geom, bool mono) {
          t_kernel = nullptr;
          t_launches = 0;
          const hipError_t e = halo::launch_trace(P, 64, nullptr, mode, geom, mono);
          if (t_launches > 1) {
            std::fprintf(stderr, "request %llu launched %d kernels\n", static_cast<unsigned long long>(ord), t_launches);
            std::exit(2);
          }
          if (t_kernel == nullptr) {
            tally.add(select_enum::error_choice(static_cast<int>(e)), ord);
            return;
          }
          if (t_kernel != last_k) {
            auto it = seen.find(t_kernel);
            if (it == seen.end()) {
              std::lock_guard<std::mutex> hold(names_lock);
              it = seen.emplace(t_kernel, choice_of_address(t_kernel)).first;
            }
            last_k = t_kernel, last_c = it->second;
          }
          tally.add(last_c, ord);
        });
        tally.print(g, [&](const char* line) { out[g] += line, out[g] += '\n'; });
      }
    });
  for (auto& t : pool) t.join();
  for (const auto& s : out) std::fputs(s.c_str(), stdout);
  return 0;
}
