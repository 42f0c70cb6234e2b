// Exercises the shard entry points of ice_halo_sim_amd/csrc/hip_trace_backend.hpp (SetShard, ExportFixed, ImportFixed): one deterministic session
// traced whole on one backend, then as two shards on two backends whose exported words are added as integers and imported into shard 0 — the image
// bytes and the landed weight must be the whole run's.  Exit codes: 0 ok, 3 BackendUnavailableError (no gfx950), 1 failure.
#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ice_halo_sim_amd/csrc/hip_trace_backend.hpp"

namespace {
// device memory without the HIP headers (this file compiles with plain g++): the runtime the library already loaded
typedef int (*malloc_fn)(void**, size_t);
typedef int (*free_fn)(void*);
typedef int (*memcpy_fn)(void*, const void*, size_t, int);
struct Hip {
  malloc_fn malloc_ = nullptr;
  free_fn free_ = nullptr;
  memcpy_fn memcpy_ = nullptr;
  bool load() {
    void* lib = dlopen("libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/libamdhip64.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return false;
    malloc_ = reinterpret_cast<malloc_fn>(dlsym(lib, "hipMalloc"));
    free_ = reinterpret_cast<free_fn>(dlsym(lib, "hipFree"));
    memcpy_ = reinterpret_cast<memcpy_fn>(dlsym(lib, "hipMemcpy"));
    return malloc_ && free_ && memcpy_;
  }
};
constexpr int kHostToDevice = 1, kDeviceToHost = 2;   // hipMemcpyKind

void make_scene(HaloScene& sc, HaloRender& rd) {
  std::memset(&sc, 0, sizeof(sc));
  sc.sun_altitude = 20.0f;
  sc.sun_diameter = 0.5f;
  sc.max_hits = 7;
  sc.layer_count = 1;
  sc.layers[0].entry_count = 2;   // two entries: every shard crosses the entry boundary
  for (int k = 0; k < 2; k++) {
    HaloEntry& e = sc.layers[0].entries[k];
    e.crystal.kind = HALO_CRYSTAL_PRISM;
    e.crystal.height[0] = {HALO_DIST_NONE, k == 0 ? 1.3f : 0.4f, 0.0f};
    for (int i = 0; i < 6; i++) e.crystal.face_dist[i] = {HALO_DIST_NONE, 1.0f, 0.0f};
    e.axis.azimuth = {HALO_DIST_UNIFORM, 0.0f, 360.0f};
    e.axis.latitude = {HALO_DIST_GAUSS, k == 0 ? 0.0f : 90.0f, 0.5f};
    e.axis.roll = {HALO_DIST_UNIFORM, 0.0f, 360.0f};
    e.proportion = k == 0 ? 0.7f : 0.3f;
    e.crystal_config_id = 3 + k;
  }
  std::memset(&rd, 0, sizeof(rd));
  rd.lens_type = HALO_LENS_FISHEYE_EQUAL_AREA;
  rd.fov = 180.0f;
  rd.width = 160;
  rd.height = 90;
  rd.view_el = 30.0f;
  rd.visible = HALO_VISIBLE_UPPER;
}
}  // namespace

int main() {
  try {
    HaloScene sc;
    HaloRender rd;
    make_scene(sc, rd);
    const HaloWl wl = {550.0f, 1.0f, -1, 0};
    const size_t n = 100003, npix = static_cast<size_t>(rd.width) * rd.height;
    const uint32_t seed = 42;
    const int64_t ray_base = 5ll << 20;

    std::vector<float> whole(npix * 3), merged(npix * 3);
    float landed_whole = 0.0f, landed_merged = 0.0f;
    {
      halo::HipTraceBackend be(0, seed);
      be.SetDeterministic(true);
      be.SetOption("ray_base", ray_base);
      be.BeginSession(sc, rd, wl, n);
      halo::LayerHandle lh = be.TraceLayer(n);
      be.EndSession();
      halo::XyzImageData xyz{whole.data(), rd.width, rd.height};
      be.ReadbackXyzAccum(xyz, landed_whole);
      if (lh.stats.root_count != n) {
        std::printf("whole run traced %llu roots\n", (unsigned long long)lh.stats.root_count);
        return 1;
      }
    }
    Hip hip;
    if (!hip.load()) {
      std::printf("error: the HIP runtime's hipMalloc / hipMemcpy are not loadable\n");
      return 1;
    }
    halo::HipTraceBackend s0(0, seed), s1(0, seed);
    halo::HipTraceBackend* shard[2] = {&s0, &s1};
    uint64_t roots[2] = {0, 0}, n_words = 0;
    std::vector<uint64_t> sum, part;
    halo::HipTraceBackend::FixedLayout layout;
    void* dev = nullptr;
    for (uint32_t k = 0; k < 2; k++) {
      halo::HipTraceBackend& be = *shard[k];
      be.SetDeterministic(true);
      be.SetOption("ray_base", ray_base);
      be.SetShard(k, 2);
      be.BeginSession(sc, rd, wl, n);          // the WHOLE session's count on every shard
      roots[k] = be.TraceLayer(n).stats.root_count;
      be.EndSession();
      if (!dev) {
        n_words = be.FixedWords(1);
        if (hip.malloc_(&dev, n_words * sizeof(uint64_t)) != 0) return 1;
        sum.assign(n_words, 0);
        part.resize(n_words);
      }
      layout = be.ExportFixed(dev, n_words);
      if (hip.memcpy_(part.data(), dev, n_words * sizeof(uint64_t), kDeviceToHost) != 0) return 1;
      for (uint64_t i = 0; i < n_words; i++) sum[i] += part[i];   // modulo 2^64
    }
    // a shard must not fold its part of the image in silence
    bool guarded = false;
    {
      s1.BeginSession(sc, rd, wl, n);
      s1.TraceLayer(n);
      s1.EndSession();
      try {
        halo::XyzImageData xyz{merged.data(), rd.width, rd.height};
        float l = 0.0f;
        s1.ReadbackXyzAccum(xyz, l);
      } catch (const std::runtime_error& e) {
        guarded = std::strstr(e.what(), "halo_export_fixed") != nullptr;
      }
    }
    if (hip.memcpy_(dev, sum.data(), n_words * sizeof(uint64_t), kHostToDevice) != 0) return 1;
    s0.ImportFixed(dev, n_words, layout, n);
    halo::XyzImageData xyz{merged.data(), rd.width, rd.height};
    s0.ReadbackXyzAccum(xyz, landed_merged);
    hip.free_(dev);
    const bool same = std::memcmp(whole.data(), merged.data(), whole.size() * sizeof(float)) == 0 && landed_whole == landed_merged;
    double y = 0.0;
    for (size_t i = 1; i < whole.size(); i += 3) y += whole[i];
    std::printf("shards: roots %llu + %llu of %zu, planes %u F %u, landed %.3f / %.3f, sumY %.3f, same_bytes %d, guarded %d\n", (unsigned long long)roots[0],
                (unsigned long long)roots[1], n, layout.plane_cnt, layout.frac_bits, landed_whole, landed_merged, y, same ? 1 : 0, guarded ? 1 : 0);
    const bool ok = same && guarded && roots[0] + roots[1] == n && roots[0] > 0 && roots[1] > 0 && layout.plane_cnt == 1 && landed_whole > 0.0f && y > 0.0;
    return ok ? 0 : 1;
  } catch (const halo::BackendUnavailableError& e) {
    std::printf("BackendUnavailableError: %s\n", e.what());
    return 3;
  } catch (const std::exception& e) {
    std::printf("error: %s\n", e.what());
    return 1;
  }
}
