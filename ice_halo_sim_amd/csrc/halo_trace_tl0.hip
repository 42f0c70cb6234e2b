// halo_trace_tl0.hip — the kAccTileFinal instantiations of halo_trace_kernel in kModePlain (option "tile_append", see halo_select.h kernel_exists).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_tl0(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_family<kFamTile + kModePlain>(P, blocks, stream, geom, mono);
}
// One resident round of the ticketed kernels: what the runtime says a CU holds of them (they share registers and LDS across lenses and root forms
// to within the allocator's whim; the headline's instantiation is asked), once per process; the bound the kernels are compiled for if it will not say.
int tile_ticket_resident_per_cu() {
  static const int per_cu = [] {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &n, halo_trace_kernel<kModePlain, kGeomOneHex, true, kAccTileFinal, HALO_LENS_FISHEYE_EQUAL_AREA, HALO_VISIBLE_UPPER, true, false, kRootTicket + kRootGenLutUniform>, kBlock, 0);
    if (e != hipSuccess) (void)hipGetLastError();
    constexpr int kBound = min_waves<kModePlain, kGeomOneHex, true, kAccTileFinal>();   // waves per SIMD = workgroups per CU: four waves, four SIMDs
    return (e == hipSuccess && n > 0) ? std::min(n, kBound) : kBound;
  }();
  return per_cu;
}
}  // namespace halo
