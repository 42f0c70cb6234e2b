// halo_trace_fxl1.hip — the kAccFixedLog instantiations of halo_trace_kernel in kModeFilter (option "deterministic" under the hit log, see halo_select.h kernel_exists).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_fxl1(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_family<kFamFixedLog + kModeFilter>(P, blocks, stream, geom, mono);
}
}  // namespace halo
