// halo_trace_fx1.hip — the kAccFixed instantiations of halo_trace_kernel in kModeFilter (option "deterministic", see halo_select.h kernel_exists).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_fx1(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_family<kFamFixed + kModeFilter>(P, blocks, stream, geom, mono);
}
}  // namespace halo
