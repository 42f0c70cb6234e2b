// halo_trace_fxl0.hip — the kAccFixedLog instantiations of halo_trace_kernel in kModePlain (option "deterministic" under the hit log, see halo_select.h kernel_exists).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_fxl0(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_family<kFamFixedLog + kModePlain>(P, blocks, stream, geom, mono);
}
}  // namespace halo
