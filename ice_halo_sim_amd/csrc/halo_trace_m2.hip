// halo_trace_m2.hip — the kModeCapture instantiations of halo_trace_kernel (see halo_trace.inl).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_m2(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_family<kFamMode + kModeCapture>(P, blocks, stream, geom, mono);
}
}  // namespace halo
