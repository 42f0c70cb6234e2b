// halo_trace_tl0.hip — the kAccTileFinal instantiations of halo_trace_kernel in kModePlain (option "tile_append", see halo_trace.inl launch_tile).
#include "halo_trace.inl"

namespace halo {
hipError_t launch_trace_tl0(const DispatchParams& P, int blocks, hipStream_t stream, int geom, bool mono) {
  return launch_tile<kModePlain>(P, blocks, stream, geom, mono);
}
}  // namespace halo
