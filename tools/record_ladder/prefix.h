// prefix.h — force-included (-include) into host-only compiles of the trace translation units by tools/record_ladder/record.sh.
// CPU-ONLY TOOL: the objects it makes register dummy code objects with the HIP runtime.  Never part of a test, never run on a machine with a GPU.
// Every kernel launch of the unit becomes a call of the recorder with the kernel's host address; nothing is launched.
#include <hip/hip_runtime.h>

extern "C" void halo_record_launch(const void* kernel);
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, ...) halo_record_launch(reinterpret_cast<const void*>(kernel))
