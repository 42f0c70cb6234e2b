#!/bin/sh
# record.sh TREE WORKDIR > selection.txt — which instantiation of halo_trace_kernel the COMPILED launchers of a source tree pick, for every
# request that tests/cpp/select_enum.h enumerates, in the format of tests/golden/kernel_selection.txt.
#
# CPU-ONLY TOOL.  It compiles the tree's trace translation units and halo_kernels.hip host-only, with every kernel launch turned into a call of
# the recorder (prefix.h), and links them with zeroed stand-ins for the code objects: the program registers dummy code objects with the HIP
# runtime.  It is never part of a test and never run on a machine with a GPU.
#
# Use: the fixture is the answer of the tree before a change of the selection (git worktree add TREE <commit>); the same run over the changed
# tree must give the same bytes.  It covers the expander and the per-unit families, which tests/cpp/select_main.cpp does not.
set -e
tree=$1
work=$2
here=$(cd "$(dirname "$0")" && pwd)
hipcc=${HIPCC:-hipcc}
mkdir -p "$work"
units="halo_trace_m0 halo_trace_m1 halo_trace_m2 halo_trace_m3 halo_trace_m4 halo_trace_fx0 halo_trace_fx1 halo_trace_fxl0 halo_trace_fxl1 halo_trace_tl0 halo_kernels"
pids=""
for u in $units; do
  "$hipcc" --cuda-host-only -std=c++17 -O1 -fPIC -I "$tree/include" -include "$here/prefix.h" -c "$tree/ice_halo_sim_amd/csrc/$u.hip" -o "$work/$u.o" &
  pids="$pids $!"
done
for p in $pids; do wait "$p"; done
objs=""
for u in $units; do objs="$objs $work/$u.o"; done
# shellcheck disable=SC2086
nm -u $objs | grep -o '__hip_fatbin_[0-9A-Za-z_]*' | sort -u | sed 's/.*/const char &[64] = {0};/' > "$work/fatbins.c"
rocm=$(dirname "$(dirname "$(command -v "$hipcc")")")
# shellcheck disable=SC2086
"$hipcc" --cuda-host-only -x hip -std=c++17 -O2 -fPIC -I "$tree/include" -I "$tree/ice_halo_sim_amd/csrc" -c "$here/record_main.cpp" -o "$work/record_main.o"
cc -c "$work/fatbins.c" -o "$work/fatbins.o"
# shellcheck disable=SC2086
c++ -rdynamic -o "$work/record" "$work/record_main.o" "$work/fatbins.o" $objs -L "$rocm/lib" -lamdhip64 -ldl -lpthread -Wl,-rpath,"$rocm/lib"
"$work/record"
