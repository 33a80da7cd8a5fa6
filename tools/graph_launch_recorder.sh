#!/bin/bash
# Build tools/graph_launch_recorder.cpp against the graph-side sources of one tree (no GPU, no device code):
#   tools/graph_launch_recorder.sh TREE OUT [extra host flags, e.g. -fsanitize=address,undefined]
# TREE: a checkout of this repository (its stonkgs_amd/csrc and include are used); OUT: the program to write.
# To compare two commits: build one program per tree, run both, `cmp` the two outputs.
set -euo pipefail
here=$(cd "$(dirname "$0")" && pwd)
tree=$(cd "$1" && pwd)
out=$2
shift 2
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
flags=(--offload-arch=gfx950 --cuda-host-only -O1 -g -std=c++17 -I"$tree/include" -I"$tree/stonkgs_amd/csrc" -Wno-unused-result
       -ffp-contract=fast "$@")
for f in node2vec link_prediction kg_baseline transe; do
  hipcc "${flags[@]}" -c "$tree/stonkgs_amd/csrc/$f.hip" -o "$work/$f.o" &
done
hipcc "${flags[@]}" -x hip -c "$here/graph_launch_recorder.cpp" -o "$work/recorder.o" &
wait
# a host-only object refers to its translation unit's device binary, __hip_fatbin_<id>: an empty bundle stands in for each
for s in $(nm -u "$work"/*.o | grep -o '__hip_fatbin_[0-9a-f]*' | sort -u); do
  echo "__attribute__((section(\".hip_fatbin\"), aligned(4096))) const char $s[32] = \"__CLANG_OFFLOAD_BUNDLE__\";"
done > "$work/fatbin_stubs.c"
llvm=${ROCM_PATH:-/opt/rocm}/lib/llvm/bin
"$llvm/clang" -c "$work/fatbin_stubs.c" -o "$work/fatbin_stubs.o"
"$llvm/clang++" "$@" -o "$out" "$work"/*.o   # (not hipcc: the HIP runtime is not linked, the program defines what is used)
