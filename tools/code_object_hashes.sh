#!/bin/bash
# usage: bash tools/code_object_hashes.sh BUILD_DIR
# For every object file of wurblpt_amd/csrc/Makefile in BUILD_DIR: "<unit> <sha256 of its gfx950 code object> <sha256 of the code
# object's disassembly>" (16 hex digits each).  Two builds compare when they were compiled from the same source path (hipcc
# derives a symbol of each unit from it), e.g. the parent's sources and this tree's copied in turn to one directory.
B=$1; T=$(mktemp -d)
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
for o in "$B"/*.o; do
  n=$(basename "$o" .o)
  "$LLVM/llvm-objcopy" --dump-section=.hip_fatbin="$T/$n.fb" "$o" /dev/null 2>/dev/null || continue
  "$LLVM/clang-offload-bundler" --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$T/$n.fb" --output="$T/$n.co" --unbundle || continue
  h1=$(sha256sum < "$T/$n.co" | cut -c1-16)
  h2=$("$LLVM/llvm-objdump" -d --no-show-raw-insn "$T/$n.co" | tail -n +3 | sha256sum | cut -c1-16)
  echo "$n $h1 $h2"
done
rm -rf "$T"
