#!/bin/bash
# A/B diagnostics: build libkpsim with extra compile flags into tools/ab/<name>.so (objects under /tmp), e.g.
#   tools/build_variant.sh blockscan0 -DKP_TOPO_BLOCK_SCAN=0
set -euo pipefail
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PKG=$ROOT/karpenter-provider-aws_amd
OUT=/tmp/kpvar_$NAME
mkdir -p "$OUT" "$ROOT/tools/ab"
FLAGS="-O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-unused-result -Wno-unused-value -mllvm --amdgpu-sched-strategy=max-ilp $*"
pids=()
FFD="base resv pref pref_resv base_topo resv_topo pref_topo pref_resv_topo"  # and their diagnostic twins (kp_ffd_prof_*)
for f in kp_kernels $(for u in $FFD; do echo kp_ffd_$u kp_ffd_prof_$u; done) kp_consolidate kp_launch; do
  /opt/rocm/bin/hipcc $FLAGS -c -o "$OUT/$f.o" "$PKG/csrc/$f.hip" & pids+=($!)
done
for f in "$PKG"/csrc/kp_host*.cpp; do  # the C-ABI host units
  /opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 $* -x hip -c -o "$OUT/$(basename "$f" .cpp).o" "$f" & pids+=($!)
done
/opt/rocm/bin/hipcc -O3 -std=c++17 -fPIC -c -o "$OUT/kp_ingest.o" "$PKG/csrc/kp_ingest.cpp" & pids+=($!)
for p in "${pids[@]}"; do wait "$p"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o "$ROOT/tools/ab/$NAME.so" "$OUT"/*.o
echo "built tools/ab/$NAME.so"
