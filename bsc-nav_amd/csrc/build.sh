#!/bin/bash
# Builds libbscnav.so (gfx950 only) next to the Python package.  -ffp-contract=off: every fma in the
# geometry chain is explicit (__fma_rn); nothing else may be fused (bit-exact parity with the reference).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
# BSC_OUT / BSC_OBJ: an A/B build (other BSC_EXTRA_FLAGS) beside the product; python picks it up through BSC_LIB_PATH
OUT="${BSC_OUT:-$HERE/../libbscnav.so}"
OBJ="${BSC_OBJ:-$HERE/_obj}"
mkdir -p "$OBJ"
FLAGS="${BSC_EXTRA_FLAGS} --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result"
ROCM="${ROCM_PATH:-$(dirname "$(dirname "$(readlink -f "$(command -v hipcc)")")")}"
# *.cpp: host-only C++ for plain g++ — host_rng (NumPy's MT19937 shuffle restated, AVX2 paths behind a runtime check), ctx_mem
# (the ledger of a context's device / pinned-host memory: the declarations of the HIP runtime API, no device code)
SOURCES="host_rng.cpp ctx_mem.cpp prims.hip radix.hip ingest.hip dense.hip flush.hip store_compact.hip surprise.hip cosine_scan.hip localize.hip score_map.hip topdown.hip render.hip cluster.hip frontier.hip encoder_ops.hip encoder_gemm.hip capi.hip"
pids=()
objs=()
for f in $SOURCES; do
  src="$HERE/$f"; obj="$OBJ/${f%.*}.o"
  objs+=("$obj")
  if [ ! -f "$obj" ] || [ "$src" -nt "$obj" ] || [ "$HERE/bsc_internal.h" -nt "$obj" ] || [ "$HERE/ctx_mem.h" -nt "$obj" ] || [ "$HERE/ingest_mail.h" -nt "$obj" ] || [ "$HERE/localize_cand.h" -nt "$obj" ] || [ "$HERE/att_ticket.h" -nt "$obj" ] || [ "$HERE/gemm_split_plan.h" -nt "$obj" ] || [ "$HERE/geometry_dev.h" -nt "$obj" ] || [ "$HERE/ray_walk.h" -nt "$obj" ] || [ "$HERE/../../include/bscnav.h" -nt "$obj" ]; then
    case "$f" in
      *.cpp) ( g++ -O3 -std=c++17 -fPIC -Wall -D__HIP_PLATFORM_AMD__ -I"$ROCM/include" -I"$HERE/../../include" -c "$src" -o "$obj" ) & ;;
      *) ( hipcc $FLAGS -c "$src" -o "$obj" ) & ;;
    esac
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $OUT"
