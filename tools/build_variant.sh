#!/bin/bash
# Build the GPU library of another git revision as searchlite_amd/lib/libsearchlite_gpu_<tag>.so,
# to time two kernels side by side on ONE box (devices differ by several percent):
#   bash tools/build_variant.sh <git-ref> <tag> [extra compiler flags, e.g. -DSLG_U4_WAVES=5];  SLG_LIB_TAG=<tag> python bench.py ...
set -e
REF=$1; TAG=$2; shift 2; EXTRA="$*"
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TMP=$(mktemp -d /tmp/slg_variant_XXXX)
git -C "$ROOT" archive "$REF" searchlite_amd/csrc include | tar -x -C "$TMP"
cd "$TMP/searchlite_amd/csrc"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Wno-unused-function $EXTRA"
OBJS=""
for kr in 1 2 4 8 16; do
  /opt/rocm/bin/hipcc $FLAGS -DSLG_INST_KREGS=$kr -c slg_score_inst.hip -o k$kr.o &
  OBJS="$OBJS k$kr.o"
done
# the host units of the revision: every .hip but the score instantiations (one slg_api.hip in older
# revisions, one unit per concern since)
for src in *.hip; do
  [ "$src" = slg_score_inst.hip ] && continue
  /opt/rocm/bin/hipcc $FLAGS -c "$src" -o "${src%.hip}.o" &
  OBJS="$OBJS ${src%.hip}.o"
done
# the plain C++ units build_gpu links (searchlite_amd/build.py); slg_segfile.cpp and the *_capi.cpp files belong to
# the host-only libraries
for src in slg_plan.cpp slg_expand_merge.cpp slg_regex.cpp slg_suggest_host.cpp slg_highlight_host.cpp; do
  [ -f "$src" ] || continue
  /opt/rocm/bin/hipcc $FLAGS -x c++ -c "$src" -o "${src%.cpp}_cpp.o" &
  OBJS="$OBJS ${src%.cpp}_cpp.o"
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$ROOT/searchlite_amd/lib/libsearchlite_gpu_$TAG.so" $OBJS
rm -rf "$TMP"
echo "$ROOT/searchlite_amd/lib/libsearchlite_gpu_$TAG.so"
