#!/bin/bash
# Build a variant of the CORE library for A/B runs (the dry-air sweeps live in tpsrhs.hip): that unit is recompiled with extra
# flags and linked with the other core objects of the regular build into tps_amd/csrc/_ab/<name>/libtpsrhs.so; run with
# TPSRHS_LIB=$PWD/tps_amd/csrc/_ab/<name>/libtpsrhs.so TPSRHS_FAMILY_PATH=$PWD/tps_amd/csrc (tools/ab_core.sh).
#   tools/build_core_variant.sh <name> "<flags>"
# Needs the objects of the regular build (tps_amd/csrc/_obj): run build() first.
set -e
name=$1; flags=$2
cd "$(dirname "$0")/../tps_amd/csrc"
mkdir -p _ab/$name
others=""
for u in *.hip; do
  case $u in plasma_*|tpsrhs.hip) continue;; esac
  [ -f _obj/${u%.hip}.o ] || { echo "no object of $u: run build() first" >&2; exit 1; }
  others="$others _obj/${u%.hip}.o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags -c tpsrhs.hip -o _ab/$name/tpsrhs.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o _ab/$name/libtpsrhs.so _ab/$name/tpsrhs.o $others -ldl
echo "built tps_amd/csrc/_ab/$name/libtpsrhs.so"
