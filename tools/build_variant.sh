#!/bin/bash
# tools/build_variant.sh NAME [extra hipcc flags...] -> air_rs_amd/lib/variants/libadsb_hip_NAME.so
set -euo pipefail
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p air_rs_amd/lib/variants
SRC=air_rs_amd/csrc
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -Wno-unused-function "$@" \
    $(sed "s|^|$SRC/|" $SRC/sources.list) \
    -o air_rs_amd/lib/variants/libadsb_hip_$name.so
echo built $name
