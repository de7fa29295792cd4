#!/bin/bash
# usage: mkvar.sh NAME FLAGS...
set -e
cd "$(dirname "$0")/../.."
name=$1; shift
SRC=air_rs_amd/csrc
FILES=$(sed "s|^|$SRC/|" $SRC/sources.list)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -Wall -Wno-unused-function "$@" $FILES -o air_rs_amd/lib/variants/libadsb_hip_$name.so
echo built $name
