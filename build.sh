#!/bin/bash
# Builds the product library (HIP, gfx950) and the CPU oracle (plain C, test infrastructure).
# Called by __graft_entry__.build(); safe to run by hand.  hipcc cross-compiles without a GPU.
#   air_rs_amd/lib/libadsb_hip.so               the product: ONE i8 scan kernel (floor(sqrt) per sample) + CS16's
#   air_rs_amd/lib/variants/libadsb_hip_ab.so   the same sources with -DADSB_AB_KERNELS=1: also the A/B scan kernels (code, nsq,
#                                               reg) round 3-4 measured against the product's; loaded only by
#                                               tests/test_gpu_ab_kernels.py (one parity smoke each) and tools/gpu/ab.sh
set -euo pipefail
cd "$(dirname "$0")"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
mkdir -p air_rs_amd/lib/variants
SRC=air_rs_amd/csrc
FILES=$(sed "s|^|$SRC/|" $SRC/sources.list) # the library's sources: one list, read by tools/build_variant.sh and tools/gpu/mkvar.sh too
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -pthread -Wall -Wno-unused-function"
# a failed compile must not leave the previous library behind to be reported (and timed) as the new one
rm -f air_rs_amd/lib/libadsb_hip.so air_rs_amd/lib/variants/libadsb_hip_ab.so
$HIPCC $FLAGS $FILES -o air_rs_amd/lib/libadsb_hip.so &
pid_product=$!
$HIPCC $FLAGS -DADSB_AB_KERNELS=1 $FILES -o air_rs_amd/lib/variants/libadsb_hip_ab.so &
pid_ab=$!
gcc -O3 -std=c99 -fPIC -shared -Wall -Wextra oracle/adsb_oracle.c -o oracle/libadsb_oracle.so -lm
# `wait` without arguments returns 0 whatever the jobs returned: wait for each by PID
rc=0
wait $pid_product || rc=$?
wait $pid_ab || rc=$?
[ $rc -eq 0 ] || { echo "build.sh: a hipcc job failed (exit $rc)" >&2; exit $rc; }
test -s air_rs_amd/lib/libadsb_hip.so && test -s air_rs_amd/lib/variants/libadsb_hip_ab.so
echo "built air_rs_amd/lib/libadsb_hip.so air_rs_amd/lib/variants/libadsb_hip_ab.so oracle/libadsb_oracle.so"
