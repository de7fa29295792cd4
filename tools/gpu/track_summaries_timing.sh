#!/bin/bash
# GPU box helper: the whole of profiles/track_summaries_timing.txt in one call.  tools/gpu/track_summaries_timing.py
# four times, alternating the parent commit's library ($1: a build of the parent's sources, e.g.
# air_rs_amd/lib/variants/libadsb_hip_parent.so) and this tree's, then rocprofv3 --kernel-trace --stats runs of their
# own (a table update of 64 frames: parent, this build, this build with a reserve; config 4 and the one-aircraft list
# with a reserve, and the latter without) and their per-kernel tables.  Every GPU step has its own time limit and the
# chain stops at the first failure.  Writes track_summaries_timing.txt into the results folder $OUT (default: out).
set -o pipefail
P=${1:?usage: $0 PARENT_LIBRARY}
P=$(readlink -f "$P")
D=${OUT:-out}
mkdir -p $D
OUT=$D/track_summaries_timing.txt
: > $OUT
T="python tools/gpu/track_summaries_timing.py"
parent() { ADSB_HIP_LIB=$P ADSB_HIP_LIB_LENIENT=1 "$@"; }
trace() { # NAME ARGS...: one traced run into $D/trace_NAME
    local name=$1
    shift
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $D/trace_$name -o t -- $T "$@" \
        > $D/trace_$name.log 2>&1 || { tail -20 $D/trace_$name.log; return 1; }
}
parent timeout -k 10 240 $T --out $OUT --label "parent commit's build, run 1" &&
    timeout -k 10 240 $T --out $OUT --label "this build, run 1" &&
    parent timeout -k 10 240 $T --out $OUT --label "parent commit's build, run 2" &&
    timeout -k 10 240 $T --out $OUT --label "this build, run 2" &&
    parent trace parent_small --trace small &&
    trace small --trace small &&
    trace small_reserved --trace small --reserve &&
    trace config4_reserved --trace config4 --reserve &&
    trace one_aircraft --trace one-aircraft &&
    trace one_aircraft_reserved --trace one-aircraft --reserve || exit 1
$T --out $OUT \
    --kernel-stats "table updates of 64 frames, parent commit's build, no reserve" $D/trace_parent_small \
    --kernel-stats "table updates of 64 frames, this build, no reserve" $D/trace_small \
    --kernel-stats "table updates of 64 frames, this build, with a reserve" $D/trace_small_reserved \
    --kernel-stats "config 4 through update_launch, this build, with a reserve" $D/trace_config4_reserved \
    --kernel-stats "one aircraft, 65536 frames, this build, no reserve" $D/trace_one_aircraft \
    --kernel-stats "one aircraft, 65536 frames, this build, with a reserve" $D/trace_one_aircraft_reserved
