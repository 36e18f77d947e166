#!/bin/bash
# Where the face tower's time goes: rocprofv3 --kernel-trace --stats of tools/face_tower/time_face_tower.py (HIP tower only: 3 warm-up + REPS
# timed calls) at B = 1 and B = 32, summarised per kernel and launch shape by tools/rocprof_summary.py, plus per call: launches, summed kernel
# time, and the HIP-event wall time per call the script printed under the tracer.
# -> profiles/face_tower_kernel_stats_b1.md, profiles/face_tower_kernel_stats_b32.md
set -euo pipefail
R=$(cd "$(dirname "$0")/../.." && pwd)
O=${O:-$R/profiles}
REPS=${REPS:-20}
for B in 1 32; do
    D=$(mktemp -d)
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$D" -o t -- env SIZES=$B REPS=$REPS YARDSTICK=0 python "$R/tools/face_tower/time_face_tower.py" > "$D/stdout.txt" 2>/dev/null
    DB=$(find "$D" -name "*.db" | head -1)
    {
        python "$R/tools/rocprof_summary.py" "$DB" "rocprofv3 --kernel-trace --stats -- env SIZES=$B REPS=$REPS YARDSTICK=0 python tools/face_tower/time_face_tower.py (face tower alone, B = $B faces of 160 x 160)"
        python "$R/tools/face_tower/per_call.py" "$DB" $((REPS + 3)) "$D/stdout.txt"
    } > "$O/face_tower_kernel_stats_b$B.md"
    rm -rf "$D"
done
