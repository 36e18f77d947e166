"""Per-call figures of a rocprofv3 trace of tools/face_tower/time_face_tower.py (driven by profile_face_tower.sh): kernel launches of the face
tower per call, their summed durations, and the HIP-event wall time per call the script printed under the tracer.
-> the tail of profiles/face_tower_kernel_stats_b{1,32}.md

    python per_call.py DB CALLS STDOUT"""
import sqlite3
import sys

db, calls, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
c = sqlite3.connect(db)
n, tot = c.execute("select count(*), sum(duration) from kernels where name like '%face_%' or name like '%copy_cols%'").fetchone()
wall = [line.split() for line in open(out) if line.strip()[:1].isdigit()]
print(f"\nper call ({calls} calls traced): **{n / calls:.1f} launches**, **{tot / calls / 1e3:.1f} us of summed kernel time** "
      f"(the kernels of one call run one after the other on one stream)")
for row in wall:
    print(f"HIP-event wall time per call under the tracer, B = {row[0]}: **{float(row[1]) * 1e3:.1f} us**")
