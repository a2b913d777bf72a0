#!/usr/bin/env python3
"""Ordered launch list of a rocprofv3 kernel trace, per stream: one line per dispatch with (kernel name, grid, workgroup size),
in enqueue order, streams numbered by first appearance.  Two builds launch the same thing exactly when their lists are equal.

    rocprofv3 --kernel-trace --output-format csv -d out -- python tools/update_fingerprint.py --only ppo/hopper/bf16 --knobs default,38=0,1=0
    python tools/launch_list.py out/*/*_kernel_trace.csv profiles/launches.txt"""
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
key = "Stream_Id" if "Stream_Id" in rows[0] else "Queue_Id"
rows.sort(key=lambda r: int(r["Dispatch_Id"]))
streams = {}
for r in rows:
    name = re.sub(r"^void ", "", r["Kernel_Name"]).replace("(anonymous namespace)::", "")
    grid = "x".join(r[f"Grid_Size_{a}"] for a in "XYZ")
    wg = "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")
    streams.setdefault(r[key], []).append(f"{name}  grid {grid}  wg {wg}")
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
print(f"# {len(rows)} dispatches on {len(streams)} streams (by {key}, numbered by first appearance)", file=out)
for i, (sid, lst) in enumerate(streams.items()):
    print(f"## stream {i}: {len(lst)} dispatches", file=out)
    for line in lst:
        print(line, file=out)
