"""Kernel times of wms_batch_kernel from a rocprofv3 kernel trace CSV of scripts/wms_kernel_bench.py CALLS: per size the median."""
import csv
import glob
import sys

import numpy as np

calls, warm, sizes = int(sys.argv[2]), 3, (150, 586, 2048)
per = warm + 2 * calls + 1   # (+1: the debug-state call)
rows = []
for path in glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True):
    with open(path) as f:
        for r in csv.DictReader(f):
            if "wms_batch_kernel" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
rows.sort()
print(f"{len(rows)} dispatches of wms_batch_kernel (expected {per * len(sizes)})")
for k, n in enumerate(sizes):
    blk = rows[k * per + warm:k * per + warm + 2 * calls]
    if not blk:
        continue
    d = np.array([e - s for s, e in blk]) / 1e3
    a, b = d[:calls], d[calls:]
    print(f"n={n}: kernel time median run A {np.median(a):.1f} us, run B {np.median(b):.1f} us (min {d.min():.1f}, max {d.max():.1f})")
