"""Duration and launch-to-launch gap of quadrotor_step_kernel from a rocprofv3 kernel trace.

    python scripts/quad_trace_gaps.py LABEL DIR    (DIR holds the *_kernel_trace.csv of `rocprofv3 --kernel-trace`)

A store policy can move time between the kernel's tail and the gap in front of the next launch, so the figure to judge
is their sum. A gap is next launch's start minus this launch's end, taken only between step launches that directly follow
each other in the trace; gaps above GAP_MAX_US (the host fell behind: warm-up, a host synchronisation) are left out and counted.
Prints one JSON line.
"""
import csv
import glob
import json
import os
import statistics
import sys

GAP_MAX_US = float(os.environ.get("GAP_MAX_US", "20"))


def main():
    label, d = sys.argv[1], sys.argv[2]
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "quadrotor_step_kernel" in r["Kernel_Name"]))
    rows.sort()
    dur = [(e - s) * 1e-3 for s, e, q in rows if q]
    gaps, left_out = [], 0
    for (s0, e0, q0), (s1, e1, q1) in zip(rows, rows[1:]):
        if q0 and q1:
            g = (s1 - e0) * 1e-3
            if g <= GAP_MAX_US:
                gaps.append(g)
            else:
                left_out += 1
    out = {"label": label, "launches": len(dur), "duration_avg_us": statistics.fmean(dur), "duration_median_us": statistics.median(dur),
           "duration_min_us": min(dur), "gaps": len(gaps), "gaps_left_out": left_out, "gap_avg_us": statistics.fmean(gaps),
           "gap_median_us": statistics.median(gaps)}
    out["duration_plus_gap_us"] = out["duration_avg_us"] + out["gap_avg_us"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
