#!/usr/bin/env python3
"""Condense a rocprofv3 kernel trace (`--kernel-trace --output-format csv`, the *_kernel_trace.csv file) to the LiftSim
kernels' durations per launch size: one CSV row per (kernel, grid size) with calls, median, mean, min and max in µs.

    python scripts/liftsim_trace_stats.py TRACE.csv [--out FILE]
"""
import argparse
import csv
import re
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    groups = {}
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            m = re.search(r"(liftsim_\w+_kernel)", r["Kernel_Name"])
            if not m:
                continue
            envs = int(r["Grid_Size_X"] if "Grid_Size_X" in r else r["Grid_Size"])
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            groups.setdefault((m.group(1), envs), []).append(us)
    rows = [["kernel", "grid_threads", "calls", "median_us", "mean_us", "min_us", "max_us"]]
    for (k, g), v in sorted(groups.items()):
        rows.append([k, g, len(v), "%.1f" % statistics.median(v), "%.1f" % statistics.mean(v), "%.1f" % min(v),
                     "%.1f" % max(v)])
    text = "\n".join(",".join(str(x) for x in r) for r in rows) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
