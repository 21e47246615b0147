#!/usr/bin/env python3
"""Per-kernel statistics from a rocprofv3 --kernel-trace database (rocpd SQLite) as CSV:

    python scripts/metalm_trace_stats.py <results.db> > profiles/metalm/kernel_stats.csv

One line per (kernel, grid in threads, LDS bytes, registers): calls, mean / min / max duration in microseconds."""
import collections
import sqlite3
import sys


def main(path):
    c = sqlite3.connect(path)
    agg = collections.OrderedDict()
    names = dict(c.execute("select id, display_name from kernel_symbols"))
    for kid, gx, lds, vgpr, sgpr, dur in c.execute(
            "select kernel_id, grid_x, lds_size, vgpr_count, sgpr_count, duration from kernels order by start"):
        name = names.get(kid, str(kid)).split("(")
        name = name[1].split("::")[-1] if name[0] == "" else name[0]          # "(anonymous namespace)::k(...)" -> k
        agg.setdefault((name, gx, lds, vgpr, sgpr), []).append(dur / 1e3)
    print("kernel,grid_x,lds_bytes,vgpr,sgpr,calls,mean_us,min_us,max_us")
    for (name, gx, lds, vgpr, sgpr), v in agg.items():
        print("%s,%d,%d,%d,%d,%d,%.2f,%.2f,%.2f" % (name, gx, lds, vgpr, sgpr, len(v), sum(v) / len(v), min(v), max(v)))


if __name__ == "__main__":
    main(sys.argv[1])
