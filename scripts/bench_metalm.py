#!/usr/bin/env python3
"""meta-lm-v0 throughput on one GPU: one JSON line per workload.

    python scripts/bench_metalm.py [--reps 10] [--warmup 3]

Workloads: seeded B = 65536 and B = 4096 rows of L = 2048 at the reference defaults (V=64, n=10, l=64, e=0.1), and chained
B = 256 (one wave continuing numpy.random's stream). Kernel time comes from HIP events recorded on the launching stream
around `reps` back-to-back calls (seeded calls skip the overflow read, check=False, so nothing synchronises in between;
the chained call synchronises by nature and is timed per call). Bytes written are 8 per token (features + labels, int32);
`hbm_write_fraction` is that rate over the 8.0 TB/s HBM peak (6.3 TB/s is the measured copy ceiling)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def run(name, B, L, reps, warmup, chained):
    import numpy as np
    import torch
    from metagym_amd.metalm import MetaLM
    gen = MetaLM(device="cuda", L=L)
    out = (torch.empty(B, L, dtype=torch.int32, device="cuda"), torch.empty(B, L, dtype=torch.int32, device="cuda"))
    np.random.seed(0)

    def call(i):
        if chained:
            gen.batch_generator(B, out=out)
        else:
            gen.batch_generator(B, seed=i * B % (2 ** 32 - B), out=out, check=False)

    for i in range(warmup):
        call(i)
    torch.cuda.synchronize()
    st = torch.cuda.current_stream()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(st)
    for i in range(reps):
        call(warmup + i)
    t1.record(st)
    t1.synchronize()
    sec = t0.elapsed_time(t1) / 1e3 / reps
    if not chained:
        assert int(gen.last_overflow.item()) == 2 ** 31 - 1
    tokens = B * L
    return {"workload": name, "batch": B, "L": L, "mode": "chained" if chained else "seeded", "reps": reps,
            "time_ms": sec * 1e3, "tokens_per_s": tokens / sec, "bytes_written": 8 * tokens,
            "write_bytes_per_s": 8 * tokens / sec, "hbm_write_fraction": 8 * tokens / sec / HBM_PEAK,
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for name, B, chained, reps in (("seeded_B65536", 65536, False, a.reps), ("seeded_B4096", 4096, False, a.reps),
                                   ("chained_B256", 256, True, max(1, a.reps // 5))):
        print(json.dumps(run(name, B, 2048, reps, a.warmup, chained)), flush=True)


if __name__ == "__main__":
    main()
