#!/usr/bin/env python3
"""How often the device's log (OCML, what liftsim.hip's normalvariate calls) differs from glibc's (CPython's math.log)
on the arguments normalvariate feeds it, and how often that flips its accept test zz <= -log(u2) (a different draw count).

    python scripts/liftsim_libm_mismatch.py [--n 20000000] [--out FILE]

u1, u2 = random(), 1 - random() from a CPython stream (the 53-bit doubles the env draws); z and zz as Lib/random.py
computes them. torch.log of a float64 CUDA tensor is OCML's log on ROCm, the same function the kernel calls."""
import argparse
import json
import math
import random

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    r = random.Random(12345)
    u1 = np.array([r.random() for _ in range(a.n)])
    u2 = 1.0 - np.array([r.random() for _ in range(a.n)])
    glibc = np.array([math.log(x) for x in u2.tolist()])
    ocml = torch.log(torch.from_numpy(u2).cuda()).cpu().numpy()
    z = random.NV_MAGICCONST * (u1 - 0.5) / u2
    zz = z * z / 4.0
    differ = glibc != ocml
    flips = (zz <= -glibc) != (zz <= -ocml)
    ulps = np.abs(glibc.view(np.int64) - ocml.view(np.int64))
    res = dict(workload="normalvariate_log_ocml_vs_glibc", samples=a.n, log_values_differ=int(differ.sum()),
               differ_rate=float(differ.mean()), max_ulp=int(ulps.max()), accept_test_flips=int(flips.sum()),
               device=torch.cuda.get_device_name())
    print(json.dumps(res))
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
