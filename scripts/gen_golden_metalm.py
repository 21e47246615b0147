#!/usr/bin/env python3
"""Golden MetaLM rows drawn by the unmodified reference (metagym/metalm/metalm.py) -> tests/golden/metalm.npz.

TEST INFRASTRUCTURE; runs only where the reference tree is available (imported through oracle/refstubs, like the other
golden generators). Records:
  - per (configuration, seed): numpy.random.seed(seed); MetaLM(**cfg).data_generator()
  - per batch case: numpy.random.seed(seed); MetaLM(**cfg).batch_generator(B), the global state it leaves behind and the
    next numpy.random.random()
  - the text of one small generate_to_file after numpy.random.seed(seed)
These pin tests/metalm_oracle.py (CPU) and mg_metalm_generate (GPU) bit for bit.

A second, small fixture, tests/golden/metalm_edges.npz, holds the rows of the edge table tests/metalm_cases.py (token and
element-index ranges, the Poisson switch, V at the int32 limit, long elements, mask_ratio and e at their ends), recorded the
same way with `mask_ratio` set on the reference's generator where the case has one.

    python scripts/gen_golden_metalm.py            # both fixtures
    python scripts/gen_golden_metalm.py edges      # one of them: "metalm" or "edges"
"""
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden  # noqa: E402  (reference import shims)
import metalm_cases  # noqa: E402  (the edge table)

D = dict(V=64, n=10, l=64, e=0.10, L=2048)
SEEDS = [0, 1, 7, 2 ** 32 - 1]
CASES = [
    (D, SEEDS),
    (dict(D, V=2, L=1000), SEEDS),                 # no token draws
    (dict(D, n=2, L=1000), SEEDS),                 # no choice draw
    (dict(D, V=50000), SEEDS),
    (dict(D, n=100, l=11.3, L=1500), SEEDS),
    (dict(D, l=1.5, L=500), SEEDS),                # multiplication Poisson
    (dict(D, l=9.99, L=500), SEEDS),
    (dict(D, l=300, L=3000), SEEDS),
    (dict(D, L=2), SEEDS),
    (dict(D, e=0.999, L=1000), SEEDS),
    (dict(D, L=65536), [3]),
]
BATCHES = [(D, 5, 4), (dict(D, V=5, n=3, l=12.5, L=700), 2 ** 31, 9)]   # (cfg, seed, B)
TEXT = (dict(V=8, n=3, l=4, e=0.3, L=20), 11, 3)


def write_metalm(ref):
    out = {"numpy_version": np.str_(np.__version__)}
    rows = []
    for ci, (cfg, seeds) in enumerate(CASES):
        for s in seeds:
            np.random.seed(s)
            f, lb = ref.MetaLM(**cfg).data_generator()
            out["row_%d_%d_features" % (ci, s)] = f.astype(np.int32)
            out["row_%d_%d_labels" % (ci, s)] = lb.astype(np.int32)
            rows.append([ci, s])
    out["cases"] = np.str_(json.dumps([c for c, _ in CASES]))
    out["rows"] = np.asarray(rows, np.int64)
    for bi, (cfg, s, B) in enumerate(BATCHES):
        np.random.seed(s)
        f, lb = ref.MetaLM(**cfg).batch_generator(B)
        st = np.random.get_state()
        out["batch_%d_features" % bi] = f.astype(np.int32)
        out["batch_%d_labels" % bi] = lb.astype(np.int32)
        out["batch_%d_key" % bi] = st[1]
        out["batch_%d_pos" % bi] = np.int64(st[2])
        out["batch_%d_next_random" % bi] = np.float64(np.random.random())
    out["batches"] = np.str_(json.dumps([[c, s, B] for c, s, B in BATCHES]))
    cfg, s, B = TEXT
    np.random.seed(s)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "out.txt")
        with open(path, "w") as fh:                   # the reference writes to an open text file as it is
            ref.MetaLM(**cfg).generate_to_file(B, fh)
        out["text"] = np.str_(open(path).read())
    out["text_case"] = np.str_(json.dumps([cfg, s, B]))
    dst = os.path.join(ROOT, "tests", "golden", "metalm.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


def write_edges(ref):
    out = {"numpy_version": np.str_(np.__version__)}
    rows = []
    for ci, _, cfg, s in metalm_cases.table_rows():
        gen = ref.MetaLM(**metalm_cases.ctor_kwargs(cfg))
        gen.mask_ratio = metalm_cases.mask_ratio(cfg)
        np.random.seed(s)
        f, lb = gen.data_generator()
        out["row_%d_%d_features" % (ci, s)] = f.astype(np.int32)
        out["row_%d_%d_labels" % (ci, s)] = lb.astype(np.int32)
        rows.append([ci, s])
    out["cases"] = np.str_(json.dumps([[name, cfg] for name, cfg, _ in metalm_cases.CASES]))
    out["rows"] = np.asarray(rows, np.int64)
    dst = os.path.join(ROOT, "tests", "golden", "metalm_edges.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


def main():
    which = sys.argv[1:] or ["metalm", "edges"]
    assert set(which) <= {"metalm", "edges"}, which
    gen_golden._import_reference()
    import metagym.metalm as ref
    if "metalm" in which:
        write_metalm(ref)
    if "edges" in which:
        write_edges(ref)


if __name__ == "__main__":
    main()
