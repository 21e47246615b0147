"""Phase timeline of the one-wave Quadrotor step (STEP_STOCK_SHADOW).

    METAGYM_HIP_LIB=<lib> python scripts/quad_phase_timeline.py

The script builds the headline batch (hovering_control, 65 536 envs, fused auto-reset, U(0.1, 15) actions), rolls it `PREROLL` steps
into its steady state, times `STEPS` eager env.step() calls with HIP events and prints one JSON line.

With a diagnostic library (built with -DMG_QUAD_PHASE_STAMPS, e.g. `scripts/build_variant.sh stamps WORK
-fno-slp-vectorize -DMG_QUAD_PHASE_STAMPS`) it also reads the per-wave stamps of `SAMPLES` single launches and
reduces each launch (100 MHz ticks, reported in us) to:
  dispatch skew  max - min of the wave entry times
  load phase     median over waves of entry -> state loaded
  compute        median of state loaded -> sub-step 10 done
  store issue    median of sub-step 10 done -> obs stores issued
  span           first entry -> last obs store issued
and counts the waves that took the fast path's fallback. The span set against the kernel's duration from
`rocprofv3 --kernel-trace --stats` of the same run is the dispatch plus the final store drain.
"""
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import metagym_amd  # noqa: E402
from metagym_amd import _lib  # noqa: E402

N = int(os.environ.get("QN", "65536"))
PREROLL = int(os.environ.get("PREROLL", "1000"))
STEPS = int(os.environ.get("STEPS", "1000"))
SAMPLES = int(os.environ.get("SAMPLES", "20"))
SLOTS, MAX_WAVES = 8, 4096


def stamps_reader():
    lib = _lib.load()
    try:
        fn = lib.mg_quadrotor_phase_stamps
    except AttributeError:
        return None
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    waves = (N + 63) // 64
    buf = (ctypes.c_uint64 * (waves * SLOTS))()

    def read():
        torch.cuda.synchronize()
        _lib.check(fn(ctypes.addressof(buf), waves), "mg_quadrotor_phase_stamps")
        return [list(buf[w * SLOTS:(w + 1) * SLOTS]) for w in range(waves)]
    return read


def reduce_launch(rows):
    us = 0.01   # one tick of the 100 MHz wall clock
    t0 = min(r[0] for r in rows)
    return {
        "skew_us": (max(r[0] for r in rows) - t0) * us,
        "load_us": statistics.median(r[1] - r[0] for r in rows) * us,
        "compute_us": statistics.median(r[2] - r[1] for r in rows) * us,
        "store_issue_us": statistics.median(r[4] - r[2] for r in rows) * us,
        "span_us": (max(r[4] for r in rows) - t0) * us,
        "last_load_done_us": (max(r[1] for r in rows) - t0) * us,
        "first_compute_done_us": (min(r[2] for r in rows) - t0) * us,
        "fallback_waves": sum(1 for r in rows if r[7] >> 32),
        "xccs": len({r[6] >> 32 & 0xf for r in rows}),
    }


def run(read):
    env = metagym_amd.make("quadrotor-v0", num_envs=N, task="hovering_control", nt=1000, auto_reset=True, seed=1)
    env.reset(seed=0)
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    acts = [a for a in torch.rand(8, N, 4, device="cuda", generator=g) * 14.9 + 0.1]
    for i in range(PREROLL):
        env.step(acts[i % 8])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(STEPS):
        env.step(acts[i % 8])
    e1.record()
    torch.cuda.synchronize()
    out = {"lib": os.path.basename(_lib.lib_path()), "n": N,
           "us_per_step": e0.elapsed_time(e1) / STEPS * 1e3}
    if read is not None:
        per = []
        for i in range(SAMPLES):
            env.step(acts[i % 8])
            per.append(reduce_launch(read()))
        out["timeline"] = {k: statistics.median(p[k] for p in per) for k in per[0]}
        out["timeline"]["fallback_waves_total"] = sum(p["fallback_waves"] for p in per)
    print(json.dumps(out), flush=True)


def main():
    read = stamps_reader()
    run(read)


if __name__ == "__main__":
    main()
