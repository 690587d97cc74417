#!/usr/bin/env python3
"""Time of one Boltzmann-learning iteration at config D's size; prints ONE JSON line.

dca_plm_bm_iterate on a float32 model with L = 500, q = 21 (random x and alignment, as tools/sampling_timing.py), n chains and
k sweeps per iteration.  Reported: the device time per iteration of the "sample" stage (the k sweeps) and of the "bm_stats"
stage (model counts, update and record: three launches), from HIP events, median over the timed iterations; the
wall-clock time per iteration; and bm_stats as a fraction of the sweeps.

    python tools/boltzmann_timing.py [--chains 10000] [--sweeps 10] [--iterations 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10000)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3)
    a = ap.parse_args()
    L, q = 500, 21
    rng = np.random.default_rng(2024)
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.plm_bm_begin(a.chains, a.sweeps, 0, seed=1, eta_h=0.05, eta_J=0.05, mu_h=1e-4, mu_J=1e-4, pseudocount=1.0 / 64)
    ctx.plm_bm_iterate(1)                           # warm-up (first launches)
    ctx.set_profiling(True)
    sample, stats, wall = [], [], []
    for _ in range(a.iterations):
        ctx.reset_kernel_times()
        t0 = time.perf_counter()
        ctx.plm_bm_iterate(1)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms, launches = ctx.kernel_time("sample")
        assert launches == a.sweeps
        sample.append(ms)
        ms, launches = ctx.kernel_time("bm_stats")
        assert launches == 1
        stats.append(ms)
    ctx.plm_bm_end()
    ctx.close()
    s, b = float(np.median(sample)), float(np.median(stats))
    print(json.dumps(dict(L=L, q=q, chains=a.chains, sweeps=a.sweeps, iterations=a.iterations, sample_ms=round(s, 3),
                          bm_stats_ms=round(b, 3), iteration_wall_ms=round(float(np.median(wall)), 3),
                          bm_stats_over_sample=round(b / s, 4))))


if __name__ == "__main__":
    main()
