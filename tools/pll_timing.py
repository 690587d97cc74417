#!/usr/bin/env python3
"""Time of the pseudo-log-likelihood entries at config D's size; prints ONE JSON line.

plm: dca_plm_pseudo_likelihood on a float32 model with L = 500, q = 21 (random x) for 50 000 random query sequences;
mf: dca_mf_pseudo_likelihood under the mean-field couplings of a random L = 500, q = 21 alignment for the same queries.
Reported per leg: the device time of the "pll" stage (site kernel + finish kernel, HIP events; median over the repetitions),
the wall time of the whole call (upload of the queries, site-major copy, kernels, copy back; median) and the coupling values
read per second of the stage (n * L * (L - 1) * q).

    python tools/pll_timing.py [--queries 50000] [--reps 5]
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


def timed(ctx, fn, X, reps):
    fn(X)                                   # warm-up (first launch, device allocations)
    dev, wall = [], []
    for _ in range(reps):
        ctx.reset_kernel_times()
        t0 = time.perf_counter()
        fn(X)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ctx.kernel_time("pll")[0])
    return float(np.median(dev)), float(np.median(wall))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    L, q = 500, 21
    rng = np.random.default_rng(2024)
    Q = rng.integers(0, q, size=(a.queries, L), dtype=np.uint8)
    values = a.queries * L * (L - 1) * q

    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.set_profiling(True)
    plm_dev, plm_wall = timed(ctx, ctx.plm_pseudo_likelihood, Q, a.reps)
    ctx.close()

    mctx = _lib.Context(0, _lib.DCA_F64)
    mctx.set_msa(rng.integers(0, q, size=(2000, L), dtype=np.uint8), q)
    mctx.compute_weights(0.8, _lib.DCA_F64)
    mctx.mf_corr_mat(0.5, want=False)
    mctx.mf_couplings(want=False)
    mctx.set_profiling(True)
    mf_dev, mf_wall = timed(mctx, mctx.mf_pseudo_likelihood, Q, a.reps)
    mctx.close()

    print(json.dumps(dict(L=L, q=q, queries=a.queries, values=values,
                          plm_f32=dict(pll_ms=round(plm_dev, 3), call_ms=round(plm_wall, 3),
                                       values_per_s=float("%.4g" % (values / plm_dev * 1e3))),
                          mf=dict(pll_ms=round(mf_dev, 3), call_ms=round(mf_wall, 3),
                                  values_per_s=float("%.4g" % (values / mf_dev * 1e3))))))


if __name__ == "__main__":
    main()
