#!/usr/bin/env python3
"""Time of the autoregressive model (ardca.hip) at config D's shape; prints ONE JSON line.

A random alignment of N = 50 000 sequences, L = 500, q = 21 (unit weights), lambda_h = 1e-6, lambda_J = 1e-2:
  eval_ms            one dca_ar_gradient (wall, median), and its device time split into the "ar_logits" and "ar_grad" stages
  fit20_s            dca_ar_fit with max_iterations = 20 from x = 0 (the library's own clock)
  logp_ms            dca_ar_log_probabilities of 50 000 random queries under the fitted x (wall: upload, kernels, copy back)
  sample_ms          dca_ar_sample of 10 000 sequences (wall) and the "ar_sample" kernel time

    python tools/ardca_timing.py [--N 50000] [--L 500] [--queries 50000] [--samples 10000] [--reps 3]
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
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--q", type=int, default=21)
    ap.add_argument("--queries", type=int, default=50000)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = rng.integers(0, a.q, size=(a.N, a.L)).astype(np.uint8)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, a.q)
    ctx.set_weights(np.ones(a.N))
    ctx.ar_configure(1e-6, 1e-2)
    ctx.set_profiling(True)
    ctx.ar_gradient()                                   # warm-up
    wall, lg, gr = [], [], []
    for _ in range(a.reps):
        ctx.reset_kernel_times()
        t0 = time.perf_counter()
        ctx.ar_gradient()
        wall.append((time.perf_counter() - t0) * 1e3)
        lg.append(ctx.kernel_time("ar_logits")[0])
        gr.append(ctx.kernel_time("ar_grad")[0])
    ctx.set_profiling(False)
    ctx.ar_init_x()
    st = ctx.ar_fit(a.iterations, 0.0)
    Q = rng.integers(0, a.q, size=(a.queries, a.L)).astype(np.uint8)
    ctx.ar_log_probabilities(Q[:1000])
    t0 = time.perf_counter()
    ctx.ar_log_probabilities(Q)
    logp_ms = (time.perf_counter() - t0) * 1e3
    ctx.set_profiling(True)
    ctx.ar_sample(64)
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    ctx.ar_sample(a.samples, seed=1)
    sample_ms = (time.perf_counter() - t0) * 1e3
    sample_kernel_ms = ctx.kernel_time("ar_sample")[0]
    values = a.N * a.L * (a.L - 1) / 2 * a.q
    out = dict(tool="ardca_timing", N=a.N, L=a.L, q=a.q, eval_ms=float(np.median(wall)), ar_logits_ms=float(np.median(lg)),
               ar_grad_ms=float(np.median(gr)), logits_values_per_s=values / (np.median(lg) * 1e-3),
               fit_iterations=st["iterations"], fit_evaluations=st["evaluations"], fit_status=st["status"], fit20_s=st["seconds"],
               queries=a.queries, logp_ms=logp_ms, samples=a.samples, sample_ms=sample_ms, sample_kernel_ms=sample_kernel_ms)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
