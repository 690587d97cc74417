#!/usr/bin/env python3
"""Time of the principal-component fit (dca_pca_fit) and of the projection entry (dca_pca_project); prints ONE JSON line.

Config D's shape -- the alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21, de-duplicated) under its weights -- for
k = 2 and k = 10 components (b = 10 and 18 vectors in the block).  One iteration of the fit applies the covariance to the block
once: one launch of the tag "pca_project", one of "pca_back" (slab sums, column sums and their reduction; the frequencies at the
start of a fit are one more launch on a single column) and the launches of "pca_small" (b x b products, rotations).  Reported
per k: ms per launch of each, the small kernels' ms per iteration, the host's ms per iteration (wall time of the call minus
the device time: the b x b eigenproblems, the copies and the waits between them), the iterations, whether they met the
tolerance (the fit is capped at --max_iterations: the time per iteration does not depend on it), ms per fit and ms for
projecting 10 000 queries.  The yardstick from the same run: the pair counts of the mean-field model ("mf_counts", through
dca_alignment_statistics).  The alarm: one application of the operator at k = 2 (project + back-project, b = 10; 5.25e9
predicated f64 adds) should not take longer than mf_counts (6.25e9 irregular LDS adds).

    python tools/pca_timing.py [--max_iterations 200] [--small]
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
from tools.gen_msa import dedup, generate  # noqa: E402


def fit_leg(ctx, k, max_iterations, Q):
    ctx.pca_fit(k, 1e-10, 2, 0)                 # warm-up: allocations
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    fit = ctx.pca_fit(k, 1e-10, max_iterations, 0)
    wall = (time.perf_counter() - t0) * 1e3
    it = max(int(fit["iterations"]), 1)
    (pm, pn), (bm, bn), (sm, _sn) = (ctx.kernel_time(t) for t in ("pca_project", "pca_back", "pca_small"))
    leg = dict(b=min(ctx.L * ctx.q, k + 8), iterations=it, converged=bool(fit["converged"]),
               worst_residual_over_lambda1=float("%.3g" % (fit["residuals"].max() / fit["eigenvalues"][0])),
               ms_per_pca_project=round(pm / max(pn, 1), 3), ms_per_pca_back=round(bm / max(bn, 1), 3),
               pca_small_ms_per_iteration=round(sm / it, 3), host_ms_per_iteration=round((wall - pm - bm - sm) / it, 3),
               ms_per_fit=round(wall, 3))
    ctx.pca_project(fit["components"], fit["offsets"], Q[:64])      # warm-up
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    ctx.pca_project(fit["components"], fit["offsets"], Q)
    leg["project_queries"] = dict(n=int(Q.shape[0]), call_ms=round((time.perf_counter() - t0) * 1e3, 3),
                                  kernel_ms=round(ctx.kernel_time("pca_project")[0], 3))
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max_iterations", type=int, default=200)
    ap.add_argument("--small", action="store_true", help="L = 100, N = 10 000 instead of config D's shape")
    a = ap.parse_args()
    q = 21
    L, N0 = (100, 10000) if a.small else (500, 50000)
    X = dedup(generate(L, N0, q, 2024))
    N = int(X.shape[0])
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.set_profiling(True)
    ctx.alignment_statistics()                  # warm-up: allocations
    ctx.reset_kernel_times()
    ctx.alignment_statistics()
    counts_ms = ctx.kernel_time("mf_counts")[0]
    rng = np.random.default_rng(7)
    Q = X[rng.integers(0, N, size=10000)].copy()
    flip = rng.random(Q.shape) < 0.15
    Q[flip] = rng.integers(0, q, size=int(flip.sum()), dtype=np.uint8)
    out = dict(q=q, L=L, N=N, max_iterations=a.max_iterations, mf_counts_ms=round(counts_ms, 3))
    for k in (2, 10):
        out["k%d" % k] = fit_leg(ctx, k, a.max_iterations, Q)
    op = out["k2"]["ms_per_pca_project"] + out["k2"]["ms_per_pca_back"]
    out["operator_ms_k2"] = round(op, 3)
    out["operator_vs_mf_counts"] = round(op / counts_ms, 3) if counts_ms > 0 else None
    out["alarm"] = bool(counts_ms > 0 and op > counts_ms)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
