#!/usr/bin/env python3
"""Time of the Hopfield-Potts fit (dca_mf_hopfield_fit) by stage; prints ONE JSON line.

Config D's shape -- the alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21, de-duplicated; n = L (q - 1) = 10 000) under
its weights -- for p = 32 (16 patterns of either end, blocks of 24 vectors) and p = 128 (64 of either end, blocks of 72).
Reported per p: ms for the per-site factors plus the whitening ("hopfield_whiten"), for the inverse ("mf_inverse"), per launch
of the operator kernel ("hopfield_apply"), the small kernels' ms per iteration ("pca_small"), the host's ms per iteration (wall
time of the call minus the device time: the b x b eigenproblems, the copies and the waits between them), the iterations of
either end and whether they met the tolerance (the fit is capped at --max_iterations: the time per iteration does not depend on
it), the assembly ("hopfield_assemble") and the whole call.  The yardsticks from the same run: a device-to-device copy of the
same n^2 doubles (the operator kernel reads that much once per application) and dca_mf_run.  The alarm: one application of the
operator at p = 128 should not take longer than 2 copies of the matrix (a copy reads and writes the n^2 doubles, the operator
reads them once, so half a copy is the HBM time of the read itself and 2 copies a quarter of that rate).

    python tools/hopfield_timing.py [--max_iterations 100] [--small]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402
from tools.gen_msa import dedup, generate  # noqa: E402

TAGS = ("hopfield_whiten", "mf_inverse", "hopfield_apply", "pca_small", "hopfield_assemble")


def copy_ms(count):
    a = torch.empty(count, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    b.copy_(a)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    return best


def fit_leg(ctx, theta, per_end, max_iterations):
    ctx.mf_hopfield_fit(theta, num_attractive=per_end, num_repulsive=per_end, max_iterations=1)       # warm-up: allocations
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    fit = ctx.mf_hopfield_fit(theta, num_attractive=per_end, num_repulsive=per_end, max_iterations=max_iterations)
    wall = (time.perf_counter() - t0) * 1e3
    ms = {t: ctx.kernel_time(t) for t in TAGS}
    its = sum(fit["iterations"])
    device = sum(v[0] for v in ms.values())
    return dict(per_end=per_end, b=per_end + 8, iterations=list(fit["iterations"]), converged=list(fit["converged"]),
                worst_residual=float("%.3g" % fit["residuals"].max()), lambda_max=float("%.6g" % fit["eigenvalues"][0]),
                lambda_min=float("%.6g" % fit["eigenvalues"][per_end]),
                factor_and_whiten_ms=round(ms["hopfield_whiten"][0], 3), inverse_ms=round(ms["mf_inverse"][0], 3),
                ms_per_apply=round(ms["hopfield_apply"][0] / max(ms["hopfield_apply"][1], 1), 4), applies=ms["hopfield_apply"][1],
                pca_small_ms_per_iteration=round(ms["pca_small"][0] / its, 3), host_ms_per_iteration=round((wall - device) / its, 3),
                assemble_ms=round(ms["hopfield_assemble"][0], 3), ms_per_fit=round(wall, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max_iterations", type=int, default=100)
    ap.add_argument("--small", action="store_true", help="L = 100, N = 10 000 instead of config D's shape")
    a = ap.parse_args()
    q, theta = 21, 0.5
    L, N0 = (100, 10000) if a.small else (500, 50000)
    X = dedup(generate(L, N0, q, 2024))
    n = L * (q - 1)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.mf_run(theta, True)                        # warm-up: allocations
    t0 = time.perf_counter()
    ctx.mf_run(theta, True)
    mf_run_ms = (time.perf_counter() - t0) * 1e3
    ctx.set_profiling(True)
    out = dict(q=q, L=L, N=int(X.shape[0]), n=n, max_iterations=a.max_iterations, mf_run_ms=round(mf_run_ms, 2),
               copy_n2_doubles_ms=round(copy_ms(n * n), 4))
    for p in (32, 128):
        out["p%d" % p] = fit_leg(ctx, theta, p // 2, a.max_iterations)
    apply_ms = out["p128"]["ms_per_apply"]
    out["apply_over_copy"] = round(apply_ms / out["copy_n2_doubles_ms"], 3)
    out["fit_over_mf_run"] = {k: round(out[k]["ms_per_fit"] / mf_run_ms, 2) for k in ("p32", "p128")}
    out["alarm"] = bool(apply_ms > 2.0 * out["copy_n2_doubles_ms"])
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
