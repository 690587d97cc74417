#!/usr/bin/env python3
"""Cost of one decimation at config D's size and the generative quality of a sparse run; prints ONE JSON line.

Cost: a float32 model with L = 500, q = 21 (random x and alignment, as tools/boltzmann_timing.py), n chains and k sweeps per
iteration.  Reported from HIP events of the same run: gauge_ms (dca_plm_zero_sum_gauge, tag "gauge"), sample_ms (the k sweeps of
one iteration, tag "sample", median over the timed iterations), bm_decimate_ms (one dca_plm_bm_decimate removing 1 % of the active
elements: score, selection and apply, with the host's part of the selection in between; tag "bm_decimate"), its wall-clock time,
and bm_decimate_over_sample.

Quality (skipped with --no_quality): PlmDCA.decimate_boltzmann to density 0.1 on a protein fixture of tests/golden/data.
Reported: the Pearson correlation of the connected correlations before the first decimation and after the last round, the
number of rounds and iterations, and the fraction of the dense model's L strongest pairs (Frobenius norm of the zero-sum-gauge
blocks of the pseudo-likelihood fit the run starts from) that keep at least one active element.

    python tools/decimation_timing.py [--chains 10000] [--sweeps 10] [--iterations 3] [--fixture PF02826.faa] [--drop_fraction 0.1]
        [--warmup_iterations 100] [--max_iterations_per_round 20] [--quality_chains 1000] [--verbose] [--no_quality] [--no_cost]
"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402
from pydca_amd.plmdca.plmdca import PlmDCA  # noqa: E402


def cost(a):
    L, q = 500, 21
    rng = np.random.default_rng(2024)
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.plm_zero_sum_gauge()                        # warm-up (first launches)
    ctx.set_profiling(True)
    ctx.plm_zero_sum_gauge()
    gauge = ctx.kernel_time("gauge")[0]
    ctx.set_profiling(False)
    ctx.plm_bm_begin(a.chains, a.sweeps, 0, seed=1, eta_h=0.05, eta_J=0.05, mu_h=1e-4, mu_J=1e-4, pseudocount=1.0 / 64)
    ctx.plm_bm_iterate(1)
    ctx.plm_bm_decimate(0)                          # warm-up of the score launch
    ctx.set_profiling(True)
    sample = []
    for _ in range(a.iterations):
        ctx.reset_kernel_times()
        ctx.plm_bm_iterate(1)
        ms, launches = ctx.kernel_time("sample")
        assert launches == a.sweeps
        sample.append(ms)
    total = L * (L - 1) // 2 * q * q
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    info = ctx.plm_bm_decimate(total // 100)
    wall = (time.perf_counter() - t0) * 1e3
    dec, launches = ctx.kernel_time("bm_decimate")
    assert launches == 1 and info["removed"] == total // 100
    ctx.plm_bm_end()
    ctx.close()
    s = float(np.median(sample))
    return dict(L=L, q=q, chains=a.chains, sweeps=a.sweeps, iterations=a.iterations, removed=int(info["removed"]),
                gauge_ms=round(gauge, 3), sample_ms=round(s, 3), bm_decimate_ms=round(dec, 3), bm_decimate_wall_ms=round(wall, 3),
                bm_decimate_over_sample=round(dec / s, 5))


def quality(a):
    path = os.path.join(ROOT, "tests", "golden", "data", a.fixture)
    t0 = time.perf_counter()
    inst = PlmDCA(path, "protein")
    ctx = inst._fitted_context()
    ctx.plm_lbfgs_end()
    ctx.plm_zero_sum_gauge()
    L, q = inst.sequences_len, 21
    J = ctx.plm_get_x(np.float32)[L * q:].reshape(-1, q, q).astype(np.float64)
    top = np.argsort(-np.sqrt((J * J).sum(axis=(1, 2))), kind="stable")[:L]
    fit = inst.decimate_boltzmann(target_density=0.1, drop_fraction=a.drop_fraction, warmup_iterations=a.warmup_iterations,
                                  max_iterations_per_round=a.max_iterations_per_round, num_chains=a.quality_chains)
    R, H = fit["rounds"], fit["history"]
    kept = fit["mask"][top].any(axis=(1, 2))
    return dict(fixture=a.fixture, L=int(L), q=q, target_density=0.1, density=float(fit["density"]), drop_fraction=a.drop_fraction,
                warmup_iterations=a.warmup_iterations, max_iterations_per_round=a.max_iterations_per_round,
                chains=a.quality_chains, rounds=int(R.shape[0]), total_iterations=int(H.shape[0]), pearson_before_first_decimation=round(float(R[0, 5]), 4),
                pearson_after_last_round=round(float(H[-1, 2]), 4), top_L_pairs_kept=round(float(kept.mean()), 4),
                seconds=round(time.perf_counter() - t0, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10000)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--fixture", default="PF02826.faa")
    ap.add_argument("--drop_fraction", type=float, default=0.1)
    ap.add_argument("--warmup_iterations", type=int, default=100)
    ap.add_argument("--max_iterations_per_round", type=int, default=20)
    ap.add_argument("--quality_chains", type=int, default=1000)
    ap.add_argument("--verbose", action="store_true", help="log every decimation round to stderr")
    ap.add_argument("--no_quality", action="store_true")
    ap.add_argument("--no_cost", action="store_true")
    a = ap.parse_args()
    if a.verbose:
        logging.basicConfig(level=logging.INFO, format="%(asctime)s %(message)s")
    out = {}
    if not a.no_cost:
        out["cost"] = cost(a)
    if not a.no_quality:
        out["quality"] = quality(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
