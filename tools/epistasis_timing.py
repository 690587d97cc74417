#!/usr/bin/env python3
"""Time of the arDCA epistatic contact scores (ar_epistasis.hip) against the brute force; prints ONE JSON line.

A random model at L = 500, q = 21 (normal couplings and fields of the given scale) and a random wild type:
  scores_ms          one dca_ar_epistatic_scores with APC (wall, median: wild-type pass, table, scoring, copy of the scores)
  kernel_ms          the device time of that call under the "ar_epistasis" tag (the four launches of ar_epistasis.hip)
  fma, tfma_per_s    the fused multiply-adds of the pair products, q^3 sum_l l (L - 1 - l), and their rate over kernel_ms
  brute_sample_ms    the same table by brute force for `--pairs` sampled site pairs: their q^2 double mutants each, built on the
                     host and pushed through dca_ar_log_probabilities (wall, build included), in the same run
  brute_all_s        that time scaled to all L (L - 1) / 2 pairs; speedup = brute_all_s / scores_ms
  max_abs_diff       largest |eps - brute force| over the sampled pairs (the table is checked where it is timed)

    python tools/epistasis_timing.py [--L 500] [--q 21] [--pairs 200] [--scale 0.1] [--reps 3]
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


def pair_index(L, k, l):
    return L * (L - 1) // 2 - (L - k) * (L - k - 1) // 2 + (l - k - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--q", type=int, default=21)
    ap.add_argument("--pairs", type=int, default=200)
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L, q = a.L, a.q
    rng = np.random.default_rng(0)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(rng.integers(0, q, size=(8, L)).astype(np.uint8), q)
    ctx.set_weights(np.ones(8))
    ctx.ar_configure(1e-6, 1e-2)
    ctx.ar_set_x(rng.normal(0.0, a.scale, ctx.ar_num_params()))
    w = rng.integers(0, q, size=L).astype(np.uint8)

    ctx.ar_epistatic_scores(w)                                    # warm-up: code objects, the pool's blocks
    ctx.set_profiling(True)
    ctx.reset_kernel_times()
    walls = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ctx.ar_epistatic_scores(w)
        walls.append((time.perf_counter() - t0) * 1e3)
    kernel_ms, launches = ctx.kernel_time("ar_epistasis")
    kernel_ms /= max(launches, 1)
    ctx.set_profiling(False)
    fma = float(q) ** 3 * sum(l * (L - 1 - l) for l in range(L))

    npairs = L * (L - 1) // 2
    sample = set()
    while len(sample) < min(a.pairs, npairs):
        k, l = sorted(int(v) for v in rng.choice(L, size=2, replace=False))
        sample.add((k, l))
    sample = sorted(sample)
    ctx.ar_log_probabilities(np.repeat(w[None, :], 1024, axis=0))   # warm-up of the brute-force path
    t0 = time.perf_counter()
    idx = np.arange(q * q)
    rows = np.repeat(w[None, :], len(sample) * q * q, axis=0)
    for n, (k, l) in enumerate(sample):
        rows[n * q * q + idx, k] = idx // q
        rows[n * q * q + idx, l] = idx % q
    lp = ctx.ar_log_probabilities(rows).reshape(len(sample), q, q)
    brute_ms = (time.perf_counter() - t0) * 1e3
    eps, _d = ctx.ar_epistasis(w, single=False)
    wk = np.array([w[k] for k, _l in sample])
    wl = np.array([w[l] for _k, l in sample])
    n = np.arange(len(sample))
    ref = lp - lp[n, :, wl][:, :, None] - lp[n, wk, :][:, None, :] + lp[n, wk, wl][:, None, None]
    got = np.stack([eps[pair_index(L, k, l)] for k, l in sample])
    scores_ms = float(np.median(walls))
    brute_all_s = brute_ms * 1e-3 * npairs / len(sample)
    print(json.dumps({
        "what": "arDCA epistatic scores vs brute force", "L": L, "q": q, "scale": a.scale, "reps": a.reps,
        "scores_ms": round(scores_ms, 3), "kernel_ms": round(kernel_ms, 3), "fma": fma,
        "tfma_per_s": round(fma / (kernel_ms * 1e-3) / 1e12, 3) if kernel_ms > 0 else None,
        "brute_pairs": len(sample), "brute_sample_ms": round(brute_ms, 3), "brute_all_s": round(brute_all_s, 3),
        "speedup": round(brute_all_s / (scores_ms * 1e-3), 1), "max_abs_diff": float(np.abs(got - ref).max()),
        "max_abs_log_p": float(np.abs(lp).max())}))


if __name__ == "__main__":
    main()
