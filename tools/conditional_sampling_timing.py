#!/usr/bin/env python3
"""Time of conditional Gibbs sampling beside the plain sampler at config D's size; prints ONE JSON line.

A float32 plm model with L = 500, q = 21 (random x, as tools/sampling_timing.py), 10 000 chains with a random background each,
F = 25, 100 and 500 free sites (a contiguous stretch from site 200; F = 500: every site).  Per F: the device time of the field pass
("cond_fields", once per call) and of one conditional sweep ("sample_cond"), and from the same run the plain sweep ("sample"):
HIP events around each launch, three repetitions, the median and the spread (max - min) of the per-repetition means.

    python tools/conditional_sampling_timing.py [--chains 10000] [--sweeps 10] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402


def stats(v):
    return dict(median_ms=round(float(np.median(v)), 4), spread_ms=round(float(np.max(v) - np.min(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10000)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L, q = 500, 21
    rng = np.random.default_rng(2024)

    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.set_profiling(True)
    X0 = rng.integers(0, q, size=(a.chains, L), dtype=np.uint8)
    lists = {F: np.arange(L) if F == L else np.arange(200, 200 + F) for F in (25, 100, 500)}

    ctx.plm_sample(a.chains, 1)                                    # warm-up (first launches, device allocations)
    for free in lists.values():
        ctx.plm_sample_conditional(X0, free, 1)
    plain, fields, sweep = [], {F: [] for F in lists}, {F: [] for F in lists}
    for r in range(a.reps):
        ctx.reset_kernel_times()
        ctx.plm_sample(a.chains, a.sweeps, seed=r)
        ms, launches = ctx.kernel_time("sample")
        assert launches == a.sweeps
        plain.append(ms / a.sweeps)
        for F, free in lists.items():
            ctx.reset_kernel_times()
            ctx.plm_sample_conditional(X0, free, a.sweeps, seed=r)
            fms, fl = ctx.kernel_time("cond_fields")
            sms, sl = ctx.kernel_time("sample_cond")
            assert fl == 1 and sl == a.sweeps and ctx.kernel_time("sample")[1] == 0
            fields[F].append(fms)
            sweep[F].append(sms / a.sweeps)
    ctx.close()

    p = stats(plain)
    out = dict(L=L, q=q, chains=a.chains, sweeps=a.sweeps, reps=a.reps, plain_sweep=p)
    for F in lists:
        s = stats(sweep[F])
        out["F%d" % F] = dict(cond_fields=stats(fields[F]), sample_cond_sweep=s,
                              sweep_over_plain=round(s["median_ms"] / p["median_ms"], 4), traffic_model=round((F / L) ** 2, 4))
    out["gate_F25_below_plain"] = bool(out["F25"]["sample_cond_sweep"]["median_ms"] < p["median_ms"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
