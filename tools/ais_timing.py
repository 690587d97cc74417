#!/usr/bin/env python3
"""Time of annealed importance sampling (dca_plm_ais / dca_mf_ais) at config D's size; prints ONE JSON line.

plm: a float32 model with L = 500, q = 21 (random x, as tools/sampling_timing.py); mf: the mean-field couplings of a random
L = 500, q = 21 alignment.  Per leg: device ms per temperature, split into the "sample" stage (the s sweeps of one
intermediate temperature) and the "ais" stage (the start draw and the K weight updates, spread over the K temperatures);
HIP events around each launch group, median over the repetitions.

    python tools/ais_timing.py [--chains 1000] [--temperatures 20] [--sweeps 1] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402


def timed(ctx, fn, chains, K, s, reps):
    fn(chains, 2, sweeps_per_temperature=s)                   # warm-up (first launches, device allocations)
    sample, ais = [], []
    for r in range(reps):
        ctx.reset_kernel_times()
        fn(chains, K, sweeps_per_temperature=s, seed=r)
        ms_s, n_s = ctx.kernel_time("sample")
        ms_a, n_a = ctx.kernel_time("ais")
        assert n_s == (K - 1) * s and n_a == K + 1
        sample.append(ms_s / max(K - 1, 1))
        ais.append(ms_a / K)
    return dict(sample_ms_per_temperature=round(float(np.median(sample)), 4), ais_ms_per_temperature=round(float(np.median(ais)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--temperatures", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=1)
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
    plm = timed(ctx, ctx.plm_ais, a.chains, a.temperatures, a.sweeps, a.reps)
    ctx.close()

    mctx = _lib.Context(0, _lib.DCA_F64)
    mctx.set_msa(rng.integers(0, q, size=(2000, L), dtype=np.uint8), q)
    mctx.compute_weights(0.8, _lib.DCA_F64)
    mctx.mf_corr_mat(0.5, want=False)
    mctx.mf_couplings(want=False)
    mctx.set_profiling(True)
    mf = timed(mctx, mctx.mf_ais, a.chains, a.temperatures, a.sweeps, a.reps)
    mctx.close()

    print(json.dumps(dict(L=L, q=q, chains=a.chains, temperatures=a.temperatures, sweeps_per_temperature=a.sweeps, plm_f32=plm,
                          mf=mf)))


if __name__ == "__main__":
    main()
