#!/usr/bin/env python3
"""Time of the Gibbs samplers at config D's size; prints ONE JSON line.

plm: dca_plm_sample on a float32 model with L = 500, q = 21 (random x, as tools/energy_timing.py);
mf: dca_mf_sample under the mean-field couplings of a random L = 500, q = 21 alignment.
Reported per leg: the device time of the "sample" stage per sweep (HIP events around each sweep's launch; median over the
repetitions), sweeps per second, and coupling lookups per second = chains * sweeps * L * (L - 1) * q / device time.

    python tools/sampling_timing.py [--chains 10000] [--sweeps 10] [--reps 3]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib  # noqa: E402


def timed(ctx, fn, chains, sweeps, reps):
    fn(chains, 1)                                   # warm-up (first launch, device allocations)
    dev = []
    for r in range(reps):
        ctx.reset_kernel_times()
        fn(chains, sweeps, seed=r)
        ms, launches = ctx.kernel_time("sample")
        assert launches == sweeps
        dev.append(ms / sweeps)
    return float(np.median(dev))


def leg(ms_per_sweep, chains, L, q):
    lookups = chains * L * (L - 1) * q
    return dict(sweep_ms=round(ms_per_sweep, 4), sweeps_per_s=round(1e3 / ms_per_sweep, 2),
                glookups_per_s=round(lookups / ms_per_sweep * 1e-6, 1))


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
    plm = timed(ctx, ctx.plm_sample, a.chains, a.sweeps, a.reps)
    ctx.close()

    mctx = _lib.Context(0, _lib.DCA_F64)
    mctx.set_msa(rng.integers(0, q, size=(2000, L), dtype=np.uint8), q)
    mctx.compute_weights(0.8, _lib.DCA_F64)
    mctx.mf_corr_mat(0.5, want=False)
    mctx.mf_couplings(want=False)
    mctx.set_profiling(True)
    mf = timed(mctx, mctx.mf_sample, a.chains, a.sweeps, a.reps)
    mctx.close()

    print(json.dumps(dict(L=L, q=q, chains=a.chains, sweeps=a.sweeps, lookups_per_sweep=a.chains * L * (L - 1) * q,
                          plm_f32=leg(plm, a.chains, L, q), mf=leg(mf, a.chains, L, q))))


if __name__ == "__main__":
    main()
