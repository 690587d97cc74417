#!/usr/bin/env python3
"""Time of replica-exchange Gibbs sampling beside the plain sampler at config D's size; prints ONE JSON line.

A float32 plm model with L = 500, q = 21 (random x, as tools/sampling_timing.py), 10 000 walkers as 1 000 ladders of 10 levels
(a geometric ladder of temperatures from 0.5 to 2), an exchange round after every sweep.  Per repetition, one after the other: a
plain run of 10 000 chains and a tempered run, each of `sweeps` sweeps; the device time of one plain sweep and of one tempered
sweep (both under "sample": the same kernel, the tempered one with a beta per chain), of one energy pass ("pt_energy") and of one
exchange kernel ("pt_swap"): HIP events around each launch, the median and the spread (max - min) of the per-repetition means.

    python tools/tempered_sampling_timing.py [--ladders 1000] [--levels 10] [--sweeps 10] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib, _potts  # noqa: E402


def stats(v):
    return dict(median_ms=round(float(np.median(v)), 4), spread_ms=round(float(np.max(v) - np.min(v)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ladders", type=int, default=1000)
    ap.add_argument("--levels", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    L, q = 500, 21
    rng = np.random.default_rng(2024)
    n = a.ladders * a.levels
    betas = np.sort(1.0 / _potts.temperature_ladder(0.5, 2.0, a.levels))

    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.set_profiling(True)

    ctx.plm_sample(n, 1)                                           # warm-up (first launches, device allocations)
    ctx.plm_sample_tempered(a.ladders, betas, 1)
    plain, tempered, energy, swap, accepted = [], [], [], [], []
    for r in range(a.reps):
        ctx.reset_kernel_times()
        ctx.plm_sample(n, a.sweeps, seed=r)
        ms, launches = ctx.kernel_time("sample")
        assert launches == a.sweeps
        plain.append(ms / a.sweeps)
        ctx.reset_kernel_times()
        res = ctx.plm_sample_tempered(a.ladders, betas, a.sweeps, swap_interval=1, seed=r)
        ms, launches = ctx.kernel_time("sample")
        ems, el = ctx.kernel_time("pt_energy")
        sms, sl = ctx.kernel_time("pt_swap")
        assert launches == a.sweeps and sl == a.sweeps and el == a.sweeps + 1      # (one more pass for the final energies)
        tempered.append(ms / a.sweeps)
        energy.append(ems / el)
        swap.append(sms / sl)
        accepted.append(float(res["accepts"].sum()) / float(res["attempts"].sum()))
    ctx.close()

    p, t, e, s = stats(plain), stats(tempered), stats(energy), stats(swap)
    print(json.dumps(dict(L=L, q=q, ladders=a.ladders, levels=a.levels, walkers=n, swap_interval=1, sweeps=a.sweeps, reps=a.reps,
                          plain_sweep=p, tempered_sweep=t, pt_energy_per_round=e, pt_swap_per_round=s,
                          tempered_over_plain=round(t["median_ms"] / p["median_ms"], 4),
                          round_over_sweep=round((e["median_ms"] + s["median_ms"]) / t["median_ms"], 4),
                          accepted_fraction=round(float(np.median(accepted)), 4))))


if __name__ == "__main__":
    main()
