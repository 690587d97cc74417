#!/usr/bin/env python3
"""Time of the greedy ascent beside the brute force at config D's size; prints ONE JSON line.

A float32 plm model with L = 500, q = 21 (random x, as tools/sampling_timing.py), 10 000 chains:
  (a) random_starts    the tag-1 random starts (plm_sample with 0 sweeps), every site free
  (b) after_10_sweeps  the same chains after 10 Gibbs sweeps, every site free
  (c) F25              (b) again with 25 free sites (200 .. 224)
Per case, three repetitions: the device time of the table pass ("ascent_init") and of the ascent ("ascent"; HIP events around
each launch), the total number of steps, the device microseconds per chain-step ((ascent_init + ascent) / steps and ascent / steps)
and the wall-clock microseconds per chain-step of the whole call; the median and the spread (max - min) over the repetitions.
In the same run the brute force: a host loop of plm_mutation_scan + arg-max over the first 5 steps of 20 chains of (a), wall clock
per chain-step; its moves must be the ascent's.  gate: the brute force costs at least 10 x the whole call of (a) per chain-step.

    python tools/ascent_timing.py [--chains 10000] [--reps 3]
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


def stats(v, digits=4):
    return dict(median=round(float(np.median(v)), digits), spread=round(float(np.max(v) - np.min(v)), digits))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--brute_chains", type=int, default=20)
    ap.add_argument("--brute_steps", type=int, default=5)
    a = ap.parse_args()
    L, q = 500, 21
    rng = np.random.default_rng(2024)

    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(rng.normal(0, 0.05, ctx.num_params()).astype(np.float32))
    ctx.set_profiling(True)
    every = np.arange(L)
    start = ctx.plm_sample(a.chains, 0, seed=1)
    swept = ctx.plm_sample(a.chains, 10, seed=1)
    cases = (("random_starts", start, every), ("after_10_sweeps", swept, every), ("F25", swept, np.arange(200, 225)))

    ctx.plm_ascend(start[:512], every)                              # warm-up (first launches, device allocations)
    out = dict(L=L, q=q, chains=a.chains, reps=a.reps)
    first = ctx.plm_ascend(start[:a.brute_chains], every, paths=True)      # the moves the brute force must repeat
    for name, X, free in cases:
        init, asc, wall, steps = [], [], [], 0
        for _ in range(a.reps):
            ctx.reset_kernel_times()
            t0 = time.perf_counter()
            res = ctx.plm_ascend(X, free)
            wall.append((time.perf_counter() - t0) * 1e3)
            ims, il = ctx.kernel_time("ascent_init")
            ams, al = ctx.kernel_time("ascent")
            assert il == 1 and al == 1
            init.append(ims)
            asc.append(ams)
            steps = int(res["steps"].sum())
        per = max(steps, 1)
        out[name] = dict(free_sites=int(free.size), total_steps=steps, converged=int(res["converged"].sum()),
                         ascent_init_ms=stats(init), ascent_ms=stats(asc), call_wall_ms=stats(wall),
                         device_us_per_chain_step=stats([(i + s) * 1e3 / per for i, s in zip(init, asc)], 5),
                         ascent_us_per_chain_step=stats([s * 1e3 / per for s in asc], 5),
                         call_wall_us_per_chain_step=stats([w * 1e3 / per for w in wall], 5))

    # the brute force: one mutation scan and an arg-max on the host per chain and step
    brute, same, done = [], True, 0
    for _ in range(a.reps):
        t0 = time.perf_counter()
        done = 0
        for k in range(min(a.brute_chains, a.chains)):
            s = start[k].copy()
            for t in range(min(a.brute_steps, int(first["steps"][k]))):
                dE = ctx.plm_mutation_scan(s)
                dE[np.arange(L), s] = -np.inf
                i, b = np.unravel_index(int(np.argmax(dE)), dE.shape)
                same = same and (int(i), int(b)) == tuple(int(v) for v in first["path"][k, t])
                s[i] = b
                done += 1
        brute.append((time.perf_counter() - t0) * 1e6 / max(done, 1))
    ctx.close()
    out["brute_force"] = dict(chains=min(a.brute_chains, a.chains), steps_each=a.brute_steps, chain_steps=done,
                              us_per_chain_step=stats(brute, 2), same_moves_as_the_ascent=bool(same))
    ratio = out["brute_force"]["us_per_chain_step"]["median"] / max(out["random_starts"]["call_wall_us_per_chain_step"]["median"], 1e-9)
    out["brute_force_over_ascent"] = round(ratio, 1)
    out["gate_10x_cheaper_than_brute_force"] = bool(ratio >= 10.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
