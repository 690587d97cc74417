#!/usr/bin/env python3
"""Time of the three-site scan (dca_three_site_scan) and of the values entry; prints ONE JSON line.

Legs: config D's shape -- the alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21, de-duplicated) under its weights and a
set of 10 000 sequences (alignment rows with 15 % of their sites redrawn) -- and a smaller alignment, L = 100, N = 10 000.  Every
scan is ONE call (K = 10 000): its passes over all C(L,3) q^3 elements (histogram, a refinement if the edge bin is crowded,
append) are the launches of the tag "three_site_scan", so ms per pass = device ms / launches.  Reported per leg: the passes, ms
per pass, the wall time of the call (host lists, tables and the final sort included), elements per second and weighted
increments per second (n C(L,3) LDS additions per pass).  The yardstick from the same run: the pair counts of the mean-field
model ("mf_counts", through dca_alignment_statistics) at N L (L - 1) / 2 nominal increments.  values: the set's c_ijk at the
alignment's K strongest elements.

    python tools/three_site_timing.py [--top 10000] [--small_only]
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


def scan_leg(ctx, K, Q, n, L, q):
    ctx.reset_kernel_times()
    t0 = time.perf_counter()
    el, _c3, _f3 = ctx.three_site_scan(K, Q)
    wall = (time.perf_counter() - t0) * 1e3
    ms, passes = ctx.kernel_time("three_site_scan")
    triples = L * (L - 1) * (L - 2) // 6
    per = ms / max(passes, 1)
    return el, dict(n=n, L=L, passes=passes, ms_per_pass=round(per, 3), call_ms=round(wall, 3),
                    elements_per_s=float("%.4g" % (triples * q ** 3 / per * 1e3)),
                    increments_per_s=float("%.4g" % (n * triples / per * 1e3)))


def counts_leg(ctx, N, L):
    ctx.alignment_statistics()                  # warm-up: allocations
    ctx.reset_kernel_times()
    ctx.alignment_statistics()
    ms, _n = ctx.kernel_time("mf_counts")
    return dict(ms=round(ms, 3), increments_per_s=float("%.4g" % (N * L * (L - 1) / 2 / ms * 1e3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--top", type=int, default=10000)
    ap.add_argument("--small_only", action="store_true", help="only the L = 100, N = 10 000 leg")
    a = ap.parse_args()
    q = 21
    out = dict(q=q, top=a.top)
    for name, L, N0 in (("small", 100, 10000),) + (() if a.small_only else (("D", 500, 50000),)):
        X = dedup(generate(L, N0, q, 2024))
        N = int(X.shape[0])
        ctx = _lib.Context(0, _lib.DCA_F64)
        ctx.set_msa(X, q)
        ctx.compute_weights(0.8, _lib.DCA_F64)
        ctx.set_profiling(True)
        leg = dict(mf_counts=counts_leg(ctx, N, L))
        el, leg["alignment_scan"] = scan_leg(ctx, a.top, None, N, L, q)
        if name == "D":
            rng = np.random.default_rng(7)
            Q = X[rng.integers(0, N, size=10000)].copy()
            flip = rng.random(Q.shape) < 0.15
            Q[flip] = rng.integers(0, q, size=int(flip.sum()), dtype=np.uint8)
            _el, leg["set_scan"] = scan_leg(ctx, a.top, Q, 10000, L, q)
            ctx.reset_kernel_times()
            t0 = time.perf_counter()
            ctx.three_site_values(el, Q)
            leg["values"] = dict(T=int(el.shape[0]), n=10000, ms=round(ctx.kernel_time("three_site_values")[0], 3),
                                 call_ms=round((time.perf_counter() - t0) * 1e3, 3))
        for k in ("alignment_scan", "set_scan"):
            if k in leg:
                leg[k]["rate_vs_mf_counts"] = round(leg[k]["increments_per_s"] / leg["mf_counts"]["increments_per_s"], 3)
        out[name] = leg
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
