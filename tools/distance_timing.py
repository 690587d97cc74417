#!/usr/bin/env python3
"""Time of the sequence-set comparison at config D's size; prints ONE JSON line.

Alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21, de-duplicated), 10 000 queries (alignment rows with 15 % of their
sites redrawn).  Reported (device time of the stage from HIP events, median over the repetitions; the wall time of the call
beside it):
  hamming           dca_hamming_nearest, queries against the alignment, with and without the histogram
  self              the alignment against itself (N x N, both halves, diagonal skipped), with the histogram
  statistics        dca_sequence_statistics split into the counts ("bm_stats") and the comparison ("set_compare")
  weights           dca_compute_weights of the same alignment with its work counter (DCA_WEIGHTS_WORK=1): the yardstick -- both
                    kernels run the same inner loop, so their rates per compared (wave, 32-site group) are comparable
and, per distance leg, pair-site compares per second, wave x group units per second and the fraction of the integer-issue roof
bench.py prices the weight kernel with (16 pairs per lane x (planes + 3) VALU instructions per unit; 256 CUs x 4 SIMDs x 2.4 GHz
/ 4 cycles per wave instruction).

    python tools/distance_timing.py [--queries 10000] [--reps 5]
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

PEAK = 256 * 4 * 2.4e9 / 4.0              # wave instructions per second


def timed(ctx, call, tags, reps):
    call()                                  # warm-up (first launch, device allocations)
    dev, wall = {t: [] for t in tags}, []
    for _ in range(reps):
        ctx.reset_kernel_times()
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for t in tags:
            dev[t].append(ctx.kernel_time(t)[0])
    return {t: float(np.median(v)) for t, v in dev.items()}, float(np.median(wall))


def leg(ms, wall, nq, nr, L, planes):
    G = (L + 127) // 128 * 4                                     # 32-site groups of the padded rows
    units = ((nq + 63) // 64) * ((nr + 63) // 64) * 4 * G        # (wave, group) units: 1024 pairs x 32 sites each
    return dict(ms=round(ms, 3), call_ms=round(wall, 3), pair_site_compares_per_s=float("%.4g" % (nq * nr * L / ms * 1e3)),
                wave_groups_per_s=float("%.4g" % (units / ms * 1e3)),
                integer_roof_frac=round(units * 16.0 * (planes + 3.0) / (ms * 1e-3) / PEAK, 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    L, N0, q = 500, 50000, 21
    X = dedup(generate(L, N0, q, 2024))
    N = int(X.shape[0])
    rng = np.random.default_rng(7)
    Q = X[rng.integers(0, N, size=a.queries)].copy()
    flip = rng.random(Q.shape) < 0.15
    Q[flip] = rng.integers(0, q, size=int(flip.sum()), dtype=np.uint8)

    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.set_profiling(True)
    os.environ["DCA_WEIGHTS_WORK"] = "1"
    w_ms, _w_wall = timed(ctx, lambda: ctx.compute_weights(0.8, _lib.DCA_F64), ("weights",), a.reps)
    groups, groups_all, planes = ctx.weights_work()
    del os.environ["DCA_WEIGHTS_WORK"]
    w_ms = w_ms["weights"]
    out = dict(L=L, N=N, q=q, queries=a.queries, planes=planes,
               weights=dict(ms=round(w_ms, 3), wave_groups=groups, wave_groups_without_exit=groups_all,
                            wave_groups_per_s=float("%.4g" % (groups / w_ms * 1e3)),
                            integer_roof_frac=round(groups * 16.0 * (planes + 3.0) / (w_ms * 1e-3) / PEAK, 4)))
    for name, hist in (("hamming_hist", True), ("hamming", False)):
        ms, wall = timed(ctx, lambda: ctx.hamming_nearest(Q, return_histogram=hist), ("hamming",), a.reps)
        out[name] = leg(ms["hamming"], wall, a.queries, N, L, planes)
    ms, wall = timed(ctx, lambda: ctx.hamming_nearest(None, None, True), ("hamming",), max(1, a.reps // 2))
    out["self_hist"] = leg(ms["hamming"], wall, N, N, L, planes)
    for name in ("hamming_hist", "hamming", "self_hist"):
        out[name]["rate_vs_weights"] = round(out[name]["wave_groups_per_s"] / out["weights"]["wave_groups_per_s"], 3)
    ms, wall = timed(ctx, lambda: ctx.sequence_statistics(Q, frequencies=False), ("bm_stats", "set_compare"), max(1, a.reps // 2))
    out["statistics"] = dict(counts_ms=round(ms["bm_stats"], 3), compare_ms=round(ms["set_compare"], 3), call_ms=round(wall, 3))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
