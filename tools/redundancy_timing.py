#!/usr/bin/env python3
"""Time of the redundancy filter and the identity clusters at config D's shape; prints ONE JSON line.

Alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21, de-duplicated), the one tools/distance_timing.py uses.  If it holds
no similar pair at the two thresholds (nothing removed at 0.9 and only singletons at 0.8) the rows are replaced by descendants
of 300 ancestors (1 to 20 % of the sites redrawn) and "alignment" says so.  Reported (device time from HIP events, median over
the repetitions; the wall time of the call beside it):
  identity_filter     dca_identity_filter at identity 0.9, file order, with the kept fraction and the block plan
  identity_clusters   dca_identity_clusters at identity 0.8, split into the bits pass, the component rounds and the degrees,
                      with the cluster count, the largest cluster and the rounds; the (wave, 32-site group) units per second
                      of the bits pass (every wave of every tile pair compares all groups)
  recomputed          the same with DCA_CLUSTER_BITS_MAX=0 (nothing stored, every round recomputes the compares)
and, from the SAME run, the yardsticks:
  weights             dca_compute_weights with its work counter (DCA_WEIGHTS_WORK=1)
  self_hist           the N x N self leg of dca_hamming_nearest with the histogram -- the same compares as the bits pass

    python tools/redundancy_timing.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib, redundancy  # noqa: E402
from tools.gen_msa import dedup, generate  # noqa: E402


def timed(ctx, call, tags, reps):
    res = call()                            # warm-up (first launch, device allocations)
    dev, wall = {t: [] for t in tags}, []
    for _ in range(reps):
        ctx.reset_kernel_times()
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        for t in tags:
            dev[t].append(ctx.kernel_time(t)[0])
    return res, {t: float(np.median(v)) for t, v in dev.items()}, float(np.median(wall))


def descendants(L, N, q, seed):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, q, size=(300, L), dtype=np.uint8)
    X = anc[rng.integers(0, 300, size=N)]
    rate = rng.uniform(0.01, 0.2, size=(N, 1))
    flip = rng.random((N, L)) < rate
    X[flip] = rng.integers(0, q, size=int(flip.sum()), dtype=np.uint8)
    return dedup(X)


def rate(units, ms):
    return float("%.4g" % (units / ms * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L, N0, q = 500, 50000, 21
    T9, T8 = redundancy.identity_threshold(L, 0.9), redundancy.identity_threshold(L, 0.8)
    X, source = dedup(generate(L, N0, q, 2024)), "tools/gen_msa.py, seed 2024"
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    keep, _rep, _info = ctx.identity_filter(T9, return_representatives=False)
    _lab, _deg, cinfo = ctx.identity_clusters(T8, return_degrees=False)
    if keep.all() and cinfo["largest"] == 1:
        X, source = descendants(L, N0, q, 2024), "descendants of 300 ancestors, 1-20 % of the sites redrawn, seed 2024"
        ctx.set_msa(X, q)
    N = int(X.shape[0])
    ctx.set_profiling(True)
    G = (L + 127) // 128 * 4
    units = ((N + 63) // 64) ** 2 * 4 * G            # (wave, group) units of one pass over all tile pairs, both halves

    (keep, _rep, finfo), ms, wall = timed(ctx, lambda: ctx.identity_filter(T9), ("identity_filter",), a.reps)
    out = dict(L=L, N=N, q=q, alignment=source,
               identity_filter=dict(identity=0.9, min_identical=T9, ms=round(ms["identity_filter"], 3), call_ms=round(wall, 3),
                                    kept=int(keep.sum()), kept_fraction=round(float(keep.sum()) / N, 4), blocks=finfo["blocks"],
                                    block_rows=finfo["block_rows"], tile_pairs=finfo["tile_pairs"]))
    tags = ("identity_clusters", "identity_clusters_bits", "identity_clusters_rounds", "identity_clusters_degrees")
    for name, cap in (("identity_clusters", None), ("recomputed", "0")):
        if cap is not None:
            os.environ["DCA_CLUSTER_BITS_MAX"] = cap
        (_lab, _deg, info), ms, wall = timed(ctx, lambda: ctx.identity_clusters(T8), tags, a.reps)
        os.environ.pop("DCA_CLUSTER_BITS_MAX", None)
        out[name] = dict(identity=0.8, min_identical=T8, ms=round(ms["identity_clusters"], 3), call_ms=round(wall, 3),
                         bits_ms=round(ms["identity_clusters_bits"], 3), rounds_ms=round(ms["identity_clusters_rounds"], 3),
                         degrees_ms=round(ms["identity_clusters_degrees"], 3), clusters=info["clusters"], largest=info["largest"],
                         rounds=info["rounds"], stored_bits=info["stored_bits"])
    out["identity_clusters"]["bits_wave_groups_per_s"] = rate(units, out["identity_clusters"]["bits_ms"])

    os.environ["DCA_WEIGHTS_WORK"] = "1"
    _w, ms, _wall = timed(ctx, lambda: ctx.compute_weights(0.8, _lib.DCA_F64), ("weights",), a.reps)
    groups, groups_all, planes = ctx.weights_work()
    del os.environ["DCA_WEIGHTS_WORK"]
    out["weights"] = dict(ms=round(ms["weights"], 3), wave_groups=int(groups), wave_groups_without_exit=int(groups_all),
                          wave_groups_per_s=rate(groups, ms["weights"]))
    _r, ms, wall = timed(ctx, lambda: ctx.hamming_nearest(None, None, True), ("hamming",), max(1, a.reps // 2))
    out["self_hist"] = dict(ms=round(ms["hamming"], 3), call_ms=round(wall, 3), wave_groups_per_s=rate(units, ms["hamming"]))
    out["identity_clusters"]["bits_rate_vs_self_hist"] = round(out["identity_clusters"]["bits_wave_groups_per_s"] /
                                                               out["self_hist"]["wave_groups_per_s"], 3)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
