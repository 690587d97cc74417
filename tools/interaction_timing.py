#!/usr/bin/env python3
"""Time of the inter-protein energies beside the brute force through dca_plm_energies; prints ONE JSON line.

L = 500 split 250 / 250, q = 21; a float32 plm model (random x, as tools/sampling_timing.py) and a mean-field model (fitted on
2 000 random rows).  Two workloads: 10 000 x 10 000 all against all (G = 1), and 2 000 species of 5 x 5.  Per model and workload
the device time of the field pass ("cross_fields") and of the pair pass ("cross_energy"): HIP events around each launch, three
repetitions, the median and the spread (max - min).  In the same run the brute force: the four-energy identity needs
dca_plm_energies of four concatenated rows per pair; a sample of pairs is timed ("energies") and extrapolated to the workload.

    python tools/interaction_timing.py [--rows 10000] [--species 2000] [--sample 4096] [--reps 3]
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
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--species", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L, LA, q = 500, 250, 21
    rng = np.random.default_rng(2024)

    plm = _lib.Context(0, _lib.DCA_F32)
    plm.set_msa(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
    plm.compute_weights(0.8, _lib.DCA_F32)
    plm.plm_configure(1.0, 1.0)
    plm.plm_set_x(rng.normal(0, 0.05, plm.num_params()).astype(np.float32))
    mf = _lib.Context(0, _lib.DCA_F64)
    mf.set_msa(rng.integers(0, q, size=(2000, L), dtype=np.uint8), q)
    mf.compute_weights(0.8, _lib.DCA_F64)
    mf.mf_run(0.5, True)

    XA = rng.integers(0, q, size=(a.rows, LA), dtype=np.uint8)
    XB = rng.integers(0, q, size=(a.rows, L - LA), dtype=np.uint8)
    off = (np.arange(a.species + 1) * 5).astype(np.int32)
    work = dict(all_against_all=dict(XA=XA, XB=XB, oa=None, ob=None, pairs=a.rows * a.rows),
                species_5x5=dict(XA=XA[:5 * a.species], XB=XB[:5 * a.species], oa=off, ob=off, pairs=25 * a.species))
    out = dict(L=L, split=LA, q=q, rows=a.rows, species=a.species, reps=a.reps)
    for name, ctx, call in (("plm_f32", plm, plm.plm_interaction_energies), ("mf", mf, mf.mf_interaction_energies)):
        ctx.set_profiling(True)
        out[name] = {}
        for wname, w in work.items():
            call(w["XA"][:512], w["XB"][:512], LA)                    # warm-up (first launches, device allocations)
            fields, pairs = [], []
            for _ in range(a.reps):
                ctx.reset_kernel_times()
                call(w["XA"], w["XB"], LA, w["oa"], w["ob"])
                fms, fl = ctx.kernel_time("cross_fields")
                pms, pl = ctx.kernel_time("cross_energy")
                assert fl >= 1 and pl == fl
                fields.append(fms)
                pairs.append(pms)
            out[name][wname] = dict(pairs=w["pairs"], cross_fields=stats(fields), cross_energy=stats(pairs),
                                    total_ms=round(float(np.median(fields) + np.median(pairs)), 4))
    # the brute force of the same run: four full energies per pair, on a sample of pairs
    n = a.sample
    ia, ib = rng.integers(0, a.rows, n), rng.integers(0, a.rows, n)
    ja, jb = (ia + 1) % a.rows, (ib + 1) % a.rows
    cat = [np.concatenate([XA[x], XB[y]], axis=1) for x, y in ((ia, ib), (ia, jb), (ja, ib), (ja, jb))]
    plm.plm_energies(cat[0][:256])
    brute = []
    for _ in range(a.reps):
        plm.reset_kernel_times()
        for c in cat:
            plm.plm_energies(c)
        brute.append(plm.kernel_time("energies")[0])
    per_pair = float(np.median(brute)) / n
    out["brute_force_plm_f32"] = dict(sample_pairs=n, four_calls=stats(brute), ms_per_pair=per_pair)
    for wname, w in work.items():
        est = per_pair * w["pairs"]
        out["brute_force_plm_f32"][wname + "_extrapolated_ms"] = round(est, 2)
        out["plm_f32"][wname]["speedup_over_brute_force"] = round(est / out["plm_f32"][wname]["total_ms"], 1)
    out["gate_faster_than_brute_force"] = bool(all(out["plm_f32"][w]["speedup_over_brute_force"] > 1.0 for w in work))
    plm.close()
    mf.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
