#!/usr/bin/env python3
"""Time of the profile aligner at config D's shape; prints ONE JSON line.

Alignment of tools/gen_msa.py (L = 500, N = 50 000, q = 21; state 20 is the gap).  Reported (device time from HIP events, median
over the repetitions; the wall time of the call beside it):
  device_search   dca_sw_scores_device: the first row with its gaps filled (500 residues) against the 50 000 gap-stripped rows,
                  BLOSUM62 -10 / -1, local mode, scores only -- `align_dp` ms and DP cells per second
  host_search     the host loop dca_sw_scores of the SAME run on the first 500 of those rows (the same integers, checked), its
                  cells per second and the time for all rows EXTRAPOLATED from them by the number of cells
  traceback       dca_profile_align in glocal mode with traceback: the first 10 000 gap-stripped rows against the profile of the
                  alignment (build_profile's defaults, the weights of the context) -- `align_dp` + `align_trace` ms and the
                  bytes of edge columns and pointer bits of the largest pass; rows_reproduced counts the rows whose gap pattern
                  comes back exactly (the generator draws gaps independently per site: a curiosity, not a quality measure)

    python tools/alignment_timing.py [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pydca_amd import _lib, profile_alignment as PA  # noqa: E402
from pydca_amd.sequence_backmapper import scoring_matrix as sm  # noqa: E402
from tools.gen_msa import generate  # noqa: E402

LETTERS = "ACDEFGHIKLMNPQRSTVWY"


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    L, N, q, host_rows, trace_rows = 500, 50000, 21, 500, 10000
    X = generate(L, N, q, 2024)
    table = np.frombuffer(LETTERS.encode(), dtype=np.uint8)
    rows = [table[r[r < q - 1]].tobytes().decode() for r in X]
    first = X[0].copy()
    first[first == q - 1] = 0
    ref = table[first].tobytes().decode()
    sub, (go, ge) = sm.MATRICES["PROTEIN"], sm.GAP_PENALTIES["PROTEIN"]
    lens = np.array([len(s) for s in rows], dtype=np.int64)

    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_profiling(True)
    scores, ms, wall = timed(ctx, lambda: ctx.sw_scores(ref, rows, sub, go, ge), ("align_dp",), a.reps)
    cells = int(len(ref) * lens.sum())
    out = dict(L=L, N=N, q=q, reference_residues=len(ref), mean_row_residues=round(float(lens.mean()), 1),
               device_search=dict(align_dp_ms=round(ms["align_dp"], 3), call_ms=round(wall, 3), cells=cells,
                                  cells_per_s=float("%.4g" % (cells / ms["align_dp"] * 1e3))))
    t0 = time.perf_counter()
    host = _lib.sw_scores(ref, rows[:host_rows], sub, go, ge)
    host_ms = (time.perf_counter() - t0) * 1e3
    host_cells = int(len(ref) * lens[:host_rows].sum())
    out["host_search"] = dict(rows=host_rows, ms=round(host_ms, 3), cells=host_cells, cells_per_s=float("%.4g" % (host_cells / host_ms * 1e3)),
                              extrapolated_ms_all_rows=round(host_ms * cells / host_cells, 1), same_scores=bool(np.array_equal(host, scores[:host_rows])))
    out["device_search"]["speedup_over_extrapolated_host"] = round(out["host_search"]["extrapolated_ms_all_rows"] / ms["align_dp"], 1)

    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    P = PA.build_profile(X, w, q)
    codes = PA.letter_codes(_lib.PROTEIN, q)
    seqs = [codes[np.frombuffer(s.encode(), dtype=np.uint8)] for s in rows[:trace_rows]]
    call = lambda: ctx.profile_align(P["match"], P["del_open"], P["del_extend"], P["ins_open"], P["ins_extend"], _lib.DCA_ALIGN_GLOCAL, seqs)
    (_score, res), ms, wall = timed(ctx, call, ("align_dp", "align_trace"), a.reps)
    tcells = int(L * lens[:trace_rows].sum())
    out["traceback"] = dict(queries=trace_rows, mode="glocal", align_dp_ms=round(ms["align_dp"], 3), align_trace_ms=round(ms["align_trace"], 3),
                            call_ms=round(wall, 3), cells=tcells, cells_per_s=float("%.4g" % (tcells / (ms["align_dp"] + ms["align_trace"]) * 1e3)),
                            scratch_bytes=ctx.profile_align_last_scratch(),
                            rows_reproduced=int(sum(bool(np.array_equal(np.nonzero(r >= 0)[0], np.nonzero(x < q - 1)[0]))
                                                    for r, x in zip(res, X[:trace_rows]))))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
