"""The CPU oracle's view of the cases of tests/test_fused_step_pass.py: every shape runs its six iterations, and the line-search
case rejects a first trial at step 1 in an iteration after the first (more evaluations than iterations + 1), so the device run
has to fall back to the three kernels there."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gen_msa  # noqa: E402

from oracle import plm as oplm  # noqa: E402

import test_fused_step_pass as F  # noqa: E402


def oracle_run(shape):
    q, L, N, seed, lh, lJ = shape
    X = gen_msa.generate(L, N, q, seed)
    w = oplm.weights(X, 0.8, np.float32)
    return oplm.lbfgs(X, w, q, lh, lJ, F.ITERS, oplm.init_x(X, w, q), trace_cap=F.ITERS)


def test_every_shape_runs_six_iterations():
    for name, shape in F.SHAPES.items():
        r = oracle_run(shape)
        assert r["iterations"] == F.ITERS, (name, r["status"], r["iterations"])


def test_line_search_case_needs_a_second_trial_after_the_first_iteration():
    r = oracle_run(F.MULTI_EVAL[1])
    assert r["iterations"] == F.ITERS and r["evaluations"] > r["iterations"] + 1, (r["iterations"], r["evaluations"])
    assert any(float(t) != 1.0 for t in r["trace"][1:, 3]), r["trace"][:, 3]
