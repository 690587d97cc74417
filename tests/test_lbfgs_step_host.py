"""CPU pin of tests/lbfgs_step_reference.py, the host reference of tests/test_lbfgs_step.py: the audit passes on a float64
trajectory of the committed oracle, its two-loop recursion equals dense BFGS, and three planted errors make it fail at the
planted iteration.  Also asserts that the oracle needs at least the audited number of iterations at every shape of the GPU
test, so none of its runs can stop early for lack of work.  Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import lbfgs_step_reference as R
from conftest import golden

LD = np.longdouble
K = 20            # toy_rna converges at its 20th iteration


@pytest.fixture(scope="module")
def oracle_run(oracle_plm):
    """x_0 .. x_K, g_0 .. g_K, steps and norms of a float64 oracle run on toy_rna; carry=False makes g a pure function of x."""
    G = golden("plm_toy_rna")
    X, q = np.ascontiguousarray(G["X"]), int(G["q"])
    lh, lJ = float(G["lambda_h"]), float(G["lambda_J"])
    w = oracle_plm.weights(X, 0.8, np.float64)
    x0 = oracle_plm.init_x(X, w, q)
    run = oracle_plm.lbfgs(X, w, q, lh, lJ, K, x0, carry=False, trace_cap=K, snapshots=range(0, K + 1))
    assert run["iterations"] == K, run["iterations"]
    xs = [x0] + [run["snapshots"][k] for k in range(1, K + 1)]
    gs = [oracle_plm.gradient(X, w, q, lh, lJ, x, carry=False)[1] for x in xs]
    tr = run["trace"]
    for v in xs + gs:
        v.setflags(write=False)
    return dict(xs=xs, gs=gs, steps=[float(t) for t in tr[:, 3]], xnorms=[None] + [float(v) for v in tr[:, 1]],
                gnorms=[None] + [float(v) for v in tr[:, 2]])


def test_audit_passes_on_the_oracle_trajectory(oracle_run):
    """Every element of every step of the oracle's own float64 run lies within the bound, and its norms within P 2^-53."""
    a = R.audit(oracle_run["xs"], oracle_run["gs"], oracle_run["steps"], np.float64, oracle_run["xnorms"], oracle_run["gnorms"])
    print("\n[lbfgs-step] oracle toy_rna: " + a.summary())
    for s in a.steps:
        print("[lbfgs-step]   %r (plain recursion off by %.3e)" % (s, s.rel_plain))
    assert a.ok, a.failures()
    assert max(a.ratios) <= 1.0
    assert [s.bound_pairs for s in a.steps] == [0, 1, 2, 3, 4] + [5] * (K - 5)


def test_two_loop_equals_dense_bfgs():
    """On a 12-variable convex quadratic the two-loop direction from five stored pairs is -H g with H from five explicit
    BFGS updates of (y.s / y.y) I, in longdouble."""
    rng = np.random.default_rng(5)
    n = 12
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = ((Q * np.linspace(1.0, 2.0, n)) @ Q.T).astype(LD)
    A = (A + A.T) / 2
    S = [rng.standard_normal(n) for _ in range(5)]
    Sl = [s.astype(LD) for s in S]
    Yl = [A @ s for s in Sl]
    g = rng.standard_normal(n)

    def exact_dot(a, b):
        return np.sum(a.astype(LD) * b.astype(LD))
    H = (exact_dot(Yl[-1], Sl[-1]) / exact_dot(Yl[-1], Yl[-1])) * np.eye(n, dtype=LD)
    I = np.eye(n, dtype=LD)
    for s, y in zip(Sl, Yl):
        r = 1 / exact_dot(y, s)
        V = I - r * np.outer(y, s)
        H = V.T @ H @ V + r * np.outer(s, s)
    want = -(H @ g.astype(LD))
    got = R.two_loop(g, Sl, Yl, dot=exact_dot)
    rel = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print("\n[lbfgs-step] two-loop against dense BFGS: %.3e relative (bound 1e-15)" % rel)
    assert rel <= 1e-15
    # the fsum dot product of the audit gives the same direction (its products of float64 inputs are rounded to longdouble)
    Yd = [y.astype(np.float64) for y in Yl]
    got64 = R.two_loop(g, S, Yd)
    want64 = R.two_loop(g, S, Yd, dot=exact_dot)
    rel64 = float(np.max(np.abs(got64 - want64)) / np.max(np.abs(want64)))
    print("[lbfgs-step] fsum dot products against longdouble sums: %.3e relative" % rel64)
    assert rel64 <= 1e-15


def _truncated(run, k, x_next):
    """The run up to the step from x_k, with x_{k+1} replaced."""
    xs = list(run["xs"][:k + 1]) + [x_next]
    return xs, run["gs"][:k + 2], run["steps"][:k + 1]


def test_control_two_oldest_pairs_swapped(oracle_run):
    k = 7                                     # five stored pairs
    d = R.reference_direction(oracle_run["xs"], oracle_run["gs"], k, order=[1, 0, 2, 3, 4])
    bad = R.apply_step(oracle_run["xs"][k], oracle_run["steps"][k], d, np.float64)
    a = R.audit(*_truncated(oracle_run, k, bad), np.float64)
    print("\n[lbfgs-step] control, pairs swapped: %r" % a.steps[k])
    assert not a.ok and a.first_failing_step() == k
    # the same construction with the pairs in order passes: the failure is the swap, not the construction
    good = R.apply_step(oracle_run["xs"][k], oracle_run["steps"][k], R.reference_direction(oracle_run["xs"], oracle_run["gs"], k), np.float64)
    assert R.audit(*_truncated(oracle_run, k, good), np.float64).ok


def test_control_tail_element_moved_by_two_ulp(oracle_run):
    """Late in the run, where the step is short: in float64 the rho term is rho |t| max|d|, so early on, with steps of the
    size of x itself, two ulp of a small element lie inside the bound by its construction."""
    k = 18
    P = len(oracle_run["xs"][0])
    start = 1 - P % 2                         # a walk that ends in a tail element in float64: odd length behind the head
    i = P - 1
    assert R.region(i, P, np.float64, (0, start) if start else (0,)).endswith("tail")
    bad = oracle_run["xs"][k + 1].copy()
    bad[i] = bad[i] + 2 * np.spacing(bad[i])
    a = R.audit(*_truncated(oracle_run, k, bad), np.float64, starts=(0, start) if start else (0,))
    print("\n[lbfgs-step] control, tail element + 2 ulp: %r" % a.steps[k])
    assert not a.ok and a.first_failing_step() == k
    assert a.steps[k].index == i and a.steps[k].where.endswith("tail")


def test_control_direction_rounded_to_float32(oracle_run):
    k = 3
    d = R.reference_direction(oracle_run["xs"], oracle_run["gs"], k).astype(np.float32)
    bad = R.apply_step(oracle_run["xs"][k], oracle_run["steps"][k], d, np.float64)
    a = R.audit(*_truncated(oracle_run, k, bad), np.float64)
    print("\n[lbfgs-step] control, d rounded to float32: %r" % a.steps[k])
    assert not a.ok and a.first_failing_step() == k


def test_region_names_the_loops_of_the_walk():
    assert R.region(0, 35, np.float32) == "packs, trip 1" and R.region(31, 35, np.float32) == "packs, trip 1"
    assert [R.region(i, 35, np.float32) for i in (32, 34)] == ["tail", "tail"]
    assert R.region(404, 405, np.float64) == "tail" and R.region(403, 405, np.float64) == "packs, trip 1"
    per_trip = R.VEC_BLOCKS * R.VEC_THREADS
    assert R.region(4 * per_trip - 1, 1128708, np.float32) == "packs, trip 1" and R.region(4 * per_trip, 1128708, np.float32) == "packs, trip 2"
    assert R.region(2 * per_trip, 1160481, np.float64) == "packs, trip 2" and R.region(1160480, 1160481, np.float64) == "tail"
    # column strips on L = 71, q = 5: rank 1 of 2 starts at 355 + 25 * 1855, two elements short of a 16-byte boundary in float32
    starts = R.strip_starts(71, 5, 2)
    assert starts == [0, 46730]
    assert [R.region(46730 + i, R.num_params(71, 5), np.float32, starts) for i in range(3)] == ["rank 1 head", "rank 1 head", "rank 1 packs, trip 1"]
    assert R.region(46729, R.num_params(71, 5), np.float32, starts) == "rank 0 tail"


@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_cases_plant_their_edges_and_keep_the_oracle_busy(oracle_plm, case):
    """Each shape has the residue and size it is there for, and the float64 oracle takes more than the audited number of
    iterations at the case's regularisation -- checked here so that an early stop on the GPU is a finding, not the data."""
    assert case.P == R.num_params(case.L, case.q) and case.P % 4 == R.P_MOD4[case.name]
    per_trip = R.VEC_BLOCKS * R.VEC_THREADS
    assert (case.P > per_trip * 4) == (case.name in R.SECOND_TRIP)            # float32 packs of 4, float64 packs of 2: both wrap
    X = R.alignment(case)
    assert len(np.unique(X, axis=0)) == len(X) and X.max() < case.q
    w = oracle_plm.weights(X, 0.8, np.float64)
    x0 = oracle_plm.init_x(X, w, case.q)
    run = oracle_plm.lbfgs(X, w, case.q, case.lam, case.lam, R.K_STEPS + 2, x0, carry=True)
    print("\n[lbfgs-step] %r N'=%d P=%d: oracle status %d after %d iterations" % (case, len(X), case.P, run["status"], run["iterations"]))
    assert run["iterations"] >= R.K_STEPS + 2, run
