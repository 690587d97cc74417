"""The optimisers' line search (pydca_amd/csrc/more_thuente.h, host code that plm_engine.hip and ardca.hip both run) against
the oracle's independent C restatement of the reference's (oracle/plm_oracle_impl.h: mt_search), on the CPU.  Both minimise
the same 1-D functions phi(t) through one ctypes callback (n = 1, x = xp + stp * s with xp = 0 and s = 1, so x IS the trial
step), with plmDCA's constants (max_linesearch = 5), and have to agree EXACTLY: the sequence of trial steps, the returned
evaluation count or libLBFGS code, the final step and value.

The functions are the six of More & Thuente (1994, section 5), from starting steps 1e-3 .. 1e3.  Together they take each of
the four cases of the trial-interval update and the first stage's modified function (seen in a traced build when this was
written: functions 2 and 3 take cases 1 to 4, cases 3 and 4 both with and without a bracket; 1, 4, 5 and 6 take case 1 on
the modified function); the extra cases end in the failure codes a caller can meet."""
import ctypes as C
import math
import os
import subprocess

import pytest

from conftest import ROOT

LB_MINIMUMSTEP, LB_MAXIMUMSTEP, LB_MAXIMUMLINESEARCH, LB_INVALIDPARAMETERS, LB_INCREASEGRADIENT = -1000, -999, -998, -995, -994

EVAL_FN = C.CFUNCTYPE(C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_size_t)
_DP = C.POINTER(C.c_double)
_ARGS = [C.c_size_t, _DP, _DP, _DP, _DP, _DP, _DP, EVAL_FN, C.c_void_p, C.POINTER(C.c_int)]


@pytest.fixture(scope="module")
def searches(oracle_plm, tmp_path_factory):
    """(oracle's search, the product's search): f(phi, stp0, deferred=False) -> (trial steps, result, final step, final value)"""
    so = str(tmp_path_factory.mktemp("mt") / "libmt_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fno-fast-math", "-ffp-contract=off", "-shared", "-fPIC", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "more_thuente_driver.cpp")])
    ours = C.CDLL(so).mt_search_driver
    ours.restype = C.c_int
    ours.argtypes = _ARGS + [C.c_int]
    theirs = oracle_plm.lib().oracle_mt_search_f64
    theirs.restype = C.c_int
    theirs.argtypes = _ARGS

    def run(fn, extra, phi, stp0):
        trials = []

        def cb(_ctx, x, g, _n):
            f, d = phi(x[0])
            trials.append(x[0])
            g[0] = d
            return f
        f0, d0 = phi(0.0)
        x, f, g, s, stp, xp, nev = (C.c_double(0.0), C.c_double(f0), C.c_double(d0), C.c_double(1.0), C.c_double(stp0),
                                    C.c_double(0.0), C.c_int(0))
        ret = fn(1, C.byref(x), C.byref(f), C.byref(g), C.byref(s), C.byref(stp), C.byref(xp), EVAL_FN(cb), None, C.byref(nev), *extra)
        assert nev.value == len(trials)
        return trials, ret, stp.value, f.value

    return (lambda phi, stp0: run(theirs, (), phi, stp0)), (lambda phi, stp0, deferred=False: run(ours, (int(deferred),), phi, stp0))


# ---- More & Thuente 1994, section 5: (phi, phi')
def mt1(a, b=2.0):
    return -a / (a * a + b), (a * a - b) / (a * a + b) ** 2


def mt2(a, b=0.004):
    return (a + b) ** 5 - 2 * (a + b) ** 4, 5 * (a + b) ** 4 - 8 * (a + b) ** 3


def mt3(a, b=0.01, l=39):
    if a <= 1 - b:
        f0, d0 = 1 - a, -1.0
    elif a >= 1 + b:
        f0, d0 = a - 1, 1.0
    else:
        f0, d0 = (a - 1) ** 2 / (2 * b) + b / 2, (a - 1) / b
    w = l * math.pi / 2
    return f0 + 2 * (1 - b) / (l * math.pi) * math.sin(w * a), d0 + (1 - b) * math.cos(w * a)


def yanai(b1, b2):
    def gamma(b):
        return math.sqrt(1 + b * b) - b

    def phi(a):
        r1, r2 = math.sqrt((1 - a) ** 2 + b2 * b2), math.sqrt(a * a + b1 * b1)
        return gamma(b1) * r1 + gamma(b2) * r2, -gamma(b1) * (1 - a) / r1 + gamma(b2) * a / r2
    return phi


FUNCTIONS = {"mt1": mt1, "mt2": mt2, "mt3": mt3, "mt4": yanai(0.001, 0.001), "mt5": yanai(0.01, 0.001), "mt6": yanai(0.001, 0.01)}
STEPS = [1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3]


@pytest.mark.parametrize("stp0", STEPS)
@pytest.mark.parametrize("name", sorted(FUNCTIONS))
def test_same_search_as_the_oracle(searches, name, stp0):
    theirs, ours = searches
    want = theirs(FUNCTIONS[name], stp0)
    assert len(want[0]) >= 1 and (want[1] == len(want[0]) or want[1] < 0)
    assert ours(FUNCTIONS[name], stp0) == want
    # the initial slope handed over with the first evaluation (plmDCA after its device two-loop recursion): the same search
    assert ours(FUNCTIONS[name], stp0, deferred=True) == want


def test_the_six_functions_end_both_ways(searches):
    """the sweep above is not one outcome repeated: searches that succeed after 1 .. 4 evaluations and ones that run out"""
    theirs, _ = searches
    results = {theirs(phi, s)[1] for phi in FUNCTIONS.values() for s in STEPS}
    assert {1, 2, 3, 4, LB_MAXIMUMLINESEARCH} <= results


def kink(a):        # claims slope -1 at 0 and rises at once
    return (0.0, -1.0) if a == 0 else (a, 1.0)


FAILURES = [
    ("max_linesearch", lambda a: (-a, -1.0), 1.0, LB_MAXIMUMLINESEARCH, 5),      # unbounded below: no step meets the curvature condition
    ("not_descent", lambda a: (a, 1.0), 1.0, LB_INCREASEGRADIENT, 0),
    ("zero_step", mt1, 0.0, LB_INVALIDPARAMETERS, 0),
    ("negative_step", mt1, -1.0, LB_INVALIDPARAMETERS, 0),
    ("max_step", lambda a: (-a, -1.0), 1e20, LB_MAXIMUMSTEP, 1),
    ("min_step", kink, 1e-30, LB_MINIMUMSTEP, 1),
]


@pytest.mark.parametrize("case", FAILURES, ids=[c[0] for c in FAILURES])
def test_failure_codes(searches, case):
    _, phi, stp0, code, nevals = case
    theirs, ours = searches
    want = theirs(phi, stp0)
    assert want[1] == code and len(want[0]) == nevals
    assert ours(phi, stp0) == want


def test_deferred_slope_of_a_direction_that_is_no_descent(searches):
    """Handed over late, the slope is judged after the first evaluation: the same code as the reference's early return, with
    the starting value restored (the engine takes the evaluation back out of its count)."""
    _, ours = searches
    trials, ret, stp, f = ours(lambda a: (a, 1.0), 1.0, deferred=True)
    assert (trials, ret, stp, f) == ([1.0], LB_INCREASEGRADIENT, 1.0, 0.0)
    assert ours(mt1, 0.0, deferred=True)[:2] == ([], LB_INVALIDPARAMETERS)
