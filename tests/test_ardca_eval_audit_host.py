"""The element audit of one arDCA evaluation (tests/ardca_eval_reference.py) on the CPU: the case table against the gradient
geometry of pydca_amd/csrc/ar_plan.h (through tests/ar_plan_driver.cpp), the bound against the float64 restatement
test_ardca_host.objective_ref (positive control: every element of every case) and against seven faulty variants of it (negative
controls: each has to be rejected), the dot bound against the dot kernels' order restated in float64.
tests/test_ardca_eval_audit.py runs the same audit on what the MI355X returns."""
import numpy as np
import pytest

import ardca_eval_reference as R
from test_ardca_host import objective_ref

LD = np.longdouble


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("arplan"))


_refs = {}


def ref_of(case, driver):
    """one reference and one restatement per case, the last two kept (the cases of a test run in table order)"""
    if case.name not in _refs:
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        ref = R.reference(case, R.plan_of(case, driver))
        fx, g = objective_ref(ref.x, ref.X, ref.w, case.L, case.q, R.LAMBDA_H, R.LAMBDA_J)
        _refs[case.name] = (ref, float(fx), g)
    ref, fx, g = _refs[case.name]
    return ref, fx, g.copy()


# ----------------------------------------------------------------------------- the table reaches what it claims
def test_geometry_constants(driver):
    """KC per alphabet as the kernel's comment block and the case table assume it, threads in whole waves within the launch
    bound, LDS as ar_grad_kernel lays it out and within the 160 KiB of a workgroup"""
    assert {q: driver(q)["KC"] for q in (2, 5, 8, 9, 21, 24, 25, 32)} == {2: 64, 5: 64, 8: 64, 9: 56, 21: 16, 24: 12, 25: 11, 32: 7}
    for q in range(2, 33):
        p = driver(q)
        assert (p["tile"], p["budget"], p["maxThreads"]) == (64, 56 * 1024, 512)
        assert 1 <= p["KC"] <= 64 and p["KC"] * q <= p["threads"] <= p["maxThreads"] and p["threads"] % 64 == 0 and p["threads"] - p["KC"] * q < 64
        assert p["lds"] == (p["KC"] * q * q + p["tile"] * q) * 8 + p["KC"] * p["tile"] <= 160 * 1024


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_plan_facts(driver, case):
    plan = R.plan_of(case, driver)
    assert {k: plan[k] for k in case.facts} == case.facts, case.reaches
    assert sum(plan["chunks"]) == case.L - 1 and sum(sum(t) for t in plan["tiles"]) == case.N


def test_the_table_covers_the_edges(driver):
    plans = [R.plan_of(c, driver) for c in R.CASES]
    assert {p["KC"] for p in plans} == {64, 56, 16, 12, 11, 7} and {p["QM"] for p in plans} == {8, 24, 32}
    assert {c.q for c in R.CASES} >= {2, 5, 8, 9, 21, 24, 25, 32}
    assert any(len(p["chunks"]) == 3 for p in plans) and any(p["chunks"][:2] == [p["KC"], 1] for p in plans)      # full + full + partial, full + 1
    assert any(p["idle"] == 0 and p["threads"] == 512 for p in plans) and any(0 < p["idle"] for p in plans)
    assert any(p["fieldBlocks"] == 2 for p in plans) and any(p["dotRows"] > 1 for p in plans) and any(p["oddP"] for p in plans)
    assert any(p["passes"] == 2 and len(p["tiles"][0]) == 2 and p["tiles"][0][1] < 64 for p in plans)             # a pass boundary inside a tile
    assert {c.N for c in R.CASES} >= {1, 64, 130} and any(c.saturate for c in R.CASES)
    for c in R.CASES:
        w = R.weights(c)
        if c.N >= 8:
            assert np.count_nonzero(w == 0) == 3 and w[w > 0].max() / w[w > 0].min() > 1e3
        X = R.alignment(c)
        assert X.max() < c.q and X.shape == (c.N, c.L)


def test_the_saturated_case_underflows(driver):
    case = R.BY_NAME["q5_L67_N130_saturated"]
    l, b, _v = case.saturate
    ref, _fx, _g = ref_of(case, driver)
    others = [a for a in range(case.q) if a != b]
    unobserved = ref.X[:, l, None] != np.array(others)[None, :]
    assert np.all(ref.R64[:, l, others][unobserved] == 0.0)      # W p of the other states: below the smallest double
    assert np.count_nonzero(ref.R64[:, l, others]) > 0           # ... and sequences that hold one of them: R = -W (1 - p)


# ----------------------------------------------------------------------------- positive control
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_restatement_stays_inside_the_bound(driver, case):
    """The float64 restatement has the device's rounding sequence up to the order of the sums, which the bound covers for any
    order: if it cannot stay inside the bound in every element, the bound is wrong."""
    ref, fx, g = ref_of(case, driver)
    a = R.audit(ref, fx, g)
    rel_A = float(np.max(np.abs(g.astype(LD) - ref.g).astype(np.float64) / (ref.A + ref.pen)))
    print("%s; largest error / (A + penalty) %.3e; exp %.3f ulps, log %.3f ulps (x %g); |g|^2 ratio %.4f" % (
        a.summary(), rel_A, ref.exp_ulps, ref.log_ulps, R.EXP_FACTOR, R.gnorm_ratio(g, np.sqrt(R.dot_emulated(g, g)))))
    assert a.checked == case.P
    assert a.ok, a.report()
    assert R.assert_within_bounds(ref, fx, g) == case.P


def test_two_passes_added_stay_inside_the_bound(driver):
    """the pass case's restatement as the sum of its two passes, each summed on its own"""
    ref, fx, g = ref_of(R.BY_NAME["q21_L35_N150_pass100"], driver)
    (f0, g0), (f1, g1) = rows_only(ref, slice(0, 100)), rows_only(ref, slice(100, 150))
    a = R.audit(ref, (f0 + f1) + penalty_fx(ref), with_penalty(ref, g0 + g1))
    print(a.summary())
    assert a.checked == ref.case.P and a.ok, a.report()


# ----------------------------------------------------------------------------- negative controls
MULTI = "q21_L35_N130"


def rows_only(ref, rows):
    """(sum of -W_n log P(s_n), gradient without penalty) over the given rows only, W normalised by ALL the weights"""
    case = ref.case
    f, g = objective_ref(ref.x, ref.X[rows], ref.w[rows], case.L, case.q, 0.0, 0.0)
    s = np.sum(ref.w[rows]) / np.sum(ref.w)
    return f * s, g * s


def with_penalty(ref, g):
    Lq = ref.case.L * ref.case.q
    return g + np.concatenate([2 * R.LAMBDA_H * ref.x[:Lq], 2 * R.LAMBDA_J * ref.x[Lq:]])


def penalty_fx(ref, J=True):
    Lq = ref.case.L * ref.case.q
    return R.LAMBDA_H * np.sum(ref.x[:Lq] ** 2) + (R.LAMBDA_J * np.sum(ref.x[Lq:] ** 2) if J else 0.0)


def rejected(ref, fx, g, what):
    a = R.audit(ref, fx, g, named=40)
    print(what, "->", len(a.failing), "elements out of bound, worst %.3g; fx ratio %.3g" % (a.worst, a.fx_ratio))
    for f in a.failures[:3]:
        print("   ", f)
    assert a.checked == ref.case.P and not a.ok, "fault not reported: " + what
    with pytest.raises(AssertionError):
        R.assert_within_bounds(ref, fx, g)
    return a


def block(ref, k, l):
    e = R.index_of(ref.case, k, l, 0, 0)
    return slice(e, e + ref.case.q ** 2)


def test_fault_one_addend_dropped(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    case, KC = ref.case, ref.plan["KC"]
    k, l = KC + 3, 30                                             # second chunk of site 30
    a_ = int(np.bincount(ref.X[:, k], minlength=case.q).argmax())  # the fullest bucket: the hardest one to see an addend in
    b = 7
    e = R.index_of(case, k, l, a_, b)
    ns = np.flatnonzero(ref.X[:, k] == a_)
    assert ref.m[e] == len(ns) > 10
    n = ns[np.argmax(np.abs(ref.R64[ns, l, b]))]
    g[e] -= ref.R64[n, l, b]
    a = rejected(ref, fx, g, "largest addend (sequence %d) of %s dropped" % (n, R.element_of(case, e)))
    assert a.failing.tolist() == [e]
    f = a.failures[0]
    assert (f.kind, f.k, f.l, f.a, f.b) == ("coupling", k, l, a_, b)
    assert f.writer == dict(kernel="ar_grad_kernel", block=(1, case.L - 1 - l), thread=3 * case.q + b, chunk=1)
    assert "chunk 1" in repr(f) and "thread %d" % (3 * case.q + b) in repr(f)


def test_fault_first_block_of_the_second_chunk_in_the_slot_before(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    KC, l = ref.plan["KC"], 33
    src, dst = block(ref, KC, l), block(ref, KC - 1, l)
    g[dst] = g[src]
    g[src] = 2 * R.LAMBDA_J * ref.x[src]                          # never written: its penalty term alone
    a = rejected(ref, fx, g, "block (%d, %d) written to the slot of (%d, %d)" % (KC, l, KC - 1, l))
    assert {(f.k, f.l) for f in a.failures} <= {(KC, l), (KC - 1, l)}
    assert set(a.failing) <= set(range(dst.start, dst.stop)) | set(range(src.start, src.stop)) and len(a.failing) > ref.case.q ** 2


def test_fault_one_block_transposed(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    q, s = ref.case.q, block(ref, 5, 20)
    g[s] = g[s].reshape(q, q).T.ravel()
    a = rejected(ref, fx, g, "block (5, 20) transposed")
    assert set(a.failing) <= set(range(s.start, s.stop)) and len(a.failing) > q * q // 2
    assert all(f.a != f.b for f in a.failures)


def test_fault_second_pass_overwrites_the_first(driver):
    ref, fx, g = ref_of(R.BY_NAME["q21_L35_N150_pass100"], driver)
    assert ref.plan["tiles"] == [[64, 36], [50]]
    _f1, g1 = rows_only(ref, slice(100, 150))
    a = rejected(ref, fx, with_penalty(ref, g1), "second pass overwrites the first")
    assert len(a.failing) > ref.case.P // 2


def test_fault_field_elements_past_the_first_block_not_written(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    Lq = ref.case.L * ref.case.q
    g[256:Lq] = 2 * R.LAMBDA_H * ref.x[256:Lq]
    a = rejected(ref, fx, g, "field elements from 256 on at their penalty term")
    assert a.failing.tolist() == list(range(256, Lq))
    assert a.failures[0].writer["kernel"] == "ar_field_kernel" and a.failures[0].writer["block"][0] >= 1


def test_fault_last_partial_tile_left_out(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    assert ref.plan["tiles"] == [[64, 64, 2]] and np.all(ref.w[128:] > 0)
    _f, g0 = rows_only(ref, slice(0, 128))
    a = rejected(ref, fx, with_penalty(ref, g0), "sequences 128 and 129 left out")
    # every element with one of the two among its addends, and no other
    Lq, q = ref.case.L * ref.case.q, ref.case.q
    hit = np.zeros(ref.case.P, dtype=bool)
    hit[:Lq] = True
    has = np.zeros((ref.case.L, q), dtype=bool)
    has[np.arange(ref.case.L)[None, :], ref.X[128:].astype(np.int64)] = True
    hit[Lq:] = np.broadcast_to(has[ref.iu][:, :, None], (len(ref.iu), q, q)).ravel()
    assert not np.any(hit[a.failing] == False)                    # noqa: E712
    assert len(a.failing) > 0.9 * np.count_nonzero(hit)


def test_fault_coupling_penalty_left_out_of_fx(driver):
    ref, fx, g = ref_of(R.BY_NAME[MULTI], driver)
    a = R.audit(ref, fx - R.LAMBDA_J * np.sum(ref.x[ref.case.L * ref.case.q:] ** 2), g)
    print("J penalty left out of fx -> fx ratio %.3g" % a.fx_ratio)
    assert len(a.failing) == 0 and a.fx_ratio > 1e6 and not a.ok
    with pytest.raises(AssertionError, match="fx out of bound"):
        R.assert_within_bounds(ref, fx - R.LAMBDA_J * np.sum(ref.x[ref.case.L * ref.case.q:] ** 2), g)


# ----------------------------------------------------------------------------- the dot bound
def test_dot_bound_holds_the_kernels_order_and_rejects_a_missing_stride_loop(driver):
    ref, _fx, g = ref_of(R.BY_NAME[MULTI], driver)
    assert len(g) > R.DOT_STRIDE
    ratio = R.gnorm_ratio(g, np.sqrt(R.dot_emulated(g, g)))
    print("|g|^2 in the dot kernels' order: ratio %.4f; numpy's dot: %.4f" % (ratio, R.gnorm_ratio(g, np.sqrt(np.dot(g, g)))))
    assert ratio <= 1.0 and R.gnorm_ratio(g, np.sqrt(np.dot(g, g))) <= 1.0
    assert R.gnorm_ratio(g, np.sqrt(R.dot_emulated(g, g, stride_loop=False))) > 1e6
    short = g[:1000]
    assert R.dot_emulated(short, short) == R.dot_emulated(short, short, stride_loop=False) and R.gnorm_ratio(short, np.sqrt(R.dot_emulated(short, short))) <= 1.0
    assert R.gnorm_ratio(g, float("nan")) > 1.0
