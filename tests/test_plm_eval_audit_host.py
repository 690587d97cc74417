"""The element audit of one plmDCA evaluation (tests/plm_eval_reference.py) on the CPU: the longdouble reference against the
float64 oracle, the case table against the launch planner, the bound against an emulation of the stages in the engine's type
(positive controls: two summation orders, every case, ratios printed) and against eight faulty variants of that emulation
(negative controls: each has to be reported with the right element, strip and tile).  tests/test_plm_eval_audit.py runs the
same audit on what the MI355X returns."""
import numpy as np
import pytest

import plm_eval_reference as R

LD = np.longdouble


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("plan"))


_refs = {}


def ref_of(case, driver):
    """one reference per case, the last two kept (the cases of a test run in table order)"""
    if case.name not in _refs:
        while len(_refs) >= 2:
            _refs.pop(next(iter(_refs)))
        _refs[case.name] = R.reference(case, R.plan_of(case, driver))
    return _refs[case.name]


# ----------------------------------------------------------------------------- the table reaches what it claims
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_plan_facts(driver, case):
    plan = R.plan_of(case, driver)
    assert plan["P"] == case.P
    assert {k: plan[k] for k in case.facts} == case.facts, case.reaches


def test_the_table_covers_the_paths(driver):
    plans = {c.name: R.plan_of(c, driver) for c in R.CASES}
    f32 = [p for c, p in zip(R.CASES, plans.values()) if c.bits == 32]
    f64 = [p for c, p in zip(R.CASES, plans.values()) if c.bits == 64]
    assert {p["pairJT"] for p in f32 if p["pairs"]} == {10, 11, 12}
    assert {p["scatWaves"] for p in f64} == {4, 8, 16} and {p["scatPerBlock"] for p in f64} == {0, 1}
    assert any(p["scatSplit"] == 2 for p in f32) and any(p["scatSplit"] > 2 for p in f32) and any(p["scatRemCT"] for p in f32)
    assert {c.mode for c in R.CASES} == {"chunked", "serial", "exact"} and any(c.halo for c in R.CASES)
    # odd L on the site-pair alphabet, a sequence count of one past a tile / a logits workgroup
    assert any(p["pairs"] and c.L % 2 for c, p in zip(R.CASES, plans.values())) and any(c.N % 128 == 1 for c in R.CASES)


# ----------------------------------------------------------------------------- the reference against the float64 oracle
SMALL = [R.Case(64, 5, 90, 7, "oracle, carry", {}, mode="serial"), R.Case(64, 21, 70, 5, "oracle, carry", {}, mode="serial"),
         R.Case(64, 5, 130, 6, "oracle, no carry", {}, mode="exact"), R.Case(64, 21, 40, 4, "oracle, no carry", {}, mode="exact")]


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_reference_agrees_with_the_oracle(driver, oracle_plm, case):
    """The oracle is a float64 implementation of the same chain and sums: it has to lie inside the float64 bound of the
    longdouble reference -- its own rounding -- in every element."""
    ref = R.reference(case, R.plan_of(case, driver))
    fx, g = oracle_plm.gradient(ref.X, ref.w, case.q, R.LAMBDA_H, R.LAMBDA_J, ref.x, carry=case.mode != "exact")
    a = R.audit(ref, fx, g)
    print(a.summary())
    assert a.checked == case.P and a.ok, a.report()
    assert abs(fx - float(ref.fx)) <= 4e-16 * abs(fx)


def test_reference_with_a_halo_is_the_difference_of_two_oracle_runs(driver, oracle_plm):
    """what test_sharded_contexts_sum_to_unsharded relies on: the owned rows' sums = (all rows) - (the rows in front), the chain
    running through; here without the regulariser, which the difference cancels"""
    full = R.Case(64, 5, 200, 6, "all rows", {}, mode="serial")
    head = R.Case(64, 5, 48, 6, "the rows in front", {}, mode="serial", head_of=full)
    tail = R.Case(64, 5, 200, 6, "owned rows", {}, mode="serial", halo=48, head_of=full)
    rf, rh, rt = (R.reference(c, R.plan_of(c, driver)) for c in (full, head, tail))
    assert np.array_equal(rt.X, rf.X) and np.array_equal(rh.X, rf.X[:48])
    reg_g = np.concatenate([2 * R.LAMBDA_H * rf.x[:30], 2 * R.LAMBDA_J * rf.x[30:]]).astype(LD)
    # the three references among themselves: longdouble rounding only
    assert np.max(np.abs((rt.g - reg_g) - ((rf.g - reg_g) - (rh.g - reg_g))) / rt.A) < 2.0 ** -58
    out = [oracle_plm.gradient(r.X, r.w, 5, R.LAMBDA_H, R.LAMBDA_J, r.x, carry=True) for r in (rf, rh)]
    diff = out[0][1].astype(LD) - out[1][1].astype(LD)
    assert np.all(np.abs(diff - (rt.g - reg_g)) <= rf.bound + rh.bound)
    xL = rf.x.astype(LD)
    reg = LD(R.LAMBDA_H) * R.fsum_ld(xL[:30] ** 2) + LD(R.LAMBDA_J) * R.fsum_ld(xL[30:] ** 2)
    assert abs(LD(out[0][0]) - LD(out[1][0]) - (rt.fx - reg)) <= rf.fx_bound + rh.fx_bound


def test_the_exact_limb_sums_are_math_fsum(driver):
    case = R.BY_NAME["f32_q21_300x7"]
    plan = R.plan_of(case, driver)
    a, b = R.reference(case, plan), R.reference(case, plan, sums="fsum")
    assert np.max(np.abs(a.g - b.g) / a.A) < 2.0 ** -60
    rng = np.random.default_rng(3)
    V = (rng.standard_normal((400, 3)) * np.exp(-20 * rng.random((400, 3)))).astype(LD).clip(-1, 1) / 3
    oh = (rng.integers(0, 4, size=400)[:, None] == np.arange(4)[None, :]).astype(np.float64)
    assert np.max(np.abs(R.exact_group_sums(oh, V) - R.exact_group_sums_fsum(oh, V))) <= 400 * R.CUT_OFF + 2.0 ** -62      # the two longdouble roundings of sums below 1


def test_dyadic_parameters_make_the_logits_exact():
    for case in R.CASES:
        x = R.parameters(case).astype(np.float64)
        Lq = case.L * case.q
        assert np.array_equal(x[:Lq] * 64, np.rint(x[:Lq] * 64)) and np.abs(x[:Lq]).max() <= 2
        assert np.array_equal(x[Lq:] * 256, np.rint(x[Lq:] * 256)) and np.abs(x[Lq:]).max() <= 0.25
    case = R.BY_NAME["f32_q5_641x43"]
    X = R.alignment(case)
    freq = np.stack([np.bincount(X[:, i], minlength=5) for i in range(case.L)])
    assert freq.max() > 4 * np.maximum(freq.min(), 1).min() and len({tuple(r) for r in freq}) == case.L      # skewed, and differently per site
    w = R.weights(case)
    assert set(np.rint(1 / w).astype(int)) == set(range(1, 9))


def test_every_site_has_buckets_that_resolve_one_addend():
    """The first term of the bound is gamma(m + 2) A with A about m typical addends: one missing addend of typical size stands out
    only while m (m + 2) u < 1, m < 4096 in float32.  The skewed state frequencies give every site of every case a state whose
    bucket is small enough to show it four times over -- the deep buckets of 10000 x 13 (up to 4948 sequences) would not."""
    for case in R.CASES:
        X, u = R.alignment(case)[case.halo:], R.unit_roundoff(case.dtype)
        for i in range(case.L):
            m = np.bincount(X[:, i], minlength=case.q)
            m = m[m > 0].min()
            assert 4 * m * (m + 2) * u < 1, (case.name, i, int(m))


# ----------------------------------------------------------------------------- positive controls
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_emulation_stays_inside_the_bound(driver, case):
    """The stages in the engine's own type with NumPy's exp, in two summation orders, on every case: if the reference's own
    arithmetic cannot stay inside the bound, the bound is wrong."""
    ref = ref_of(case, driver)
    for order in ("sequential", "blas"):
        fx, g = R.emulate(ref, order)
        a = R.audit(ref, fx, g)
        print("%s [%s]: exp %.3f ulps, log %.3f ulps (x %g)" % (a.summary(), order, ref.exp_ulps, ref.log_ulps, R.EXP_FACTOR))
        assert a.checked == case.P
        assert a.ok, a.report()


# ----------------------------------------------------------------------------- negative controls
def rows_of(f):
    return {(v["row_site"], v["row_state"]) for v in f.views}


def caught(ref, fault, order="sequential"):
    fx, g = R.emulate(ref, order, fault=fault)
    a = R.audit(ref, fx, g, named=40)
    print(fault, "->", len(a.failing), "elements out of bound, worst %.3g" % a.worst)
    for f in a.failures[:3]:
        print("   ", f)
    assert a.checked == ref.case.P and len(a.failing) > 0 and not a.ok, "fault %r not reported" % (fault,)
    return a


def all_failing(ref, a):
    return [R.element_of(ref.case, e) for e in a.failing]


def test_fault_last_row_of_a_tile_dropped(driver):
    ref = ref_of(R.BY_NAME["f32_q5_641x43"], driver)
    j, tile = 5, 2
    n = 128 * tile + 127
    b = int(ref.X[n, j])
    a = caught(ref, ("drop_tile_last_row", j, tile))
    for kind, i_, j_, a_, b_ in all_failing(ref, a):        # only sums of row (site 5, that state)
        assert (kind == "coupling" and ((j_, b_) == (j, b) or (i_, a_) == (j, b))) or (kind == "field" and j == 0), (kind, i_, j_, a_, b_)
    named = [f for f in a.failures if f.explained and f.explained[0] == "missing addend"]
    assert named and all(f.explained[2] == (n, tile, 0) for f in named)
    assert all(any(v["first"][1] <= tile <= v["last"][1] and (v["row_site"], v["row_state"]) == (j, b) for v in f.views) for f in named)


def test_fault_one_slab_of_one_strip_not_added(driver):
    ref = ref_of(R.BY_NAME["f32_q21_3000x60"], driver)
    strip, split = 3, 1
    assert ref.plan["scatSplit"] == 2 and ref.plan["strips"] == 10
    a = caught(ref, ("drop_slab", strip, split), order="blas")
    for f in a.failures:
        assert strip in {v["strip"] for v in f.views}
        assert f.explained and f.explained[0] == "missing slab" and f.explained[2][2] == split, f
    cols = {e[1] for e in all_failing(ref, a)} | {e[2] for e in all_failing(ref, a) if e[2] is not None}
    assert any(128 * strip <= s * 21 < 128 * (strip + 1) or 128 * strip <= s * 21 + 20 < 128 * (strip + 1) for s in cols)
    for kind, i_, j_, a_, b_ in all_failing(ref, a):
        hit = [(s * 21 + st) // 128 for s, st in ((i_, a_), (j_, b_)) if s is not None]
        assert strip in hit


def test_fault_padding_site_of_an_odd_length_contributes(driver):
    ref = ref_of(R.BY_NAME["f32_q5_641x43"], driver)
    a = caught(ref, ("padding_site",))
    for kind, i_, j_, a_, b_ in all_failing(ref, a):
        assert kind == "coupling" and (j_, b_) == (42, 0), (kind, i_, j_, a_, b_)
    assert all((42, 0) in rows_of(f) for f in a.failures)


def test_fault_two_states_swapped(driver):
    ref = ref_of(R.BY_NAME["f32_q21_300x7"], driver)
    a = caught(ref, ("swap_states", 3, 2, 5))
    for kind, i_, j_, a_, b_ in all_failing(ref, a):
        assert kind == "coupling" and ((j_ == 3 and b_ in (2, 5)) or (i_ == 3 and a_ in (2, 5))), (kind, i_, j_, a_, b_)


def test_fault_conditional_from_the_transposed_block(driver):
    ref = ref_of(R.BY_NAME["f32_q21_300x7"], driver)
    a = caught(ref, ("transposed_block", 1, 4))
    for kind, i_, j_, a_, b_ in all_failing(ref, a):
        assert (kind, i_, j_) == ("coupling", 1, 4) and a_ != b_
    assert len(a.failing) > 100


def test_fault_halo_row_summed(driver):
    ref = ref_of(R.BY_NAME["f32_q5_1000x33_halo64"], driver)
    a = caught(ref, ("halo_row",))
    named = [f for f in a.failures if f.explained]
    assert named and all(f.explained[0] == "halo row summed" and f.explained[2][0] == 63 for f in named)
    for kind, i_, j_, a_, b_ in all_failing(ref, a):
        assert kind == "field" or ref.X[63, j_] == b_ or ref.X[63, i_] == a_


def test_fault_field_column_shifted(driver):
    ref = ref_of(R.BY_NAME["f32_q21_300x7"], driver)
    a = caught(ref, ("shift_field", 2))
    assert {(k, i_) for k, i_, _, _, _ in all_failing(ref, a)} == {("field", 2)}


def test_fault_warm_up_cut_to_four_steps(driver):
    ref = ref_of(R.BY_NAME["f32_q21_300x7"], driver)
    a = caught(ref, ("warm_up_4",))
    # every scan chunk but the first starts from a carry that is 2^-4, not 2^-40, off: the error sits in the first rows of the
    # chunks 32 k, k >= 1, and every element reported has such a row among its addends
    assert ref.plan["chunk"] == 32
    for e in a.failing:
        ns = np.concatenate([v["addends"] for v in R.conditionals(ref, e)])
        assert np.any((ns >= 32) & (ns % 32 < 8)), R.element_of(ref.case, e)


def test_a_faulty_device_gradient_fails_the_gpu_assertion_by_name(driver):
    """what tests/test_plm_eval_audit.py asserts of the device, fed the emulation with one fault in place of the device's output"""
    ref = ref_of(R.BY_NAME["f32_q5_641x43"], driver)
    fx, g = R.emulate(ref, "sequential", fault=("drop_tile_last_row", 5, 2))
    with pytest.raises(AssertionError) as info:
        R.assert_within_bounds(ref, fx, g)
    text = str(info.value)
    b = int(ref.X[383, 5])
    assert "sum of row (site 5, state %d)" % b in text and "strip 0" in text and "site group 0" in text
    assert "missing addend of sum 2" in text and "(383, 2, 0)" in text
    fx, g = R.emulate(ref, "sequential")
    assert R.assert_within_bounds(ref, fx, g).checked == ref.case.P
