"""The element audit of the arDCA epistasis (tests/ar_epistasis_reference.py) on the CPU: the case table against the geometry
of pydca_amd/csrc/ar_epistasis_plan.h (through tests/ar_epistasis_plan_driver.cpp), the bounds against the float64
restatement of the kernel's order (positive control: every element of every case) and against planted faults of that order
(negative controls: each has to be rejected and has to move an element by at least 100 bounds, so the bounds are not slack),
the range case's preconditions.  tests/test_ar_epistasis_audit.py runs the same audit on what the MI355X returns."""
import numpy as np
import pytest

import ar_epistasis_reference as R
from test_ardca_epistasis_host import epistasis_ref, scores_ref
from test_ardca_host import log_probabilities_ref

LD = np.longdouble


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("epiplan"))


_refs = {}


def ref_of(case, driver):
    """one reference and one restatement per case"""
    if case.name not in _refs:
        ref = R.reference(case, R.plan_of(case, driver))
        _refs[case.name] = (ref,) + R.restate(ref.x, case.L, case.q, ref.w, ref.plan)
    ref, eps, d = _refs[case.name]
    return ref, eps.copy(), d.copy()


# ----------------------------------------------------------------------------- the table reaches what it claims
def test_geometry_constants(driver):
    p = driver(13, 5)
    assert (p["threads"], p["rowsPerThread"], p["colsPerThread"], p["tileR"], p["tileC"], p["rescale"]) == (512, 4, 4, 128, 64, 4)
    assert {q: driver(4, q)["QM"] for q in (2, 5, 8, 9, 21, 24, 25, 32)} == {2: 8, 5: 8, 8: 8, 9: 24, 21: 24, 24: 24, 25: 32, 32: 32}
    for q in range(2, 33):
        p = driver(7, q)
        assert p["NPRE"] == {8: 3, 24: 9, 32: 12}[p["QM"]] and p["NPRE"] * p["threads"] >= (p["tileR"] + p["tileC"]) * q
        assert p["lds"] == 2 * (p["tileR"] + p["tileC"]) * q * 8 <= 160 * 1024
        for t in p["tiles"]:
            C0 = t["ct"] * p["tileC"]
            assert t["mstart"] == C0 // q + 1 and t["steps"] == 7 - t["mstart"] >= 0 and t["mid"] == (C0 % q != 0)
            assert t["rows"] == min(p["tileR"], 7 * q - t["rt"] * p["tileR"]) > 0 and t["cols"] == min(p["tileC"], 7 * q - C0) > 0
    assert driver(9, 32)["lds"] == 98304 > 64 * 1024


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_plan_facts(driver, case):
    plan = R.plan_of(case, driver)
    assert {k: plan[k] for k in case.facts} == case.facts, case.reaches
    # every pair element is written by exactly one launched tile, in launch order heaviest first
    L, q = case.L, case.q
    owner = np.zeros((L * q, L * q), dtype=np.int64)
    for t in plan["tiles"]:
        owner[t["rt"] * 128: t["rt"] * 128 + t["rows"], t["ct"] * 64: t["ct"] * 64 + t["cols"]] += 1
    site = np.arange(L * q) // q
    assert np.all(owner[site[:, None] < site[None, :]] == 1) and owner.max() == 1
    assert plan["steps"] == sorted(plan["steps"], reverse=True)


def test_the_table_covers_the_edges(driver):
    plans = [R.plan_of(c, driver) for c in R.CASES]
    tiles = [t for p in plans for t in p["tiles"]]
    assert {p["QM"] for p in plans} == {8, 24, 32}
    assert {c.q for c in R.CASES} >= {2, 5, 8, 9, 21, 24, 25, 32}                                  # q = QM and q < QM for 8, 24 and 32
    assert any(t["mid"] for t in tiles)
    assert any(t["rows"] == 128 and t["cols"] == 64 for t in tiles)
    assert any(p["rows"] == [128] and p["cols"] == [64] for p in plans)                            # a shape with no ragged edge at all
    assert any(t["rows"] < 128 for t in tiles) and any(t["cols"] < 64 for t in tiles)
    assert any(p["skipped"] > 0 for p in plans)
    steps = {t["steps"] for t in tiles}
    assert steps >= {0, 1, 3, 4, 5} and {s % 4 for s in steps} == {0, 1, 2, 3}
    assert any(p["splits"] == 0 and max(p["steps"]) > 0 for p in plans) and any(p["splits"] == 16 for p in plans)
    assert any(p["lds"] > 64 * 1024 for p in plans)
    assert {c.scale for c in R.CASES} == {0.5, 2.0}
    for c in R.CASES:
        w = R.wildtype(c)
        assert w.shape == (c.L,) and w.max() < c.q
        if not c.planted:
            assert w[0] == 0 and w[-1] == c.q - 1


# ----------------------------------------------------------------------------- positive control
@pytest.mark.parametrize("case", R.CASES + [R.OFF_CONTRACT], ids=lambda c: c.name)
def test_restatement_stays_inside_the_bound(driver, case):
    """The float64 restatement has the device's rounding sequence: if it cannot stay inside the bound in every element, the
    bound is wrong."""
    ref, eps, d = ref_of(case, driver)
    a = R.audit(ref, eps, d)
    print(a.summary(), "; largest |eps| %.4g, largest bound %.3e" % (np.abs(eps).max(), ref.eps_bound.max()))
    assert a.checked == case.pairs * case.q ** 2 + case.L * case.q
    assert a.ok, a.report()
    R.assert_within_bounds(ref, eps, d)
    # the exact zeros: the rows a = w_k and the columns b = w_l, and nothing else
    for n, (k, l) in enumerate(zip(ref.iu, ref.ju)):
        z = np.zeros((case.q, case.q), dtype=bool)
        z[ref.w[k], :] = z[:, ref.w[l]] = True
        assert np.array_equal(ref.zero[n], z)
    assert np.all(eps[ref.zero] == 0.0) and np.all(ref.eps_bound[ref.zero] == 0) and np.all(ref.eps_bound[~ref.zero] > 0)
    assert np.all(d[ref.d_zero] == 0.0) and np.all(ref.d_bound[~ref.d_zero] > 0) and ref.d_zero.sum() == case.L


def test_restatement_is_the_factored_form(driver):
    """the restatement against the one the existing tests use (one logarithm per term there, products here)"""
    case = R.BY_NAME["q5_L13_s0.5"]
    ref, eps, d = ref_of(case, driver)
    eps_f, d_f = epistasis_ref(ref.x, case.L, case.q, ref.w)
    assert np.abs(eps - eps_f).max() <= 1e-12 and np.abs(d - d_f).max() <= 1e-12


@pytest.mark.parametrize("name", ["q5_L27_s2", "q2_L65_s0.5", "q24_L11_s2", "q32_L4_s0.5", "q2_L12_s0.5_planted"])
def test_single_mutants_by_log_probabilities(driver, name):
    """d_k(a) as log P(single mutant) - log P(wild type): the two longdouble evaluations agree, and the float64 restatement of
    the library's log P stays inside logp_reference's bound (and leaves it when one site value is dropped)"""
    case = R.BY_NAME[name]
    ref, _eps, _d = ref_of(case, driver)
    L, q = case.L, case.q
    X = R.single_mutants(ref.w, L, q)
    assert X.shape == (L * q + 1, L) and np.array_equal(X[-1], ref.w) and X[q + 1, 1] == 1 and np.array_equal(np.delete(X[q + 1], 1), np.delete(ref.w, 1))
    lp_ref, lp_bound = R.logp_reference(ref.x, L, q, X)
    route = (lp_ref[:L * q] - lp_ref[L * q]).reshape(L, q)
    assert np.abs(route - ref.d).max() <= 2.0 ** -55 * (np.abs(lp_ref).max() + 1)
    lp, site = log_probabilities_ref(ref.x, X, L, q)
    r = R.ratios_of(lp, lp_ref, lp_bound).max()
    print("%s: log P restatement / bound %.4f" % (name, r))
    assert r <= 1.0
    assert np.median(R.ratios_of(lp - site[:, L // 2], lp_ref, lp_bound)) > 100          # (a planted mutant may saturate that site: its value is 0)


@pytest.mark.parametrize("name", ["q5_L13_s0.5", "q2_L65_s2", "q21_L2_s0.5", "q25_L6_s2"])
def test_score_bounds_hold_numpy_scores(driver, name):
    """float64 NumPy scores of the restatement's table against the longdouble scores, inside the bounds, from either source"""
    case = R.BY_NAME[name]
    ref, eps, _d = ref_of(case, driver)
    for src, extra in ((eps, None), (ref.eps, ref.eps_bound)):
        fn, fb = R.fn_reference(src, case.q, extra)
        apc, ab = R.apc_reference(fn, fb, case.L)
        with np.errstate(divide="ignore", invalid="ignore"):
            r_fn = R.score_ratios(scores_ref(eps, case.L, case.q, False), fn, fb).max()
            r_apc = R.score_ratios(scores_ref(eps, case.L, case.q, True), apc, ab).max()
        print("%s: FN ratio %.4f, APC ratio %.4f (%s source)" % (name, r_fn, r_apc, "own" if extra is None else "reference"))
        assert r_fn <= 1.0 and r_apc <= 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            assert R.score_ratios(scores_ref(eps, case.L, case.q, False) * (1 + 1e-9) + 1e-9, fn, fb).max() > 100


# ----------------------------------------------------------------------------- negative controls
def rejected(ref, eps, d, what):
    a = R.audit(ref, eps, d, named=40)
    moved = max(a.worst, a.worst_d)
    print("%s -> %d elements out of bound, moved by %.3g bounds" % (what, len(a.failing) + len(a.failing_d), moved))
    for f in a.failures[:3]:
        print("   ", f)
    assert not a.ok, "fault not reported: " + what
    assert moved >= 100.0, "the bound is slack: %s moves no element by 100 bounds" % what
    with pytest.raises(AssertionError):
        R.assert_within_bounds(ref, eps, d)
    return a


def faulty(ref, fault):
    return R.restate(ref.x, ref.case.L, ref.case.q, ref.w, ref.plan, fault)


def test_fault_one_later_site_dropped(driver):
    ref, _eps, d = ref_of(R.BY_NAME["q21_L13_s0.5"], driver)
    q, C, m = 21, 64 + 5, 7                                        # column (site 3, state 6) of the second column tile
    assert ref.w[3] != 6
    a = rejected(ref, faulty(ref, ("drop", C, m))[0], d, "site 7 dropped from the product of column (3, 6)")
    assert len(a.failing) > 0 and all((f.l, f.b) == (3, 6) for f in a.failures if f.what == "eps")
    assert {(int(ref.ju[i[0]]), int(i[2])) for i in a.failing} == {(3, 6)}
    assert len(a.failing) == 3 * (q - 1)                           # every row (k, a), k < 3, a != w_k
    f = a.failures[0]
    assert f.tile == (0, 1) and f.steps == 9 and f.joined == 9 and "tile (row 0, column 1) of 9 steps" in repr(f)


def test_fault_column_joins_at_its_own_site(driver):
    ref, _eps, d = ref_of(R.BY_NAME["q5_L26_s0.5"], driver)
    C = 70                                                         # site 14 in the tile that streams the sites from 13 on
    assert ref.w[14] != 0 and R.tile_of(ref.plan, 0, C)["mstart"] == 13
    a = rejected(ref, faulty(ref, ("join_ge", C))[0], d, "column (14, 0) joins at m >= l")
    assert {(int(ref.ju[i[0]]), int(i[2])) for i in a.failing} == {(14, 0)}


def test_fault_one_split_exponent_off_by_one(driver):
    ref, _eps, d = ref_of(R.BY_NAME["q2_L65_s0.5"], driver)
    k, l = 1, 2
    a_, b = 1 - int(ref.w[k]), 1 - int(ref.w[l])
    a = rejected(ref, faulty(ref, ("esum", k * 2 + a_, l * 2 + b, 5))[0], d, "the sixth split of (1, 2, %d, %d) adds one to the exponent" % (a_, b))
    assert [tuple(i) for i in a.failing] == [(R.pair_index(65, k, l), a_, b)]
    assert abs(abs(a.failures[0].dev - a.failures[0].ref) - np.log(2)) < 1e-9 and a.failures[0].steps == 64


def test_split_alignment_shows_only_beyond_the_contract(driver):
    """Counting the splits from l + 1 instead of from the tile's mstart.  The split is exact and a product's rounding does not
    depend on its exponent, so while every 4 consecutive steps stay within 2^+-1000 the two counts carry the same mantissas and
    differ only in how the last logarithm and esum ln 2 share the result: both are inside the bound, on the range case and on
    a multi-tile case (asserted), and no audit of values can tell them apart there.  The fault shows once a run of 4 that the
    wrong count forms leaves the range while the runs of the right count stay inside: the off-contract model."""
    for case in (R.RANGE, R.BY_NAME["q21_L13_s2"], R.BY_NAME["q5_L26_s0.5"]):
        ref, eps, d = ref_of(case, driver)
        assert any(t["cols"] > case.q for t in ref.plan["tiles"])      # a tile of more than one site: columns whose l + 1 is not mstart
        wrong = faulty(ref, ("count_from_l",))[0]
        a = R.audit(ref, wrong, d)
        print("%s, splits counted from l + 1: worst ratio %.4f, largest difference from the right count %.3e" % (case.name, a.worst, np.abs(wrong - eps).max()))
        assert a.ok and np.abs(wrong - eps).max() <= 2 * ref.eps_bound.max()
    off, eps_off, d_off = ref_of(R.OFF_CONTRACT, driver)
    e = (R.pair_index(12, 0, 1), 1, 1)
    assert off.window[e] > 1000 * np.log(2) and np.isfinite(eps_off[e])
    a = rejected(off, faulty(off, ("count_from_l",))[0], d_off, "splits counted from l + 1 (off-contract model)")
    assert e in [tuple(i) for i in a.failing]


def test_fault_block_transposed(driver):
    ref, eps, d = ref_of(R.BY_NAME["q9_L15_s0.5"], driver)
    p = R.pair_index(15, 4, 9)
    eps[p] = eps[p].T.copy()
    a = rejected(ref, eps, d, "block (4, 9) transposed")
    assert {int(i[0]) for i in a.failing} == {p} and len(a.failing) > 9 * 9 // 2


def test_fault_last_ragged_row_tile_not_written(driver):
    ref, _eps, d = ref_of(R.BY_NAME["q5_L27_s0.5"], driver)
    last = ref.plan["tiles"][-1]
    assert (last["rt"], last["ct"], last["rows"], last["cols"]) == (1, 2, 7, 7)
    a = rejected(ref, faulty(ref, ("skip_tile", 1, 2))[0], d, "tile (1, 2), the ragged last row tile, not written")
    assert {(int(ref.iu[i[0]]), int(ref.ju[i[0]])) for i in a.failing} == {(25, 26)}
    # rows 128 and 129 are the states 3 and 4 of site 25: those rows, less the wild type's, times the 4 mutant columns
    assert len(a.failing) == len({3, 4} - {int(ref.w[25])}) * 4


def test_fault_second_run_read_from_the_wrong_offset(driver):
    ref, eps, d = ref_of(R.BY_NAME["q21_L13_s0.5"], driver)
    a = rejected(ref, faulty(ref, ("b_offset", 1))[0], d, "column tile 1 reads its second run from offset C0 instead of C0 q")
    cols = {int(ref.ju[i[0]]) * 21 + int(i[2]) for i in a.failing}
    assert cols <= set(range(64, 128)) and len(cols) > 32
    assert np.array_equal(faulty(ref, ("b_offset", 0))[0], eps)   # C0 = 0: the same offset


def test_fault_wild_type_rows_not_zeroed(driver):
    ref, _eps, d = ref_of(R.BY_NAME["q8_L17_s2"], driver)
    bad = faulty(ref, ("keep_wt_rows",))[0]
    a = rejected(ref, bad, d, "the rows a = w_k not zeroed")
    assert all(int(i[1]) == int(ref.w[ref.iu[i[0]]]) for i in a.failing) and np.isinf(a.worst)


def test_fault_single_site_term_dropped(driver):
    ref, eps, d = ref_of(R.BY_NAME["q24_L11_s0.5"], driver)
    a_ = (int(ref.w[2]) + 1) % 24
    d[2, a_] -= float(ref.term[2, 7, a_])
    a = rejected(ref, eps, d, "site 7's term left out of d_2(%d)" % a_)
    assert [tuple(i) for i in a.failing_d] == [(2, a_)] and len(a.failing) == 0


# ----------------------------------------------------------------------------- the range case
def test_the_range_case_needs_the_split_and_keeps_the_contract(driver):
    ref, eps, _d = ref_of(R.RANGE, driver)
    e = (R.pair_index(12, 0, 1), 1, 1)
    total = -ref.ln_r_sum[e] / np.log(2)                           # the product of the r_m is 2^-total
    print("range case: product 2^-%.1f, largest run of 4 steps 2^+-%.1f, eps %.17g (restatement %.17g), bound %.3e" % (
        total, ref.window.max() / np.log(2), float(ref.eps[e]), eps[e], ref.eps_bound[e]))
    assert total > 1100 and float(ref.eps[e]) > 1100 * np.log(2)
    assert ref.window.max() <= 1000 * np.log(2)                    # the header's contract, on every element
    assert np.all(np.isfinite(eps)) and abs(eps[e] - float(ref.eps[e])) <= ref.eps_bound[e] < 1e-11
    # a float64 product without the split: 0, and an infinite eps
    plain = R.restate(ref.x, 12, 2, ref.w, dict(ref.plan, rescale=1 << 20))[0]
    assert np.isinf(plain[e])
