"""The element audit of the sequence-model kernels (tests/potts_audit_reference.py) on the CPU: the case table against the launch
geometry of pydca_amd/csrc/potts_plan.h (through tests/potts_plan_driver.cpp), the limits that geometry has to keep for every
alphabet, the bounds against the float64 restatements of the suite (positive control: every element of the restatements' outputs, on 600 queries for the energies and on 70
for the conditionals, 16 where L > 131, and the margin condition of every draw) and against faulty variants (negative controls: each has to be rejected by the audit functions that
tests/test_potts_audit.py calls on what the MI355X returns)."""
import numpy as np
import pytest

import potts_audit_reference as R
import test_potts_sampling as sampling

LDS_LIMIT = 160 * 1024
NAMES = ["q5_L131_f32", "q5_L33_f64", "q21_L20_f32", "q21_L19_f64", "q5_L643_f32", "q21_L513_f32", "q2_L2_mf", "q2_L70_mf", "q4_L49_mf",
         "q6_L33_mf", "q8_L20_mf", "q8_L131_mf", "q9_L20_mf", "q9_L47_mf", "q16_L130_mf", "q16_L27_mf", "q24_L9_mf", "q25_L11_mf", "q25_L46_mf",
         "q32_L11_mf", "q32_L20_mf", "q21_L8_mf", "q2_L643_mf", "q9_L513_mf", "q25_L513_mf"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("pottsplan"))


# ----------------------------------------------------------------------------- the table reaches what it claims
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_plan_facts(driver, case):
    plan = R.plan_of(case, driver)
    assert {k: plan[k] for k in case.facts} == case.facts, case.reaches
    if case.mf:
        X, _w = R.mf_alignment(case)
        assert X.shape[1] == case.L and X.max() < case.q


def test_the_table_covers_the_edges(driver):
    # the name list pins every case: one taken out or added is a decision made here too.  The union below needs most of them
    # on its own; the largest q of a tile size, the stage-shape alignments and the toy golden are asserted as such
    assert [c.name for c in R.CASES] == NAMES
    plans = [(c, R.plan_of(c, driver)) for c in R.CASES]

    def reached(key, family, elem=None, where=lambda c, p: True):
        return {p[key] for c, p in plans if family in c.families and (elem is None or c.elem == elem) and where(c, p)}

    plm = lambda c, p: c.src != "mf"                               # noqa: E731
    mf = lambda c, p: c.src == "mf"                                # noqa: E731
    # kind 0 is q = 5 and q = 21: two tile sizes and two accumulator counts per type, TB 16 and 4
    assert reached("TS", "energy", 4, plm) == {24, 6} and reached("TS", "energy", 8, plm) == {16, 4}
    for elem in (4, 8):
        for key, family in (("QM", "pll"), ("sQM", "sample"), ("sQM", "ais")):
            assert reached(key, family, elem, plm) == {8, 24}
        assert reached("TB", "bm", elem) == {16, 4}
    assert reached("bmRagged", "bm") == {0, 1}
    # kind 1 is float64 at every alphabet
    assert reached("TS", "energy", 8, mf) == {24, 16, 12, 8, 6, 4, 3}
    for key, family in (("QM", "pll"), ("sQM", "sample"), ("sQM", "ais")):
        assert reached(key, family, 8, mf) == {8, 24, 32}
    assert reached("CPT", "pll") == {1, 2} and reached("KPB", "pll") == {1, 3, 4}
    assert 1 in reached("siteLast", "pll") and any(p["siteLast"] == p["CJ"] and p["siteChunks"] > 1 for c, p in plans if "pll" in c.families)
    assert 1 in reached("nch", "sample") and max(reached("nch", "sample")) >= 3
    assert any(p["sLast"] == p["sCJ"] for c, p in plans if "sample" in c.families) and 1 in reached("sLast", "sample")
    for qm in (8, 24, 32):
        assert reached("res", "sample", None, lambda c, p: p["sQM"] == qm) == {0, 1}
    assert reached("res", "sample", 4) == {0, 1} and reached("res", "sample", 8) == {0, 1} and reached("res", "ais") == {0, 1}
    assert len({p["TS"] for c, p in plans if "energy" in c.families and p["tpg"] > 1}) >= 2
    assert {c.q for c in R.CASES if c.src == "mf"} >= {2, 8, 9, 24, 25, 32} and {c.q for c in R.CASES if c.src != "mf"} == {5, 21}
    for ts, q in ((24, 4), (16, 6)):                               # float64: the largest alphabet of the two large tiles
        assert any(c.q == q and p["TS"] == ts for c, p in plans if "energy" in c.families and c.elem == 8) and driver(q + 1, 8, 50)["TS"] < ts
    assert {c.mf for c in R.CASES} >= {"N1_L2_q2", "N700_L20_q8", "N700_L20_q9", "N700_L20_q32", "mf_toy_protein"}
    assert any(p["eLds"] == p["eBudget"] for c, p in plans) and any(p["chunkVals"] == p["regVals"] for c, p in plans if "sample" in c.families)


def test_limits_for_every_alphabet(driver):
    """what the code keeps only implicitly: every LDS size within the 160 KiB of a workgroup, the sampler's chunk within the
    registers that stage it (one more value would be dropped silently), the energy tile within its budget"""
    for q in range(2, 33):
        for elem in (4, 8):
            for L in (1, 2, 131, 512, 513, 5000):
                p = driver(q, elem, L)
                assert p["TS"] in (24, 16, 12, 8, 6, 4, 3) and p["eLds"] == p["TS"] ** 2 * q * q * elem <= p["eBudget"] == 72 * 1024
                assert p["G"] <= 128 and (p["G"] - 1) * p["tpg"] < p["ntiles"] <= p["G"] * p["tpg"]
                assert p["QM"] == p["sQM"] >= q and p["QM"] in (8, 24, 32) and p["QM"] % (16 // elem) == 0
                assert 1 <= p["CJ"] <= 16 and p["CJ"] * p["QM"] ** 2 * elem <= 16 * 1024 and q * q <= 256 * p["KPB"] and p["CPT"] in (1, 2)
                assert p["CJ"] * 512 <= 16 * 256 * p["CPT"]
                assert p["siteLds"] <= LDS_LIMIT and p["siteLds"] >= 2 * p["CJ"] * (q * p["QM"] * elem + 512)
                assert p["sCJ"] >= 4 and p["sCJ"] % 4 == 0 and p["chunkVals"] == p["sCJ"] * q * q <= p["regVals"] == 256 * (32 if elem == 4 else 16)
                assert p["sCJ"] * q * p["QM"] * elem <= 40 * 1024 and p["sLds"] <= LDS_LIMIT and p["res"] == int(L <= p["residentL"])
                assert p["TB"] in (16, 4, 2) and p["bmLds"] == p["TB"] ** 2 * q * q * 4 <= 64 * 1024 and p["bmLds"] + p["bmStatic"] <= LDS_LIMIT


# ----------------------------------------------------------------------------- positive control
@pytest.mark.parametrize("case", R.cases_of("energy"), ids=lambda c: c.name)
def test_energy_restatement_stays_inside_the_bound(driver, case):
    plan = R.plan_of(case, driver)
    h, Jp = R.model_of(case, R.SIGMA_PLL)
    X = R.queries(case, 32 if case.L > 131 else R.N_QUERIES)
    ref = R.energy_reference(h, Jp, X, plan["G"])
    E, _S = R._terms(h, Jp, X)
    a = R.audit_energies(ref, E)
    s = R.scan_reference(h, Jp, X[3 % len(X)])
    b = R.audit_scan(s, R.mutation_ref(h, Jp, X[3 % len(X)].astype(np.int64)))
    print(a.summary(), ";", b.summary())
    assert a.checked == len(X) and b.checked == case.L * case.q
    R.assert_ok(a, b)
    if case.L <= 47:                                               # the tile order restated: inside the bound too
        R.assert_ok(R.audit_energies(ref, R.energy_by_tiles(h, Jp, X, plan)))


@pytest.mark.parametrize("case", R.cases_of("pll"), ids=lambda c: c.name)
def test_conditionals_restatement_stays_inside_the_bound(driver, case):
    h, Jp = R.model_of(case, R.SIGMA_PLL)
    X = R.queries(case, 16 if case.L > 131 else 70)
    ref = R.cond_reference(h, Jp, X)
    pll, site, cond, _umax = R.conditionals_ref(h, Jp, X)
    audits = R.audit_conditionals(ref, pll, site, cond)
    print("; ".join(a.summary() for a in audits), "; exp %.3f ulps, log %.3f ulps" % (ref.exp_ulps, ref.log_ulps))
    assert audits[0].checked == X.size * case.q
    R.assert_ok(*audits)


@pytest.mark.parametrize("case", [c for c in R.cases_of("sample") if not c.device_model_only], ids=lambda c: c.name)
def test_every_draw_keeps_the_margin(case):
    """sample_reference asserts |cum - r| / T >= 10 eps_draw for every draw of every run of the case (q25_L513_mf has its model on
    the device only; tests/test_potts_audit.py asserts the same there)"""
    h, Jp = R.model_of(case, R.SIGMA_SAMPLE)
    runs = R.sample_reference(case, h, Jp)
    need = R.MARGIN_FACTOR * R.eps_draw(case.q, case.L, max(r[0] for r in runs), R.model_sabs(h, Jp))
    print("%s: smallest margin %.3g, needed %.3g" % (case.name, min(r[-1] for r in runs), need))
    assert len(runs) == len(R.sample_runs(case))


@pytest.mark.parametrize("case", R.cases_of("ais"), ids=lambda c: c.name)
def test_ais_restatement_stays_inside_the_bound(driver, case):
    plan = R.plan_of(case, driver)
    h, Jp = R.model_of(case, R.SIGMA_SAMPLE)
    for k, run in enumerate(R.ais_runs(case)):
        ref = R.ais_reference(case, h, Jp, plan["G"], run, k)
        K, s, h0, betas, c0 = run
        chains = np.arange(c0, c0 + case.chains)
        X, logw, _lz0, _m = R.ais_ref(h, Jp, h if h0 is None else h0, K, s, ref.args["seed"], chains, betas)
        audits = R.audit_ais(ref, logw, X)
        print("; ".join(a.summary() for a in audits), "; smallest margin %.3g" % ref.margin)
        R.assert_ok(*audits)


# ----------------------------------------------------------------------------- negative controls
def rejected(audits, what):
    audits = audits if isinstance(audits, (tuple, list)) else [audits]
    bad = [a for a in audits if not a.ok]
    print(what, "->", "; ".join("%s: %d out of bound, worst %.3g%s" % (a.what, len(a.failing), a.worst, " " + "; ".join(a.identities) if a.identities else "")
                                for a in audits))
    assert bad, "fault not reported: " + what
    with pytest.raises(AssertionError):
        R.assert_ok(*audits)
    return bad


COND_CASE = "q9_L47_mf"


@pytest.fixture(scope="module")
def cond_ref(driver):
    case = R.BY_NAME[COND_CASE]
    h, Jp = R.model_of(case, R.SIGMA_PLL)
    X = R.queries(case, 40)
    return case, R.plan_of(case, driver), h, Jp, X, R.cond_reference(h, Jp, X)


@pytest.mark.parametrize("fault", [None, "untransposed", "self", "ragged", "next_fields", "no_last_state", "padding_lane"])
def test_fault_in_the_site_conditionals(cond_ref, fault):
    """the block of a pair read untransposed for j < i; the neighbour j = i included; the last neighbour of a ragged chunk
    dropped; the fields of site i + 1; state q - 1 left out of the softmax; the padding lane q read as a state"""
    case, plan, h, Jp, X, ref = cond_ref
    assert case.L % plan["CJ"] != 0
    table = fault if fault in ("untransposed", "self", "ragged", "next_fields") else None
    u, _A = R.site_table(h, Jp, X, np.float64, fault=table, plan=plan)
    cond, site, pll, _lz = R.conditionals_of(u, X, fault=None if table else fault)
    audits = R.audit_conditionals(ref, pll, site, cond)
    if fault is None:                                              # the faultless variant passes: the faults alone are rejected
        R.assert_ok(*audits)
        return
    bad = rejected(audits, fault)
    assert any(a.what == "cond" for a in bad)
    if fault == "untransposed":                                    # site 0 has no j < i
        assert set(audits[0].failing[:, 1]) == set(range(1, case.L))


def test_fault_identities_between_the_outputs(cond_ref):
    case, _plan, h, Jp, X, ref = cond_ref
    pll, site, cond, _ = R.conditionals_ref(h, Jp, X)
    s2 = site.copy()
    s2[5, 7] = np.nextafter(s2[5, 7], 0)
    assert any("site != cond" in s for s in rejected(R.audit_conditionals(ref, pll, s2, cond), "site one ulp off cond")[0].identities)
    p2 = site[:, ::-1].cumsum(axis=1)[:, -1]                         # the descending-i sum
    assert np.any(p2 != pll)
    assert any("PLL" in s for s in rejected(R.audit_conditionals(ref, p2, site, cond), "PLL summed in descending i")[0].identities)


def test_fault_in_the_scan(cond_ref):
    case, plan, h, Jp, X, _ref = cond_ref
    w = X[3]
    ref = R.scan_reference(h, Jp, w)
    rows = np.arange(case.L)
    for fault in ("untransposed", "self", "ragged"):
        S, _A = R.site_sums(h, Jp, w, np.float64, fault=fault, plan=plan)
        dE = (h - h[rows, w][:, None]) + (S - S[rows, w][:, None])
        dE[rows, w] = 0.0
        rejected(R.audit_scan(ref, dE), "scan: " + fault)
    good = R.mutation_ref(h, Jp, w.astype(np.int64))
    good[rows, w] = -0.0
    assert rejected(R.audit_scan(ref, good), "scan: -0.0 at the wild type")[0].identities


@pytest.mark.parametrize("name,fault", [("q25_L46_mf", "last_tile"), ("q25_L11_mf", "diagonal"), ("q25_L46_mf", "diagonal")])
def test_fault_in_the_energy_tiles(driver, name, fault):
    """the last tile of a tile group dropped; the diagonal tiles' pairs counted twice"""
    case = R.BY_NAME[name]
    plan = R.plan_of(case, driver)
    h, Jp = R.model_of(case, R.SIGMA_PLL)
    X = R.queries(case, 20)
    ref = R.energy_reference(h, Jp, X, plan["G"])
    R.assert_ok(R.audit_energies(ref, R.energy_by_tiles(h, Jp, X, plan)))
    bad = rejected(R.audit_energies(ref, R.energy_by_tiles(h, Jp, X, plan, fault=fault)), fault)
    assert len(bad[0].failing) == len(X)


def test_fault_mf_gap_row_not_zero(driver):
    case = R.BY_NAME["q9_L20_mf"]
    plan = R.plan_of(case, driver)
    h, Jp = R.model_of(case, R.SIGMA_PLL)
    assert np.all(Jp[:, -1, :] == 0) and np.all(Jp[:, :, -1] == 0) and np.all(h[:, -1] == 0) and np.any(Jp != 0)
    X = R.queries(case, 40)
    assert np.any(X == case.q - 1)
    J2 = Jp.copy()
    J2[:, -1, :] = J2[:, 0, :]                                     # the gap row reads the row of state 0
    rejected(R.audit_energies(R.energy_reference(h, Jp, X, plan["G"]), R._terms(h, J2, X)[0]), "mf gap row non-zero: energies")
    pll, site, cond, _ = R.conditionals_ref(h, J2, X)
    rejected(R.audit_conditionals(R.cond_reference(h, Jp, X), pll, site, cond), "mf gap row non-zero: conditionals")


def test_fault_in_the_draws(monkeypatch):
    """the Philox tag of the initial state used for a sweep; the draw with >= for >"""
    case = R.BY_NAME["q21_L19_f64"]
    h, Jp = R.model_of(case, R.SIGMA_SAMPLE)
    good = R.sample_reference(case, h, Jp)
    real = sampling.uniforms
    monkeypatch.setattr(sampling, "uniforms", lambda seed, chains, sweep, site, tag: real(seed, chains, sweep, site, 1 if tag == 0 else tag))
    bad = R.sample_reference(case, h, Jp, fault="tag")
    monkeypatch.undo()
    for g, b in zip(good, bad):
        rejected(R.audit_codes("chains", g[5], b[5]), "sweep draws from the tag of the initial state")
    # >= differs from > only where a cumulative sum equals r, which no Philox draw of the table does (the margin condition): a
    # draw made to tie shows only that the code audit sees differing codes; no case of the table can catch this rule
    p, r = np.array([[1.0, 1.0, 1.0]]), np.array([1.0])
    pick, _m = R.draw(p, r)
    cum = np.cumsum(p, axis=1)
    pick_ge = (cum >= r[:, None]).argmax(axis=1)
    assert pick.tolist() == [1] and pick_ge.tolist() == [0]
    rejected(R.audit_codes("draw", pick.astype(np.uint8), pick_ge.astype(np.uint8)), "draw with >= for >")


def test_fault_bm_counts_from_one_chain_more():
    case = R.BY_NAME["q21_L20_f32"]
    x = R.plm_x(case.name, R.SIGMA_SAMPLE)
    X = R.training_alignment(case, 60)
    _fi, _fij, want = R.bm_reference(case, x, X)
    _fi, _fij, more = R.bm_reference(case, x, X, extra_chain=True)
    S, xx, gi, gij, rec = more[0]
    n = case.chains
    gi2, gij2 = R.model_stats(S, case.q)                           # n + 1 chains counted, divided by n + 1 ...
    got = (S[:n], xx, gi2, gij2, rec)
    assert np.array_equal(S[:n], want[0][0])                       # the first n chains are the same chains
    bad = rejected(R.audit_bm("bm iteration 0", want[0], got), "bm counts from n + 1 chains")
    assert any("g differs" in s for s in bad[0].identities)
    R.assert_ok(R.audit_bm("bm iteration 0", want[0], want[0]))
