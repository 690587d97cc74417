"""Every element of the arDCA epistasis (dca_ar_epistasis: eps and d) and the scores made of it (dca_ar_epistatic_scores) at the
edges of the product kernel's geometry and at every QM instantiation, against the longdouble reference of
tests/ar_epistasis_reference.py within the bounds derived there from the rounding sequence of pydca_amd/csrc/ar_epistasis.hip
and scoring.hip.  One context and one reference per case; the case table names the edge each shape reaches and
tests/test_ar_epistasis_audit_host.py holds the table to ar_epistasis_plan.h, the bounds to positive and negative controls."""
import numpy as np
import pytest

import ar_epistasis_reference as R

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("epiplan"))


def worst(dev, ref, bound):
    """the largest |dev - ref| / bound; an element with a bound of 0 has to be equal"""
    return float(R.ratios_of(np.asarray(dev, dtype=np.float64), ref, bound).max())


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_every_element_within_its_bound(L_, driver, case):
    L, q, Lq = case.L, case.q, case.L * case.q
    ref = R.reference(case, R.plan_of(case, driver))
    ctx = L_.Context(0, L_.DCA_F64)
    try:
        # any alignment serves: the entries under test read the model alone
        ctx.set_msa(np.random.default_rng(1).integers(0, q, size=(8, L)).astype(np.uint8), q)
        ctx.set_weights(np.ones(8))
        ctx.ar_configure(0.01, 0.01)
        ctx.ar_set_x(ref.x)

        # ---- eps and d, every element
        eps, d = ctx.ar_epistasis(ref.w)
        a = R.assert_within_bounds(ref, eps, d)
        assert np.all(eps[ref.zero] == 0.0) and np.all(d[ref.d_zero] == 0.0)
        assert np.all(np.isfinite(eps)) and np.all(np.isfinite(d))
        e2, d2 = ctx.ar_epistasis(ref.w)
        e3, none = ctx.ar_epistasis(ref.w, single=False)
        none2, d3 = ctx.ar_epistasis(ref.w, eps=False)
        assert none is None and none2 is None
        assert np.array_equal(e2, eps) and np.array_equal(e3, eps) and np.array_equal(d2, d) and np.array_equal(d3, d)
        if case.planted:
            e = (R.pair_index(L, 0, 1), 1, 1)
            print("%s: planted element device %.17g, reference %.17g, bound %.3e" % (case.name, eps[e], float(ref.eps[e]), ref.eps_bound[e]))
            assert np.isfinite(eps[e]) and abs(float(LD(eps[e]) - ref.eps[e])) <= ref.eps_bound[e] and eps[e] > 1100 * np.log(2)

        # ---- d by the route of ArDCA.compute_single_mutant_effects: log P of the L q + 1 single mutants
        X = R.single_mutants(ref.w, L, q)
        lp = ctx.ar_log_probabilities(X)
        lp_ref, lp_bound = R.logp_reference(ref.x, L, q, X)
        r_lp = worst(lp, lp_ref, lp_bound)
        route = (lp[:Lq] - lp[Lq]).reshape(L, q)
        route_bound = ((lp_bound[:Lq] + lp_bound[Lq]).reshape(L, q) + R.U * np.abs(ref.d).astype(np.float64)) * R.UP
        r_route = worst(route, ref.d, route_bound)
        r_both = float((np.abs(d - route) / (ref.d_bound + route_bound)).max())
        assert np.all(route[ref.d_zero] == 0.0)                    # the wild type against itself

        # ---- the scores: fn_kernel on the plm-layout float64 table, from the device's own eps (i) and from the reference's (ii)
        r_scores = {}
        for apc in (False, True):
            s = ctx.ar_epistatic_scores(ref.w, apc=apc)
            order = ctx.scores_order()
            with np.errstate(invalid="ignore"):
                assert np.array_equal(order, np.argsort(-s, kind="stable"))
            for src, extra, tag in ((eps, None, "i"), (ref.eps, ref.eps_bound, "ii")):
                sr, sb = R.fn_reference(src, q, extra)
                if apc:
                    sr, sb = R.apc_reference(sr, sb, L)
                r_scores[(apc, tag)] = float(R.score_ratios(s, sr, sb).max())
            assert np.array_equal(ctx.ar_epistatic_scores(ref.w, apc=apc), s, equal_nan=True)
        print("%s ratios: eps %.4f  d %.4f  log P %.4f  d by log P %.4f  d against it %.4f  FN (i) %.4f (ii) %.4f  APC (i) %.4f (ii) %.4f" % (
            case.name, a.worst, a.worst_d, r_lp, r_route, r_both, r_scores[(False, "i")], r_scores[(False, "ii")],
            r_scores[(True, "i")], r_scores[(True, "ii")]))
        assert r_lp <= 1.0 and r_route <= 1.0 and r_both <= 1.0
        assert all(r <= 1.0 for r in r_scores.values()), r_scores
        assert np.array_equal(ctx.ar_get_x(), ref.x)
    finally:
        ctx.close()
