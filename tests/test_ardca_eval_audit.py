"""Every element of the arDCA objective and gradient at the edges of the kernels' geometry, against the longdouble reference of
tests/ardca_eval_reference.py within the bound derived there from the rounding sequence of pydca_amd/csrc/ardca.hip and
site_conditionals.h.  One context, one reference and one evaluation per case (plus its repeat and the single evaluation of a
fit of no iterations, which gives the optimiser's |g|); the case table names the edge each shape reaches and
tests/test_ardca_eval_audit_host.py holds the table to ar_plan.h, the bound to positive and negative controls."""
import numpy as np
import pytest

import ardca_eval_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("arplan"))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_every_element_within_its_bound(L_, driver, monkeypatch, case):
    ref = R.reference(case, R.plan_of(case, driver))
    monkeypatch.delenv("DCA_AR_PASS", raising=False)
    if case.pass_size:
        monkeypatch.setenv("DCA_AR_PASS", str(case.pass_size))          # ar_configure reads it
    ctx = L_.Context(0, L_.DCA_F64)
    try:
        ctx.set_msa(ref.X, case.q)
        ctx.set_weights(ref.w)
        ctx.ar_configure(R.LAMBDA_H, R.LAMBDA_J)
        ctx.ar_set_x(ref.x)
        fx = ctx.ar_gradient()
        g = ctx.ar_get_g()
        a = R.audit(ref, fx, g)
        assert R.assert_within_bounds(ref, fx, g) == case.P
        assert ctx.ar_gradient() == fx and np.array_equal(ctx.ar_get_g(), g)          # a second evaluation: the same bits
        # a fit of no iterations returns after its single evaluation: the same fx, and the |g| of the dot kernels
        st = ctx.ar_fit(0, 1e-300)
        assert st["iterations"] == 0 and st["evaluations"] == 1
        assert st["fx"] == fx and np.array_equal(ctx.ar_get_g(), g)
        gn = R.gnorm_ratio(g, st["gnorm"])
        print("%s ratios: g %.4f  fx %.4f  |g|^2 %.4f  (dot rows per thread %d)" % (case.name, a.worst, a.fx_ratio, gn, ref.plan["dotRows"]))
        assert gn <= 1.0
    finally:
        ctx.close()
