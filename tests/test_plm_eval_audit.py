"""Every element of the plmDCA objective and gradient, per launch path, against the longdouble reference of
tests/plm_eval_reference.py within the bound derived there from the kernels' rounding sequence (pydca_amd/csrc/plm_stages.h).
One context, one evaluation and one reference per case; the case table names the path each shape reaches and
tests/test_plm_eval_audit_host.py holds the table to the launch planner, the bound to positive and negative controls.
The float64 cases also keep what test_gradient_float64_vs_oracle asserts against the float64 oracle."""
import numpy as np
import pytest

import plm_eval_reference as R
from conftest import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return R.compile_plan_driver(tmp_path_factory.mktemp("plan"))


def evaluate(L_, case, ref, monkeypatch):
    for k in R.KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():              # the engine reads them once per configure
        monkeypatch.setenv(k, v)
    ctx = L_.Context(0, L_.DCA_F32 if case.bits == 32 else L_.DCA_F64)
    try:
        ctx.set_msa(ref.X, case.q)
        ctx.set_weights(ref.w)
        ctx.plm_configure(R.LAMBDA_H, R.LAMBDA_J, R.CARRY[case.mode], case.chunk, 0, halo=case.halo)
        ctx.plm_set_x(ref.x)
        fx = ctx.plm_gradient()
        return fx, ctx.plm_get_g(case.dtype.type)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_every_element_within_its_bound(L_, driver, oracle_plm, monkeypatch, case):
    ref = R.reference(case, R.plan_of(case, driver))
    fx, g = evaluate(L_, case, ref, monkeypatch)
    a = R.assert_within_bounds(ref, fx, g)
    assert a.checked == case.P
    if case.bits == 64:
        # the float64 mode against the float64 oracle, as test_gradient_float64_vs_oracle holds it: the objective equal or one
        # unit in the last place off, the gradient to a few 1e-16 of its norm and most elements equal
        fx_o, g_o = oracle_plm.gradient(ref.X, ref.w, case.q, R.LAMBDA_H, R.LAMBDA_J, ref.x, carry=case.mode != "exact")
        print("%s: fx %.17g oracle %.17g, rel_err(g, oracle) %.3e, %.3f of the elements differ" % (case.name, fx, fx_o, rel_err(g, g_o), float(np.mean(g != g_o))))
        assert abs(fx - fx_o) <= 4e-16 * abs(fx_o)
        assert rel_err(g, g_o) < 5e-15
        assert np.mean(g != g_o) < 0.3
