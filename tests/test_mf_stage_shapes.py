"""The mfDCA stage kernels (pydca_amd/csrc/mf_engine.hip, the FN / APC kernels of scoring.hip) element by element at the shapes
where they change path: buckets around the 32-entry batch of the counts kernel, a second block of 256 sites, sort segments
longer than one sequence, q = 2 / 8 / 9 / 32, n = L (q-1) beyond 256.  The cases, their constructed alignments and the exact
count reference are in tests/mf_shape_cases.py; everything after the counts is oracle/mf.py on those exact frequencies, so no
reference value ever comes from the device.  Every check prints the figure it asserts (pytest -s shows the margins).

Run on an MI355X:  python -m pytest tests/test_mf_stage_shapes.py -q -m gpu"""
import numpy as np
import pytest

import mf_shape_cases as M
from conftest import assert_scores_within, rel_err

pytestmark = pytest.mark.gpu

U = M.U
# Correlation matrix: every intermediate (frequencies, regularised frequencies, their products) lies in [0, 1]; the kernel and
# construct_corr_mat each perform about ten roundings of at most half an ulp of 1 (2^-53) on the way to an entry.
CORR_ATOL = 32 * U


@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


def dyadic_ctx(L_, case):
    X, k = M.alignment(case.name)
    ctx = L_.Context(0, L_.DCA_F64)
    ctx.set_msa(X, case.q)
    ctx.set_weights(k / 8.0)
    return ctx


def report(case, what, value, bound):
    print("\n[mf-shapes] %-28s %-34s %.3e (bound %.3e)" % (case, what, value, bound))
    return value


# ----------------------------------------------------------------------------- dyadic weights: counts are exact
@pytest.mark.parametrize("case", M.DYADIC, ids=repr)
def test_frequencies_equal_the_exact_counts(L_, case):
    """Every weighted count is an exact sum and the kernel divides once by Meff, as the reference does: equal bits."""
    ref = M.dyadic_reference(case.name)
    ctx = dyadic_ctx(L_, case)
    fi, fij = ctx.mf_single_site_freqs(), ctx.mf_pair_site_freqs()
    ctx.close()
    report(case, "fi: elements that differ", float(np.sum(fi != ref.fi)), 0)
    report(case, "fij: elements that differ", float(np.sum(fij != ref.fij)), 0)
    np.testing.assert_array_equal(fi, ref.fi)
    np.testing.assert_array_equal(fij, ref.fij)


@pytest.mark.parametrize("name", ["N257_L9_q5", "N300_L258_q5"])
def test_gap_state_counts_through_the_boltzmann_statistics(L_, name):
    """The gap rows and columns of the raw counts are visible in the data statistics of a Boltzmann-learning run,
    (1 - lam) f + lam / q and (1 - lam) f + lam / q^2.  The reference applies the same three operations to the exact
    frequencies; 2 ulp are allowed per element."""
    case, lam = M.BY_NAME[name], 0.03
    ref = M.dyadic_reference(name)
    ctx = dyadic_ctx(L_, case)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_bm_begin(8, 1, 0, pseudocount=lam)
    fi, fij = ctx.plm_bm_freqs(0)
    ctx.close()
    rfi, rfij = ref.bm_freqs(lam)
    ui = report(case, "bm fi: ulps", float(M.ulps(fi, rfi).max()), 2)
    uij = report(case, "bm fij (gap included): ulps", float(M.ulps(fij, rfij).max()), 2)
    assert ui <= 2 and uij <= 2


@pytest.mark.parametrize("case", M.DYADIC, ids=repr)
def test_correlation_matrix(L_, case):
    ref = M.dyadic_reference(case.name)
    ctx = dyadic_ctx(L_, case)
    C = ctx.mf_corr_mat(M.THETA)
    assert np.array_equal(C, C.T), "the correlation matrix is not bit-symmetric"
    err = report(case, "corr_mat: max abs error", float(np.abs(C - ref.corr).max()), CORR_ATOL)
    assert err <= CORR_ATOL
    del C
    C2 = ctx.mf_corr_from_freqs(ref.reg_fi, ref.reg_fij, case.L, case.q)
    ctx.close()
    err = report(case, "corr_from_freqs: max abs error", float(np.abs(C2 - ref.corr).max()), CORR_ATOL)
    assert err <= CORR_ATOL


# ----------------------------------------------------------------------------- inverse, fields, scores
def check_model_and_scores(ctx, case, ref):
    """Couplings against -inv(C_ref) (LAPACK) at the project's bound for the inverse, fields at the bound of the toy fields
    test, FN / APC scores at 1e-9 and the device ranking against a stable descending argsort of the device scores."""
    ctx.mf_corr_mat(M.THETA, want=False)
    J = ctx.mf_couplings()
    err = report(case, "couplings: rel_err", rel_err(J, ref.couplings), 1e-9)
    assert err <= 1e-9
    err = report(case, "fields: rel_err", rel_err(ctx.mf_fields(), ref.fields), 1e-8)
    assert err <= 1e-8
    for apc in (False, True):
        scores = ctx.mf_run(M.THETA, apc)
        order = ctx.scores_order()
        s_ref = ref.scores(apc)
        if np.all(np.isfinite(s_ref)):
            worst = assert_scores_within(scores, s_ref, ref.fn, rtol=1e-9)
            report(case, "scores apc=%d: worst ratio" % apc, worst, 1e-9)
        else:
            # q = 2: 1 x 1 blocks, every FN is exactly 0 and the correction is 0 / 0 on both sides
            assert not np.any(ref.fn) and np.array_equal(np.isnan(scores), np.isnan(s_ref)) and np.all(np.isnan(scores))
        np.testing.assert_array_equal(order, np.argsort(-scores, kind="stable"))


@pytest.mark.parametrize("case", [c for c in M.DYADIC if c.inverse], ids=repr)
def test_couplings_fields_and_scores(L_, case):
    ref = M.dyadic_reference(case.name)
    ctx = dyadic_ctx(L_, case)
    check_model_and_scores(ctx, case, ref)
    ctx.close()


def test_energies_under_the_reference_model(L_):
    """mf_energies against energies of the REFERENCE couplings and fields (the other energy tests build their model from the
    device's own mf_couplings / mf_fields): 1e-8 relative to the largest |E|."""
    case = M.BY_NAME["N300_L258_q5"]
    ref = M.dyadic_reference(case.name)
    ctx = dyadic_ctx(L_, case)
    ctx.mf_corr_mat(M.THETA, want=False)
    ctx.mf_couplings(want=False)
    Q = np.random.default_rng(258).integers(0, case.q, (100, case.L), dtype=np.uint8)
    E = ctx.mf_energies(Q)
    ctx.close()
    E_ref, _ = ref.energies(Q)
    scale = float(np.abs(E_ref).max())
    err = report(case, "energies: max error / max |E|", float(np.abs(E - E_ref).max()) / scale, 1e-8)
    assert E.shape == (100,) and err <= 1e-8


# ----------------------------------------------------------------------------- general weights
@pytest.mark.parametrize("case", M.GENERAL, ids=repr)
def test_general_weights(L_, case):
    """1 / count weights: the sums round.  A k-term sum of positive numbers is off by at most (k-1) u relative; a bucket has at
    most N terms, a dominant-state row is the column total f_j(b) minus the q - 1 other rows (q more terms, each at most the
    column total), and the division, Meff and the final rounding take the remaining 4: |f - f_ref| <= (N + q + 4) u f_j(b),
    for f_i itself with f_j(b) = f_i.  The correlation matrix gets its own bound plus this one with the column total at its
    maximum 1."""
    X, _ = M.alignment(case.name)
    N, L, q = case.N, case.L, case.q
    ctx = L_.Context(0, L_.DCA_F64)
    ctx.set_msa(X, q)
    w = ctx.compute_weights(0.8, L_.DCA_F64)
    assert not np.all(w == 1.0)
    ref = M.Reference(X, q, *M.fsum_freqs(X, q, w))
    fi, fij = ctx.mf_single_site_freqs(), ctx.mf_pair_site_freqs()
    bound = (N + q + 4) * U
    with np.errstate(divide="ignore", invalid="ignore"):
        ri = np.where(ref.fi > 0, np.abs(fi - ref.fi) / ref.fi, np.where(fi == 0, 0.0, np.inf))
        col = ref.fi[np.triu_indices(L, 1)[1]][:, None, :q - 1]          # f_j(b) of pair (i, j), broadcast over a
        rij = np.where(col > 0, np.abs(fij - ref.fij) / col, np.where(fij == 0, 0.0, np.inf))
    ei = report(case, "fi: error / f_i", float(ri.max()), bound)
    eij = report(case, "fij: error / f_j(b)", float(rij.max()), bound)
    assert ei <= bound and eij <= bound
    C = ctx.mf_corr_mat(M.THETA)
    assert np.array_equal(C, C.T)
    err = report(case, "corr_mat: max abs error", float(np.abs(C - ref.corr).max()), CORR_ATOL + bound)
    assert err <= CORR_ATOL + bound
    check_model_and_scores(ctx, case, ref)
    ctx.close()
