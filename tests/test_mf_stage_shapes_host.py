"""CPU pins of tests/mf_shape_cases.py, the exact count reference and case builder that tests/test_mf_stage_shapes.py measures
the mfDCA stage kernels against: it reproduces the toy goldens of the real reference, equals oracle/mf.py bit for bit on
dyadic weights, and its constructed alignments hold the edges they exist for."""
import numpy as np
import pytest

import mf_shape_cases as M
from conftest import golden

SHAPES = [(c.N, c.L, c.q) for c in M.DYADIC if c.n <= 1100] + [(2100, 40, 5), (257, 257, 21)]


@pytest.mark.parametrize("tag", ["toy_rna", "toy_protein", "toy_rna_theta02_seqid1"])
def test_count_references_reproduce_the_toy_goldens(tag):
    """Same tolerances as test_mf_stages_vs_reference (tests/test_gpu_parity.py)."""
    G = golden("mf_" + tag)
    X, q, w = (G["X"] - 1).astype(np.uint8), int(G["q"]), G["w"]
    fi, fij = M.fsum_freqs(X, q, w)
    np.testing.assert_allclose(fi, G["fi"], rtol=1e-13, atol=1e-16)
    np.testing.assert_allclose(fij[:, :q - 1, :q - 1], G["fij"], rtol=1e-12, atol=1e-15)
    if np.all(w == 1.0):                        # weights 8 / 8: the integer path applies as well
        fi, fij = M.exact_freqs(X, q, np.full(X.shape[0], 8))
        np.testing.assert_allclose(fi, G["fi"], rtol=1e-13, atol=1e-16)
        np.testing.assert_allclose(fij[:, :q - 1, :q - 1], G["fij"], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("N,L,q", SHAPES)
def test_exact_counts_equal_the_oracle_bit_for_bit(oracle_mf, N, L, q):
    """Dyadic weights: the oracle's float64 sums are exact too, so integer counts divided once by the integer Meff and the
    oracle's frequencies are the same bits; so are the fsum reference's.  The gap rows and columns, which the oracle does not
    form, are pinned by their marginals: sum_b f_ij(a, b) = f_i(a) exactly, in integers."""
    rng = np.random.default_rng([N, L, q])
    X = rng.integers(0, q, (N, L), dtype=np.uint8)
    k = rng.integers(1, 9, N)
    fi, fij = M.exact_freqs(X, q, k)
    np.testing.assert_array_equal(fi, oracle_mf.compute_single_site_freqs(X.astype(np.int64) + 1, q, k / 8.0))
    np.testing.assert_array_equal(fij[:, :q - 1, :q - 1], oracle_mf.compute_pair_site_freqs(X.astype(np.int64) + 1, q, k / 8.0))
    single, pair, meff = M.exact_counts(X, q, k)
    iu, ju = np.triu_indices(L, 1)
    assert meff == k.sum() and np.all(single.sum(1) == meff)
    np.testing.assert_array_equal(pair.sum(2), single[iu])
    np.testing.assert_array_equal(pair.sum(1), single[ju])
    if N * L * L <= 2_000_000:
        gi, gij = M.fsum_freqs(X, q, k / 8.0)
        np.testing.assert_array_equal(gi, fi)
        np.testing.assert_array_equal(gij, fij)


def test_exact_counts_on_a_hand_counted_alignment():
    X = np.array([[0, 1, 2], [0, 2, 2], [1, 1, 0]], dtype=np.uint8)
    single, pair, meff = M.exact_counts(X, 3, np.array([8, 4, 1]))
    assert meff == 13
    assert single.tolist() == [[12, 1, 0], [0, 9, 4], [1, 0, 12]]
    assert pair[0].tolist() == [[0, 8, 4], [0, 1, 0], [0, 0, 0]]      # sites (0, 1)
    assert pair[1].tolist() == [[0, 0, 12], [1, 0, 0], [0, 0, 0]]     # sites (0, 2)
    assert pair[2].tolist() == [[0, 0, 0], [1, 0, 8], [0, 0, 4]]      # sites (1, 2)


@pytest.mark.parametrize("case", M.CASES, ids=repr)
def test_constructed_alignments_hold_their_edges(case):
    """alignment() asserts the planted edges itself (check_planted); here additionally what each case is for."""
    X, k = M.alignment(case.name)
    assert X.shape == (case.N, case.L) and X.dtype == np.uint8 and int(X.max()) < case.q
    assert not X.flags.writeable
    if case.weights == "dyadic":
        assert k.shape == (case.N,) and 1 <= k.min() and k.max() <= 8
    if case.planted:
        M.check_planted(X, case.q)
    if case.N == 1:
        assert M.nondominant_bucket_lengths(X, case.q) == {0}
    if case.weights == "general":               # near-duplicates at 80 % identity exist, so 1 / count weights are not all 1
        ident = (X[:40, None, :] == X[None, :, :]).mean(2)
        assert (ident > 0.8).sum(1).max() > 1


@pytest.mark.parametrize("q", [5, 21])
def test_check_planted_notices_a_dropped_edge(q):
    X = np.array(M.alignment({5: "N257_L9_q5", 21: "N513_L9_q21"}[q])[0])
    X[:, [2, 5, 7, 8]] = (np.arange(X.shape[0]) % 2)[:, None]      # the random columns: no edge may be present by chance
    M.check_planted(X, q)
    lost = X.copy()
    c = np.bincount(lost[:, 1], minlength=q)    # the column with the buckets 33, 63, 64: 33 joins the dominant one
    lost[lost[:, 1] == list(c).index(33), 1] = np.argmax(c)
    with pytest.raises(AssertionError, match="bucket lengths"):
        M.check_planted(lost, q)
    lost = X.copy()
    lost[0, 6] = (lost[0, 6] + 1) % q           # the constant column
    with pytest.raises(AssertionError, match="constant"):
        M.check_planted(lost, q)


@pytest.mark.parametrize("case", [c for c in M.DYADIC if c.inverse], ids=repr)
def test_reference_correlation_matrix_is_positive_definite(case):
    """The couplings are checked against -inv of this matrix: it has to be invertible on the reference side."""
    ref = M.dyadic_reference(case.name)
    np.linalg.cholesky(ref.corr)
    assert np.array_equal(ref.corr, ref.corr.T)
