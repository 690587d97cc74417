"""Ownership of device memory, seen through dca_device_blocks_in_use(): the number of blocks the library has allocated and
not yet released, over the whole process.

(a) every entry called twice leaves as many blocks in use after the second call as after the first (the first may create
    buffers that an engine keeps); (b) closing the context brings the count back to what it was before the context existed;
(c) a call that fails its argument or state checks -- some of them after they have allocated -- leaves the count as it was
and returns the code it always returned.

Shapes: N = 48 with L = 6, q = 5 and L = 5, q = 21, random codes with a few duplicated rows: the smallest at which every
entry still takes its normal path (both alphabets' kernels, more than one site pair and triple).  DCA_NN_PASS = 16 makes the
pass loops of dca_hamming_nearest and dca_three_site_values run three times over 40 rows."""
import ctypes as C

import numpy as np
import pytest

from pydca_amd import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(48, 6, 5, _lib.DCA_F32), (48, 5, 21, _lib.DCA_F64)]


def in_use():
    return _lib.device_blocks_in_use()


def alignment(N, L, q, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, q, size=(N, L), dtype=np.uint8)
    X[5] = X[2]
    X[17] = X[2]
    X[40] = X[39]
    Q = np.ascontiguousarray(rng.integers(0, q, size=(40, L), dtype=np.uint8))
    Q[7] = X[3]
    return np.ascontiguousarray(X), Q, rng


def twice(name, fn):
    fn()
    first = in_use()
    fn()
    assert in_use() == first, "%s: %d blocks in use after the first call, %d after the second" % (name, first, in_use())


def elements(L, q, rng):
    el = [(0, 1, 2, 0, 1, 2), (0, 1, 2, 1, 1, 0), (1, 2, L - 1, q - 1, 0, 3), (0, 1, 2, 0, 1, 2)]
    return np.array(el, dtype=np.int32)


@pytest.mark.parametrize("N,L,q,precision", SHAPES)
def test_every_entry_balances_and_the_context_gives_everything_back(N, L, q, precision):
    X, Q, rng = alignment(N, L, q, 11 * L + q)
    npairs = L * (L - 1) // 2
    before = in_use()
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    twice("weights", lambda: ctx.compute_weights(0.8))

    # mean field
    twice("mf_single_site_freqs", ctx.mf_single_site_freqs)
    twice("mf_pair_site_freqs", ctx.mf_pair_site_freqs)
    twice("mf_corr_mat", lambda: ctx.mf_corr_mat(0.5))
    twice("mf_couplings", ctx.mf_couplings)
    twice("mf_scores", ctx.mf_scores)
    twice("scores_order", ctx.scores_order)
    twice("mf_di_scores", lambda: ctx.mf_di_scores(True))
    twice("mf_fields", ctx.mf_fields)
    twice("mf_pair_couplings", lambda: ctx.mf_pair_couplings([[0, 1], [1, L - 1]]))
    twice("mf_run", lambda: ctx.mf_run(0.5, True, want_couplings=True))
    twice("mf_energies", lambda: ctx.mf_energies(Q))
    twice("mf_mutation_scan", lambda: ctx.mf_mutation_scan(X[0]))
    twice("mf_pseudo_likelihood", lambda: ctx.mf_pseudo_likelihood(Q, per_site=True, conditionals=True))
    twice("mf_sample", lambda: ctx.mf_sample(9, 2, seed=3))
    twice("mf_ais", lambda: ctx.mf_ais(8, 3, 1, seed=5, return_chains=True))
    J = ctx.mf_couplings()
    reg_fi = 0.5 / q + 0.5 * ctx.mf_single_site_freqs()
    twice("di_from_arrays", lambda: ctx.di_from_arrays(J, 1, reg_fi, L, q, want_fields=True))
    fi = ctx.mf_single_site_freqs()
    fij = ctx.mf_pair_site_freqs()
    twice("mf_corr_from_freqs", lambda: ctx.mf_corr_from_freqs(fi, fij, L, q))
    B = rng.standard_normal((70, 78))
    A = B @ B.T / 70 + 0.5 * np.eye(70)
    twice("spd_inverse", lambda: ctx.spd_inverse(A))

    # pseudo-likelihood model
    twice("plm_configure", lambda: ctx.plm_configure(1.0, 2.0))
    ctx.plm_init_x()
    ctx.plm_set_x((0.05 * rng.standard_normal(ctx.num_params())).astype(np.float32 if precision == _lib.DCA_F32 else np.float64))
    twice("plm_gradient", ctx.plm_gradient)
    twice("plm_scores", ctx.plm_scores)
    twice("plm_di_scores", lambda: ctx.plm_di_scores(reg_fi, True))
    twice("plm_pair_couplings", lambda: ctx.plm_pair_couplings([[0, 2], [1, L - 1]]))
    twice("plm_energies", lambda: ctx.plm_energies(Q))
    twice("plm_mutation_scan", lambda: ctx.plm_mutation_scan(X[1]))
    twice("plm_pseudo_likelihood", lambda: ctx.plm_pseudo_likelihood(Q, per_site=True, conditionals=True))
    twice("plm_sample", lambda: ctx.plm_sample(9, 2, seed=3, initial=Q[:9]))
    twice("plm_sample from random starts", lambda: ctx.plm_sample(70, 1, seed=4))
    twice("plm_ais", lambda: ctx.plm_ais(8, 3, 1, seed=5, return_chains=True))
    twice("plm_bm_begin", lambda: ctx.plm_bm_begin(8, 1, 1, seed=2, eta_h=0.01, eta_J=0.01, pseudocount=0.1))
    twice("plm_bm_iterate", lambda: ctx.plm_bm_iterate(2))
    twice("plm_bm_freqs", lambda: ctx.plm_bm_freqs(1))
    twice("plm_bm_chains", ctx.plm_bm_chains)
    twice("plm_bm_end", ctx.plm_bm_end)
    twice("plm_release", ctx.plm_release)

    # autoregressive model
    twice("ar_configure", lambda: ctx.ar_configure(0.01, 0.01))
    twice("ar_fit", lambda: ctx.ar_fit(max_iterations=2))
    twice("ar_log_probabilities", lambda: ctx.ar_log_probabilities(Q, per_site=True, conditionals=True))
    twice("ar_sample", lambda: ctx.ar_sample(9, seed=1))
    twice("ar_epistasis", lambda: ctx.ar_epistasis(X[0]))
    twice("ar_epistatic_scores", lambda: ctx.ar_epistatic_scores(X[0]))
    twice("ar_release", ctx.ar_release)

    # sequence sets against the alignment
    twice("hamming_nearest", lambda: ctx.hamming_nearest(Q))
    twice("hamming_nearest of the alignment", lambda: ctx.hamming_nearest(skip_same_index=True))
    twice("sequence_statistics", lambda: ctx.sequence_statistics(Q))
    twice("alignment_statistics", ctx.alignment_statistics)
    el = elements(L, q, rng)
    twice("three_site_values", lambda: ctx.three_site_values(el))
    twice("three_site_values of a set", lambda: ctx.three_site_values(el, Q))
    twice("three_site_scan", lambda: ctx.three_site_scan(5))
    twice("three_site_scan of a set", lambda: ctx.three_site_scan(5, Q))
    assert npairs == ctx.mf_scores().size

    ctx.close()
    assert in_use() == before, "%d blocks in use before the context, %d after it was closed" % (before, in_use())


def test_pass_loops_balance(monkeypatch):
    """40 query rows in passes of 16: the row buffers of a pass are reused, not allocated per pass, and go back once."""
    N, L, q, precision = SHAPES[0]
    X, Q, rng = alignment(N, L, q, 3)
    monkeypatch.setenv("DCA_NN_PASS", "16")
    before = in_use()
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8)
    el = elements(L, q, rng)
    whole = in_use()
    dist, index, hist = ctx.hamming_nearest(Q)
    assert dist[7] == 0 and int(hist.sum()) == 40 * N            # every pass was counted
    assert in_use() == whole
    count, denom, _f3, _c3 = ctx.three_site_values(el, Q)
    assert denom == 40 and count[0] == int(((Q[:, 0] == 0) & (Q[:, 1] == 1) & (Q[:, 2] == 2)).sum())
    assert in_use() == whole
    ctx.close()
    assert in_use() == before


def test_failing_calls_release_what_they_allocated(monkeypatch):
    N, L, q, precision = SHAPES[0]
    X, Q, rng = alignment(N, L, q, 5)
    bad = Q.copy()
    bad[33, L - 1] = q
    lib = _lib.lib()
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8)
    ctx.mf_run(0.5, True)
    ctx.mf_fields()                                   # (the engine keeps its regularised frequencies from here on)
    ctx.plm_configure(1.0, 2.0)
    ctx.plm_init_x()
    el = elements(L, q, rng)
    out_of_range = el.copy()
    out_of_range[2, 2] = L
    c3 = np.zeros(len(el))
    rec = np.zeros((1, 3))
    eps = np.zeros((L * (L - 1) // 2, q, q))
    wt = np.ascontiguousarray(X[0])
    indefinite = np.eye(70)
    indefinite[7, 7] = -1.0

    def code(fn):
        try:
            rc = fn()
        except _lib.DcaBackendError as e:
            return e.code
        return rc if isinstance(rc, int) else _lib.DCA_OK

    calls = [
        ("weights: unknown compare precision", lambda: ctx.compute_weights(0.8, 7), _lib.DCA_ERR_ARG),
        ("mf_pair_couplings: pair out of order", lambda: ctx.mf_pair_couplings([[0, 1], [3, 1]]), _lib.DCA_ERR_ARG),
        ("spd_inverse: indefinite matrix", lambda: ctx.spd_inverse(indefinite), _lib.DCA_ERR_NOT_SPD),
        ("di_from_arrays: q > 21", lambda: ctx.di_from_arrays(np.zeros((4, 4)), 1, np.ones((2, 23)), 2, 23), _lib.DCA_ERR_ARG),
        ("plm_pair_couplings: site out of range", lambda: ctx.plm_pair_couplings([[0, L]]), _lib.DCA_ERR_ARG),
        ("plm_energies: code >= q", lambda: ctx.plm_energies(bad), _lib.DCA_ERR_ARG),
        ("mf_energies: code >= q", lambda: ctx.mf_energies(bad), _lib.DCA_ERR_ARG),
        ("plm_mutation_scan: code >= q", lambda: ctx.plm_mutation_scan(bad[33]), _lib.DCA_ERR_ARG),
        ("plm_pseudo_likelihood: code >= q", lambda: ctx.plm_pseudo_likelihood(bad, conditionals=True), _lib.DCA_ERR_ARG),
        ("plm_sample: initial code >= q", lambda: ctx.plm_sample(40, 1, initial=bad), _lib.DCA_ERR_ARG),
        ("plm_ais: no chains", lambda: ctx.plm_ais(0, 3), _lib.DCA_ERR_ARG),
        ("plm_bm_begin: no chains", lambda: ctx.plm_bm_begin(0, 1, 1), _lib.DCA_ERR_ARG),
        ("plm_bm_begin: initial code >= q", lambda: ctx.plm_bm_begin(40, 1, 1, initial=bad), _lib.DCA_ERR_ARG),
        ("dca_plm_bm_iterate without a run", lambda: lib.dca_plm_bm_iterate(ctx._h, 1, rec.ctypes.data), _lib.DCA_ERR_STATE),
        ("dca_ar_epistasis before dca_ar_configure", lambda: lib.dca_ar_epistasis(ctx._h, wt.ctypes.data, eps.ctypes.data, None),
         _lib.DCA_ERR_STATE),
        ("ar_sample before ar_configure", lambda: ctx.ar_sample(4), _lib.DCA_ERR_STATE),
        ("hamming_nearest: code >= q", lambda: ctx.hamming_nearest(bad), _lib.DCA_ERR_ARG),
        ("sequence_statistics: code >= q", lambda: ctx.sequence_statistics(bad), _lib.DCA_ERR_ARG),
        ("three_site_values: code >= q", lambda: ctx.three_site_values(el, bad), _lib.DCA_ERR_ARG),
        ("three_site_scan: code >= q", lambda: ctx.three_site_scan(5, bad), _lib.DCA_ERR_ARG),
        ("dca_three_site_values: site out of range",
         lambda: lib.dca_three_site_values(ctx._h, None, 0, out_of_range.ctypes.data, len(el), None, None, None, c3.ctypes.data),
         _lib.DCA_ERR_ARG),
    ]
    for name, fn, expected in calls:
        held = in_use()
        assert code(fn) == expected, name
        assert in_use() == held, "%s: %d blocks in use before, %d after" % (name, held, in_use())
    # refused after its buffers exist: more elements tie with the K-th than the candidate list may hold
    monkeypatch.setenv("DCA_THREE_SITE_CAP", "1")
    held = in_use()
    assert code(lambda: ctx.three_site_scan(5)) == _lib.DCA_ERR_ARG and b"tie with the K-th largest" in lib.dca_last_error()
    assert in_use() == held
    ctx.close()
