"""The autoregressive model on the GPU (dca_ar_*, ArDCA and the ardca command line), checked against the float64 numpy
restatement of tests/test_ardca_host.py, scipy's L-BFGS-B, exact enumeration and itself (bitwise invariance)."""
import itertools
import os

import numpy as np
import pytest

from conftest import data_file
from test_ardca_host import log_probabilities_ref, conditionals_ref, objective_ref, random_alignment, random_model, sample_ref
from test_pseudo_likelihood_host import mf_model
from pydca_amd import _lib, _potts, ardca_main
from pydca_amd.ardca.ardca import ArDCA

pytestmark = pytest.mark.gpu


def ar_context(X, q, w=None, lambda_h=0.01, lambda_J=0.02):
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    if w is None:
        ctx.compute_weights(0.8, _lib.DCA_F64)
    else:
        ctx.set_weights(w)
    ctx.ar_configure(lambda_h, lambda_J)
    return ctx


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("N,L,q", [(300, 7, 5), (200, 6, 21)])
def test_objective_and_gradient_match_numpy(N, L, q, monkeypatch):
    X = random_alignment(N, L, q, 1)
    w = np.random.default_rng(2).uniform(0.2, 1.0, N)
    x = random_model(L, q, 3, scale=0.4)
    ctx = ar_context(X, q, w)
    ctx.ar_set_x(x)
    assert np.array_equal(ctx.ar_get_x(), x)
    fx = ctx.ar_gradient()
    g = ctx.ar_get_g()
    f_ref, g_ref = objective_ref(x, X, w, L, q, 0.01, 0.02)
    assert abs(fx - f_ref) <= 1e-12 * abs(f_ref)
    assert rel(g, g_ref) <= 1e-12
    assert ctx.ar_gradient() == fx and np.array_equal(ctx.ar_get_g(), g)          # repeats: the same bits
    monkeypatch.setenv("DCA_AR_PASS", "37")                                        # 37-sequence passes: several boundaries
    small = ar_context(X, q, w)
    small.ar_set_x(x)
    fs = small.ar_gradient()
    assert abs(fs - fx) <= 1e-12 * abs(fx) and rel(small.ar_get_g(), g) <= 1e-12
    assert small.ar_gradient() == fs


def test_state_and_argument_errors():
    X = random_alignment(20, 4, 5, 4)
    ctx = _lib.Context(0, _lib.DCA_F64)
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_gradient()
    assert e.value.code == _lib.DCA_ERR_STATE
    ctx.set_msa(X, 5)
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_configure(0.1, 0.1)                                                  # no weights yet
    assert e.value.code == _lib.DCA_ERR_STATE
    ctx.compute_weights(0.8, _lib.DCA_F64)
    for lh, lJ in ((-1.0, 0.1), (0.1, float('inf')), (float('nan'), 0.1)):
        with pytest.raises(_lib.DcaBackendError) as e:
            ctx.ar_configure(lh, lJ)
        assert e.value.code == _lib.DCA_ERR_ARG
    ctx.ar_configure(0.1, 0.1)
    assert ctx.ar_num_params() == ctx.num_params()
    for args in ((-1, 1e-5), (10, -1.0), (10, float('nan'))):
        with pytest.raises(_lib.DcaBackendError) as e:
            ctx.ar_fit(*args)
        assert e.value.code == _lib.DCA_ERR_ARG
    bad = X[:2].copy()
    bad[1, 2] = 5
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_log_probabilities(bad)
    assert e.value.code == _lib.DCA_ERR_ARG
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_sample(-1)
    assert e.value.code == _lib.DCA_ERR_ARG
    assert ctx.ar_log_probabilities(X[:0]).shape == (0,) and ctx.ar_sample(0).shape == (0, 4)
    ctx.set_weights(np.ones(20))                                                   # new weights: configure again
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_gradient()
    assert e.value.code == _lib.DCA_ERR_STATE
    ctx.ar_log_probabilities(X)                                                    # x is still there
    ctx.ar_release()
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_sample(3)
    assert e.value.code == _lib.DCA_ERR_STATE


@pytest.mark.parametrize("L,q", [(9, 5), (6, 21)])
def test_log_probabilities_match_numpy_and_are_batch_invariant(L, q, monkeypatch):
    X = random_alignment(40, L, q, 5)
    x = random_model(L, q, 6)
    ctx = ar_context(X, q)
    ctx.ar_set_x(x)
    Q = random_alignment(700, L, q, 7)
    logp, site, cond = ctx.ar_log_probabilities(Q, per_site=True, conditionals=True)
    lp_ref, site_ref = log_probabilities_ref(x, Q, L, q)
    assert rel(logp, lp_ref) <= 1e-12 and rel(site, site_ref) <= 1e-12
    assert rel(cond, conditionals_ref(x, Q, L, q)) <= 1e-12
    s = np.zeros(Q.shape[0])
    for l in range(L):
        s = s + site[:, l]
    assert np.array_equal(s, logp)                                                 # ascending sum of the site values, bit for bit
    perm = np.random.default_rng(8).permutation(Q.shape[0])[:333]
    assert np.array_equal(ctx.ar_log_probabilities(Q[perm]), logp[perm])
    assert np.array_equal(ctx.ar_log_probabilities(Q[5:6]), logp[5:6])
    monkeypatch.setenv("DCA_AR_PASS", "50")
    assert np.array_equal(ctx.ar_log_probabilities(Q), logp)


# (2, 5): site 0 has no chunk at all; (17, 8): QM = 8, 16 blocks per chunk and one block into a second chunk; (19, 9): the first
# q of QM = 24; (8, 24): q = QM, no padding column; (7, 25): the first q of QM = 32, 2 blocks per chunk; (5, 32): q = QM = 32.
# 600 queries cross the 256-lane and the 512-query block boundary.
@pytest.mark.parametrize("L,q", [(2, 5), (17, 8), (19, 9), (8, 24), (7, 25), (5, 32)])
def test_log_probabilities_at_chunk_and_padding_edges(L, q):
    ctx = ar_context(random_alignment(16, L, q, L * q), q)
    x = random_model(L, q, L + q)
    ctx.ar_set_x(x)
    Q = random_alignment(600, L, q, 17)
    logp, site, cond = ctx.ar_log_probabilities(Q, per_site=True, conditionals=True)
    lp_ref, site_ref = log_probabilities_ref(x, Q, L, q)
    assert rel(logp, lp_ref) <= 1e-12 and rel(site, site_ref) <= 1e-12
    assert rel(cond, conditionals_ref(x, Q, L, q)) <= 1e-12
    assert np.array_equal(np.cumsum(site, 1)[:, -1], logp)                         # ascending sum of the site values, bit for bit
    assert np.array_equal(site, cond[np.arange(600)[:, None], np.arange(L)[None, :], Q.astype(np.int64)])


@pytest.mark.parametrize("L,q", [(9, 5), (7, 21), (5, 30)])
def test_last_site_conditionals_equal_the_pseudo_likelihood_ones(L, q):
    """At the last site the arDCA and the Potts conditionals are the same sum, term for term and in the same order: h first,
    then the blocks (k, L-1) for k ascending, read as J(s_k, .).  Both kernels run one body, so the bits agree.  The plm engine
    holds models of q = 5 and q = 21 only; at q = 30 the Potts model is the mean-field one of a random alignment, and arDCA
    gets the same numbers in the plm layout (zero on the gap state, as the mean-field source reads it)."""
    ctx = ar_context(random_alignment(64, L, q, 18), q)
    if q in (5, 21):
        x = np.random.default_rng(L * q).normal(0, 0.3, L * q + L * (L - 1) // 2 * q * q)
        ctx.plm_configure(1.0, 1.0)
        ctx.plm_set_x(x)
        entry = ctx.plm_pseudo_likelihood
    else:
        ctx.mf_corr_mat(0.5, want=False)
        h, Jp = mf_model(ctx.mf_couplings(), ctx.mf_fields(), L, q)
        x = np.concatenate([h.ravel(), Jp.ravel()])
        entry = ctx.mf_pseudo_likelihood
    ctx.ar_set_x(x)
    Q = random_alignment(600, L, q, 19)
    _pll, cond_pll = entry(Q, conditionals=True)
    _lp, cond_ar = ctx.ar_log_probabilities(Q, conditionals=True)
    assert np.array_equal(cond_pll[:, L - 1, :], cond_ar[:, L - 1, :])


@pytest.mark.parametrize("L,q", [(4, 5), (3, 21)])
def test_enumeration_on_the_gpu_sums_to_one(L, q):
    X = random_alignment(10, L, q, 9)
    ctx = ar_context(X, q)
    ctx.ar_set_x(random_model(L, q, 10, scale=0.7))
    allX = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.uint8)
    assert abs(np.exp(ctx.ar_log_probabilities(allX)).sum() - 1.0) <= 1e-12


def _scipy_fit(X, w, L, q, lh, lJ):
    from scipy.optimize import minimize
    res = minimize(lambda v: objective_ref(v, X, w, L, q, lh, lJ), np.zeros(L * q + L * (L - 1) // 2 * q * q), jac=True,
                   method='L-BFGS-B', options=dict(maxiter=20000, maxcor=20, gtol=1e-13, ftol=1e-16))
    return res.x, res.fun


def test_fit_matches_scipy_on_a_synthetic_alignment():
    N, L, q = 300, 12, 21
    rng = np.random.default_rng(11)
    X = (np.minimum(rng.geometric(0.35, size=(N, L)) - 1, q - 1)).astype(np.uint8)   # skewed states: a structured profile
    X[:, 6] = (X[:, 2] + X[:, 4]) % q                                                # and some correlations
    lh, lJ = 1e-2, 1e-2
    ctx = ar_context(X, q, lambda_h=lh, lambda_J=lJ)
    w = ctx.weights()
    st = ctx.ar_fit(1000, 1e-8)
    assert st['status'] == _lib.AR_CONVERGED, st
    x = ctx.ar_get_x()
    assert st["gnorm"] <= 1e-8 * max(1.0, np.linalg.norm(x))
    xs, fs = _scipy_fit(X, w, L, q, lh, lJ)
    assert np.max(np.abs(x - xs)) <= 1e-6 * np.max(np.abs(xs)), np.max(np.abs(x - xs))
    assert abs(st['fx'] - fs) <= 1e-10 * abs(fs)
    ctx.ar_init_x()
    st2 = ctx.ar_fit(1000, 1e-8)
    assert np.array_equal(ctx.ar_get_x(), x) and st2['fx'] == st['fx'] and st2['iterations'] == st['iterations']


@pytest.mark.parametrize("name,bio", [("toy_protein.fa", "protein"), ("toy_rna.fa", "rna")])
def test_fit_converges_on_the_toy_alignments(name, bio):
    inst = ArDCA(data_file(name), bio)
    st = inst.fit()
    assert st['status'] == 'converged', st
    x, order = inst.get_fields_and_couplings()
    assert st['gnorm'] <= 1e-5 * max(1.0, np.linalg.norm(x))
    assert sorted(order.tolist()) == list(range(inst.sequences_len))
    assert inst.last_status['fx'] == st['fx']


# (19, 9, 37), (13, 24, 33), (9, 32, 20): the instantiations QM = 24 and QM = 32 (q = 24 and q = 32 without a padding column),
# lanes that add four and more terms, code slots 0 .. 4 at L = 19, chain counts that are no multiple of the 16 of a wave.  The
# seeds are the same: the restatement's margin at these shapes is 7e-6 and more.
@pytest.mark.parametrize("L,q,n", [(7, 5, 200), (6, 21, 150), (19, 9, 37), (13, 24, 33), (9, 32, 20)])
def test_sampler_is_bit_exact_and_split_invariant(L, q, n):
    cut, one = (37, 50) if n > 50 else (n // 2, n - 1)                              # where the run is split; a chain drawn alone
    X = random_alignment(10, L, q, 12)
    x = random_model(L, q, 13, scale=0.8)
    ctx = ar_context(X, q)
    ctx.ar_set_x(x)
    codes = ctx.ar_sample(n, seed=77)
    ref, margin = sample_ref(x, L, q, n, seed=77)
    print("smallest |cumsum - r| / T of the restatement: %.3e" % margin)
    assert margin > 1e-12
    assert np.array_equal(codes, ref)
    assert np.array_equal(ctx.ar_sample(n, seed=77), codes)
    a = ctx.ar_sample(cut, seed=77)
    b = ctx.ar_sample(n - cut, seed=77, first_chain=cut)
    assert np.array_equal(np.concatenate([a, b]), codes)
    assert np.array_equal(ctx.ar_sample(1, seed=77, first_chain=one), codes[one:one + 1])
    assert not np.array_equal(ctx.ar_sample(n, seed=78), codes)


def test_sampler_reproduces_the_enumerated_distribution():
    L, q, n = 3, 5, 200000
    X = random_alignment(10, L, q, 14)
    ctx = ar_context(X, q)
    ctx.ar_set_x(random_model(L, q, 15, scale=0.8))
    codes = ctx.ar_sample(n, seed=3)
    allX = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.uint8)
    P = np.exp(ctx.ar_log_probabilities(allX))
    idx = (codes.astype(np.int64) * (q ** np.arange(L - 1, -1, -1))).sum(axis=1)
    emp = np.bincount(idx, minlength=q ** L) / n
    # E|emp_c - P_c| <= sqrt(P_c (1 - P_c) / n): the expected total variation is at most half their sum (0.011 here);
    # three times that bound fails with negligible probability at a fixed seed
    bound = 3 * np.sum(np.sqrt(P * (1 - P) / n)) / 2
    assert 0.5 * np.abs(emp - P).sum() < bound


def test_class_matches_the_library_on_permuted_columns():
    path = data_file('toy_protein.fa')
    probe = ArDCA(path, 'protein', order='natural')
    L = probe.sequences_len
    perm = np.random.default_rng(16).permutation(L)
    inst = ArDCA(path, 'protein', order=perm, max_iterations=50)
    inst.fit()
    X, _raw = _lib.read_msa(path, _lib.DCA_BIOMOLECULE_PROTEIN, L)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, 21)
    w = ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.set_msa(np.ascontiguousarray(X[:, perm]), 21)
    ctx.set_weights(w)
    ctx.ar_configure(1e-6, 1e-2)
    ctx.ar_fit(50, 1e-5)
    x, order = inst.get_fields_and_couplings()
    assert np.array_equal(order, perm) and np.array_equal(x, ctx.ar_get_x())
    logp, site = inst.compute_sequence_log_probabilities(per_site=True)
    Q = _potts.query_codes(path, _lib.DCA_BIOMOLECULE_PROTEIN, L, 0, ValueError)
    lp_lib, site_lib = ctx.ar_log_probabilities(Q[:, perm], per_site=True)
    assert np.array_equal(logp, lp_lib) and np.array_equal(site[:, perm], site_lib)
    cond = inst.compute_conditional_log_probabilities(path)
    assert np.allclose(np.exp(cond).sum(axis=2), 1.0, atol=1e-12)
    codes = inst.sample_sequences(64, seed=4, return_codes=True)
    assert np.array_equal(codes[:, perm], ctx.ar_sample(64, seed=4))
    seqs = inst.sample_sequences(3, seed=4)
    assert len(seqs) == 3 and all(len(s) == L for s in seqs)
    ll = inst.compute_log_likelihood()
    lp_train, _s = ctx.ar_log_probabilities(np.ascontiguousarray(X[:, perm]), per_site=True)
    assert abs(ll - np.dot(w, lp_train) / w.sum()) <= 1e-12 * abs(ll)
    wt = Q[0]
    letters = 'ACDEFGHIKLMNPQRSTVWY-'
    d = inst.compute_single_mutant_effects(''.join(letters[c] for c in wt))
    assert d.shape == (L, 21) and np.all(d[np.arange(L), wt] == 0.0)
    i, a = 3, (int(wt[3]) + 2) % 21
    mut = wt.copy()
    mut[i] = a
    lp = inst.compute_sequence_log_probabilities([''.join(letters[c] for c in s) for s in (mut, wt)])
    assert d[i, a] == lp[0] - lp[1]


def test_every_subcommand_writes_its_file(tmp_path):
    path = data_file('toy_protein.fa')
    out = str(tmp_path)
    params, fit = ardca_main.run_ardca(['fit', 'protein', path, '--output_dir', out, '--max_iterations', '30'])
    assert os.path.basename(params) == 'ARDCA_params_toy_protein.npy' and os.path.basename(fit) == 'ARDCA_fit_toy_protein.txt'
    assert np.load(params).size == _lib.lib().dca_ar_num_params(ArDCA(path, 'protein').sequences_len, 21)
    lp = ardca_main.run_ardca(['compute_log_probabilities', 'protein', path, '--output_dir', out, '--max_iterations', '30'])
    assert os.path.basename(lp) == 'ARDCA_log_probabilities_toy_protein.txt'
    rows = [r for r in open(lp).read().splitlines() if not r.startswith('#')]
    assert len(rows) == ArDCA(path, 'protein').num_sequences
    ll = ardca_main.run_ardca(['compute_log_likelihood', 'protein', path, '--output_dir', out, '--max_iterations', '30'])
    assert os.path.basename(ll) == 'ARDCA_log_likelihood_toy_protein.txt'
    assert 'Weighted log-likelihood per effective sequence' in open(ll).read()
    fa = ardca_main.run_ardca(['sample_sequences', 'protein', path, '--output_dir', out, '--num_sequences', '5', '--seed', '2',
                               '--max_iterations', '30'])
    assert os.path.basename(fa) == 'ARDCA_samples_toy_protein.fa'
    assert sum(1 for r in open(fa) if r.startswith('>sample_')) == 5
    wt = tmp_path / 'wt.fa'
    with open(path) as fh:
        wt.write_text(''.join(fh.readlines()[:2]))
    me = ardca_main.run_ardca(['compute_mutation_effects', 'protein', path, '--output_dir', out, '--wildtype_file', str(wt),
                               '--max_iterations', '30'])
    assert os.path.basename(me) == 'ARDCA_mutation_effects_toy_protein.txt'
    rows = [r for r in open(me).read().splitlines() if not r.startswith('#')]
    assert len(rows) == ArDCA(path, 'protein').sequences_len * 21
