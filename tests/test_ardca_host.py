"""Host-side checks of the autoregressive model (arDCA): a float64 numpy restatement of the conditionals, log P, the objective
and its gradient (checked against central differences and exact enumeration), the draw rule of the ancestral sampler, the
entropic site order and the permutations of the class, argument validation, and the command line's parsing and writers.
The restatement is the reference of the GPU tests in tests/test_ardca.py."""
import itertools
import os

import numpy as np
import pytest

from conftest import data_file
from test_potts_sampling_host import philox_np
from pydca_amd import ardca_main
from pydca_amd.ardca import ardca
from pydca_amd.ardca.ardca import ArDCA, ArDCAException


def pair_index(L, k, l):
    return L * (L - 1) // 2 - (L - k) * (L - k - 1) // 2 + (l - k - 1)


def unpack(x, L, q):
    """x (plm layout) -> h[L, q], J[L, L, q, q] with J[k, l] the block of the pair k < l (zero elsewhere)."""
    x = np.asarray(x, dtype=np.float64)
    h = x[:L * q].reshape(L, q)
    J = np.zeros((L, L, q, q))
    for k in range(L):
        for l in range(k + 1, L):
            p = pair_index(L, k, l)
            J[k, l] = x[L * q + p * q * q: L * q + (p + 1) * q * q].reshape(q, q)
    return h, J


def conditionals_ref(x, X, L, q):
    """cond[n, l, b] = log P(s_l = b | s_<l) in the library's order: u = h_l, then + J_kl(s_k, .) for k ascending; the
    log-softmax as (u - m) - log sum exp(u - m)."""
    h, J = unpack(x, L, q)
    X = np.asarray(X, dtype=np.int64)
    n = X.shape[0]
    cond = np.zeros((n, L, q))
    for l in range(L):
        u = np.repeat(h[l][None, :], n, axis=0).copy()
        for k in range(l):
            u = u + J[k, l][X[:, k]]
        m = u.max(axis=1, keepdims=True)
        z = np.zeros(n)
        for b in range(q):
            z = z + np.exp(u[:, b] - m[:, 0])
        cond[:, l] = (u - m) - np.log(z)[:, None]
    return cond


def log_probabilities_ref(x, X, L, q):
    """-> (logp[n], site[n, L]); logp the ascending sum of the site values"""
    cond = conditionals_ref(x, X, L, q)
    X = np.asarray(X, dtype=np.int64)
    site = np.take_along_axis(cond, X[:, :, None], axis=2)[:, :, 0]
    logp = np.zeros(X.shape[0])
    for l in range(L):
        logp = logp + site[:, l]
    return logp, site


def objective_ref(x, X, w, L, q, lambda_h, lambda_J):
    """f(x) and its gradient (include/dca_hip.h) with W = w / sum w"""
    x = np.asarray(x, dtype=np.float64)
    X = np.asarray(X, dtype=np.int64)
    W = np.asarray(w, dtype=np.float64) / np.sum(w)
    cond = conditionals_ref(x, X, L, q)
    site = np.take_along_axis(cond, X[:, :, None], axis=2)[:, :, 0]
    f = -np.dot(W, site.sum(axis=1)) + lambda_h * np.sum(x[:L * q] ** 2) + lambda_J * np.sum(x[L * q:] ** 2)
    onehot = np.eye(q)[X]                                      # n x L x q
    R = W[:, None, None] * (np.exp(cond) - onehot)
    g = np.zeros_like(x)
    g[:L * q] = R.sum(axis=0).reshape(-1)
    for k in range(L):
        for l in range(k + 1, L):
            p = pair_index(L, k, l)
            g[L * q + p * q * q: L * q + (p + 1) * q * q] = (onehot[:, k, :].T @ R[:, l, :]).reshape(-1)
    g[:L * q] += 2 * lambda_h * x[:L * q]
    g[L * q:] += 2 * lambda_J * x[L * q:]
    return f, g


def philox_uniform(seed, chain, sweep, site, tag):
    ctr = np.array([chain & 0xffffffff, sweep & 0xffffffff, site & 0xffffffff, tag], dtype=np.uint64)
    w = philox_np(ctr, (seed & 0xffffffff, seed >> 32))
    return float((int(w[0]) >> 5) * 67108864 + (int(w[1]) >> 6)) * 2.0 ** -53


def sample_ref(x, L, q, n, seed, first_chain=0):
    """Ancestral sampling as dca_ar_sample defines it -> (codes uint8[n, L], the smallest |cumsum - r| / T met)"""
    h, J = unpack(x, L, q)
    out = np.zeros((n, L), dtype=np.uint8)
    margin = np.inf
    for c in range(n):
        chain = first_chain + c
        s = []
        for l in range(L):
            parts = []
            for w in range(4):
                acc = h[l].copy() if w == 0 else np.zeros(q)
                for k in range(w, l, 4):
                    acc = acc + J[k, l][s[k]]
                parts.append(acc)
            u = parts[0]
            for w in range(1, 4):
                u = u + parts[w]
            m = u.max()
            p = np.exp(u - m)
            T = 0.0
            for b in range(q):
                T += p[b]
            r = philox_uniform(seed, chain, 0, l, 3) * T
            cum, pick, last = 0.0, -1, 0
            for b in range(q):
                cum += p[b]
                margin = min(margin, abs(cum - r) / T)
                if pick < 0 and cum > r:
                    pick = b
                if p[b] > 0:
                    last = b
            s.append(pick if pick >= 0 else last)
        out[c] = s
    return out, margin


def random_model(L, q, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, scale, L * q + L * (L - 1) // 2 * q * q)


def random_alignment(N, L, q, seed):
    return np.random.default_rng(seed).integers(0, q, size=(N, L)).astype(np.uint8)


# ---- the restatement itself
@pytest.mark.parametrize("L,q", [(4, 5), (3, 21)])
def test_enumeration_sums_to_one(L, q):
    x = random_model(L, q, 1)
    X = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.uint8)
    logp, _site = log_probabilities_ref(x, X, L, q)
    assert abs(np.exp(logp).sum() - 1.0) < 1e-12


def test_conditionals_are_normalised_and_causal():
    L, q = 5, 5
    x = random_model(L, q, 2)
    X = random_alignment(20, L, q, 3)
    cond = conditionals_ref(x, X, L, q)
    assert np.allclose(np.exp(cond).sum(axis=2), 1.0, atol=1e-14)
    Y = X.copy()
    Y[:, 3] = (Y[:, 3] + 1) % q                                # a later site does not change the earlier conditionals
    cy = conditionals_ref(x, Y, L, q)
    assert np.array_equal(cond[:, :4], cy[:, :4])
    assert np.allclose(conditionals_ref(x, X, L, q)[:, 0], np.log(np.exp(x[:q]) / np.exp(x[:q]).sum())[None, :], atol=1e-14)


@pytest.mark.parametrize("L,q", [(4, 5), (3, 21)])
def test_gradient_matches_central_differences(L, q):
    x = random_model(L, q, 4, scale=0.3)
    X = random_alignment(30, L, q, 5)
    w = np.random.default_rng(6).uniform(0.2, 1.0, 30)
    lh, lJ = 0.01, 0.02
    f, g = objective_ref(x, X, w, L, q, lh, lJ)
    rng = np.random.default_rng(7)
    idx = np.concatenate([rng.choice(L * q, 10, replace=False), L * q + rng.choice(x.size - L * q, 20, replace=False)])
    eps = 1e-6
    for i in idx:
        xp, xm = x.copy(), x.copy()
        xp[i] += eps
        xm[i] -= eps
        num = (objective_ref(xp, X, w, L, q, lh, lJ)[0] - objective_ref(xm, X, w, L, q, lh, lJ)[0]) / (2 * eps)
        assert abs(num - g[i]) <= 1e-7 * max(1.0, abs(g[i])), (i, num, g[i])


def test_objective_is_negative_weighted_log_likelihood_without_penalty():
    L, q = 4, 5
    x = random_model(L, q, 8)
    X = random_alignment(25, L, q, 9)
    w = np.random.default_rng(10).uniform(0.1, 1.0, 25)
    f, _g = objective_ref(x, X, w, L, q, 0.0, 0.0)
    logp, _site = log_probabilities_ref(x, X, L, q)
    assert abs(f + np.dot(w, logp) / w.sum()) < 1e-12


def test_sampler_restatement_is_exact_on_a_tiny_model():
    L, q = 3, 5
    x = random_model(L, q, 11, scale=0.8)
    codes, margin = sample_ref(x, L, q, 4000, seed=5)
    assert margin > 1e-12
    X = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.uint8)
    P = np.exp(log_probabilities_ref(x, X, L, q)[0])
    idx = (codes.astype(np.int64) * (q ** np.arange(L - 1, -1, -1))).sum(axis=1)
    emp = np.bincount(idx, minlength=q ** L) / codes.shape[0]
    # total variation of 4000 draws over 125 cells: E TV <= sum sqrt(p (1 - p) / n) / 2
    bound = 3 * np.sum(np.sqrt(P * (1 - P) / codes.shape[0])) / 2
    assert 0.5 * np.abs(emp - P).sum() < bound


# ---- entropic order and permutations of the class
def test_entropic_order_is_ascending_and_stable():
    q = 5
    X = np.array([[0, 1, 2, 0], [0, 1, 3, 0], [0, 2, 4, 1], [0, 2, 0, 1]], dtype=np.uint8)
    w = np.ones(4)
    H = ardca.site_entropies(X, w, q)
    assert H[0] == 0.0
    assert np.isclose(H[1], np.log(2)) and np.isclose(H[3], np.log(2)) and np.isclose(H[2], np.log(4))
    assert ardca.entropic_order(X, w, q).tolist() == [0, 1, 3, 2]        # tie of sites 1 and 3 in ascending site number
    w2 = np.array([1.0, 1.0, 0.0, 0.0])                                   # zero weights drop rows: 0 log 0 = 0
    assert ardca.site_entropies(X, w2, q)[1] == 0.0


def test_explicit_order_validation():
    assert ardca.explicit_order([2, 0, 1], 3).tolist() == [2, 0, 1]
    for bad in ([0, 1], [0, 0, 1], [0, 1, 3], [[0, 1, 2]], [0.5, 1, 2], 'x'):
        with pytest.raises(ArDCAException):
            ardca.explicit_order(bad, 3)


def test_class_permutes_queries_and_samples_round_trip():
    path = data_file('toy_protein.fa')
    inst = ArDCA(path, 'protein', order='natural')
    L = inst.sequences_len
    assert inst.site_order.tolist() == list(range(L))
    perm = np.random.default_rng(1).permutation(L)
    inst = ArDCA(path, 'protein', order=perm)
    assert inst.site_order.tolist() == perm.tolist() and inst.order == 'explicit'
    X = random_alignment(7, L, 21, 2)
    Xm = inst._to_model(X)
    assert np.array_equal(Xm, X[:, perm])
    back = np.empty_like(Xm)
    back[:, inst.site_order] = Xm                                          # what sample_sequences does with model codes
    assert np.array_equal(back, X)
    site = np.arange(L, dtype=np.float64)[None, :] + 0 * Xm               # model position j carries the value j
    inv = np.argsort(inst.site_order)
    assert np.array_equal(site[:, inv][0, perm], np.arange(L))


def test_class_argument_validation():
    path = data_file('toy_rna.fa')
    ArDCA(path, 'RNA')
    for kw in (dict(seqid=0.0), dict(seqid=1.5), dict(lambda_h=-1.0), dict(lambda_J=float('nan')), dict(max_iterations=-1),
               dict(max_iterations=2.5), dict(epsilon=-1e-5), dict(order='random'), dict(order=[0, 1]), dict(device=-1)):
        with pytest.raises(ArDCAException):
            ArDCA(path, 'rna', **kw)
    with pytest.raises(ArDCAException):
        ArDCA(path, 'dna')
    with pytest.raises(FileNotFoundError):
        ArDCA(path + '.missing', 'rna')
    inst = ArDCA(path, 'rna')
    assert (inst.lambda_h, inst.lambda_J, inst.max_iterations, inst.epsilon, inst.order) == (1e-6, 1e-2, 1000, 1e-5, 'entropy')
    with pytest.raises(ArDCAException):
        inst.compute_sequence_log_probabilities(per_site='yes')
    with pytest.raises(ArDCAException):
        inst.compute_conditional_log_probabilities(None)
    with pytest.raises(ArDCAException):
        inst.sample_sequences(-1)
    with pytest.raises(ArDCAException):
        inst.compute_single_mutant_effects('AC')                            # wrong length: rejected on the host


# ---- command line
def test_command_line_parsing():
    p = ardca_main.build_parser()
    a = vars(p.parse_args(['sample_sequences', 'protein', 'x.fa', '--num_sequences', '5', '--seed', '3', '--order', 'natural',
                           '--lambda_J', '0.1', '--epsilon', '1e-6']))
    assert (a['subcommand_name'], a['num_sequences'], a['seed'], a['order'], a['lambda_J'], a['epsilon']) == \
        ('sample_sequences', 5, 3, 'natural', 0.1, 1e-6)
    a = vars(p.parse_args(['compute_mutation_effects', 'rna', 'x.fa', '--wildtype_file', 'w.fa']))
    assert a['wildtype_file'] == 'w.fa' and a['order'] is None
    a = vars(p.parse_args(['compute_log_probabilities', 'rna', 'x.fa', '--query_file', 'q.fa', '--max_iterations', '7']))
    assert a['query_file'] == 'q.fa' and a['max_iterations'] == 7
    for bad in (['sample_sequences', 'rna', 'x.fa'], ['compute_mutation_effects', 'rna', 'x.fa'], ['fit', 'rna', 'x.fa', '--order', 'x'],
                ['nothing', 'rna', 'x.fa']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert set(p._subparsers._group_actions[0].choices) == set(ardca_main.ARDCA_SUBCOMMANDS)


def test_command_line_writers(tmp_path):
    meta = ['# PARAMETERS USED FOR THIS COMPUTATION: ', '#\tlambda_J: 0.01']
    f = tmp_path / 'lp.txt'
    ardca_main.write_log_probabilities(str(f), [-1.5, -2.25], metadata=meta, query_file='q.fa', weighted=-1.75)
    text = f.read_text()
    assert '#\tQuery sequences: q.fa' in text and 'Weighted log-likelihood per effective sequence: -1.75' in text
    rows = [r for r in text.splitlines() if not r.startswith('#')]
    assert [float(r.split()[1]) for r in rows] == [-1.5, -2.25] and rows[0].split()[0] == '1'
    f = tmp_path / 's.fa'
    ardca_main.write_samples(str(f), ['AC-', 'GGU'], [-0.1, -0.2])
    assert f.read_text().splitlines() == ['>sample_1 log_probability=-0.10000000000000001', 'AC-',
                                          '>sample_2 log_probability=-0.20000000000000001', 'GGU']
    f = tmp_path / 'm.txt'
    d = np.array([[0.0, 1.0], [-2.0, 0.0]])
    ardca_main.write_mutation_effects(str(f), d, ['A', 'C'], ['A', 'C'], metadata=meta, wildtype_file='w.fa')
    rows = [r.split() for r in f.read_text().splitlines() if not r.startswith('#')]
    assert rows == [['1', 'A', 'A', '0'], ['1', 'A', 'C', '1'], ['2', 'C', 'A', '-2'], ['2', 'C', 'C', '0']]
    f = tmp_path / 'fit.txt'
    ardca_main.write_fit(str(f), {'status': 'converged', 'iterations': 3}, np.array([2, 0, 1]), metadata=meta)
    text = f.read_text()
    assert '#\tstatus: converged' in text
    assert [r.split() for r in text.splitlines() if not r.startswith('#')] == [['0', '3'], ['1', '1'], ['2', '2']]
    inst = ArDCA(data_file('toy_rna.fa'), 'rna', order='natural')
    lines = ardca_main.ardca_param_metadata(inst)
    assert lines[0] == '# PARAMETERS USED FOR THIS COMPUTATION: ' and '#\tSite order: natural' in lines
