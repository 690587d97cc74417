"""arDCA epistasis on the GPU (ar_epistasis.hip): dca_ar_epistasis / dca_ar_epistatic_scores against the brute force over explicit
double mutants (through the existing device entry dca_ar_log_probabilities and through numpy), the class in file order, the
contact scores and their ranking, a planted-contact alignment, a shape that crosses several tiles, the command line, errors."""
import os
import time

import numpy as np
import pytest

from conftest import data_file
from test_ardca_host import log_probabilities_ref, pair_index, random_alignment, random_model
from test_ardca_epistasis_host import epistasis_brute, epistasis_ref, random_wildtype, scores_ref
from pydca_amd import _lib, ardca_main
from pydca_amd.ardca import ardca
from pydca_amd.ardca.ardca import ArDCA
from pydca_amd.plmdca.plmdca import PlmDCA

pytestmark = pytest.mark.gpu

LETTERS = {5: 'ACGU-', 21: 'ACDEFGHIKLMNPQRSTVWY-'}


def model_context(x, L, q):
    """A context that holds the model x (any alignment serves: the entries under test read x alone)."""
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(random_alignment(8, L, q, 1), q)
    ctx.set_weights(np.ones(8))
    ctx.ar_configure(0.01, 0.01)
    ctx.ar_set_x(x)
    return ctx


@pytest.mark.parametrize("L,q,scale", [(9, 5, 0.5), (6, 21, 0.5), (7, 5, 2.0)])
def test_epistasis_matches_both_brute_forces(L, q, scale):
    x = random_model(L, q, 300 + L, scale=scale)
    w = random_wildtype(L, q, 400 + L)
    ctx = model_context(x, L, q)
    eps, d = ctx.ar_epistasis(w)
    eps_dev, d_dev = epistasis_brute(lambda X: ctx.ar_log_probabilities(X), L, q, w)
    eps_np, d_np = epistasis_brute(lambda X: log_probabilities_ref(x, X, L, q)[0], L, q, w)
    eps_f, d_f = epistasis_ref(x, L, q, w)
    print("L %d q %d scale %g: max |eps| %.3g; eps vs device brute %.3g, numpy brute %.3g, factored numpy %.3g; d %.3g, %.3g, %.3g" % (
        L, q, scale, np.abs(eps).max(), np.abs(eps - eps_dev).max(), np.abs(eps - eps_np).max(), np.abs(eps - eps_f).max(),
        np.abs(d - d_dev).max(), np.abs(d - d_np).max(), np.abs(d - d_f).max()))
    for ref in (eps_dev, eps_np):
        assert np.abs(eps - ref).max() <= 1e-12
    for ref in (d_dev, d_np):
        assert np.abs(d - ref).max() <= 1e-12
    for k in range(L):
        assert d[k, w[k]] == 0.0
        for l in range(k + 1, L):
            e = eps[pair_index(L, k, l)]
            assert not e[w[k]].any() and not e[:, w[l]].any()
    # the same bits on every call and whichever outputs are asked for
    e2, d2 = ctx.ar_epistasis(w)
    e3, none = ctx.ar_epistasis(w, single=False)
    none2, d3 = ctx.ar_epistasis(w, eps=False)
    assert none is None and none2 is None
    assert np.array_equal(e2, eps) and np.array_equal(e3, eps) and np.array_equal(d2, d) and np.array_equal(d3, d)
    assert np.array_equal(ctx.ar_get_x(), x)


@pytest.mark.parametrize("L,q", [(9, 5), (6, 21), (2, 5)])
def test_scores_match_numpy_on_the_returned_table(L, q):
    x = random_model(L, q, 500 + L, scale=0.5)
    w = random_wildtype(L, q, 600 + L)
    ctx = model_context(x, L, q)
    eps, _d = ctx.ar_epistasis(w, single=False)
    fn = ctx.ar_epistatic_scores(w, apc=False)
    order_fn = ctx.scores_order()
    apc = ctx.ar_epistatic_scores(w, apc=True)
    order_apc = ctx.scores_order()
    fn_ref, apc_ref = scores_ref(eps, L, q, False), scores_ref(eps, L, q, True)
    print("L %d q %d: FN rel %.3g, APC |diff| / FN %.3g" % (L, q, np.max(np.abs(fn - fn_ref) / fn_ref), np.max(np.abs(apc - apc_ref) / fn_ref)))
    assert np.all(np.abs(fn - fn_ref) <= 1e-12 * fn_ref)
    # an APC score is a difference of two numbers of FN's size and crosses zero: relative to the uncorrected score of its pair
    assert np.all(np.abs(apc - apc_ref) <= 1e-12 * fn_ref)
    assert np.array_equal(order_fn, np.argsort(-fn, kind='stable')) and np.array_equal(order_apc, np.argsort(-apc, kind='stable'))
    assert np.array_equal(ctx.ar_epistatic_scores(w, apc=True), apc)


@pytest.mark.parametrize("name,bio,q", [("toy_protein.fa", "protein", 21), ("toy_rna.fa", "rna", 5)])
def test_class_in_file_order_on_a_permuted_model(name, bio, q):
    path = data_file(name)
    L = ArDCA(path, bio, order='natural').sequences_len
    rng = np.random.default_rng(21)
    perm = rng.permutation(L)
    inst = ArDCA(path, bio, order=perm, max_iterations=40)
    pairs = [tuple(int(v) for v in rng.choice(L, size=2, replace=False)) for _ in range(20)]
    wt_codes = inst._wildtype(None)
    letters = LETTERS[q]
    eff = inst.compute_double_mutant_effects(pairs=pairs)
    eps = inst.compute_epistasis(pairs=pairs)
    assert eff.shape == eps.shape == (20, q, q)
    worst, scale = 0.0, 0.0
    for n, (i, j) in enumerate(pairs):
        rows = np.repeat(wt_codes[None, :], q * q + 1, axis=0)
        idx = np.arange(q * q)
        rows[idx, i] = idx // q
        rows[idx, j] = idx % q
        lp = inst.compute_sequence_log_probabilities([''.join(letters[c] for c in r) for r in rows])
        ref = (lp[:q * q] - lp[q * q]).reshape(q, q)
        worst, scale = max(worst, np.abs(eff[n] - ref).max()), max(scale, np.abs(lp).max())
        assert np.abs(eff[n] - ref).max() <= 1e-12 * (1.0 + np.abs(lp).max())
    print("%s: double-mutant effects vs explicit mutants %.3g (max |log P| %.3g)" % (name, worst, scale))
    swapped = inst.compute_epistasis(pairs=[(j, i) for i, j in pairs])
    assert np.array_equal(swapped, np.transpose(eps, (0, 2, 1)))
    assert np.array_equal(inst.compute_epistasis(pairs=pairs), eps)
    every = inst.compute_epistasis()
    assert every.shape == (L * (L - 1) // 2, q, q)
    for n, (i, j) in enumerate(pairs):
        blk = every[pair_index(L, min(i, j), max(i, j))]
        assert np.array_equal(eps[n], blk if i < j else blk.T)
    # the single-mutant part equals the existing scan to rounding
    d = inst.compute_single_mutant_effects(''.join(letters[c] for c in wt_codes))
    i, j = pairs[0]
    a, b = (int(wt_codes[i]) + 1) % q, (int(wt_codes[j]) + 1) % q
    assert abs((eff[0][a, b] - eps[0][a, b]) - (d[i, a] + d[j, b])) <= 1e-12 * (1.0 + scale)

    # ranking: numpy's stable descending sort of the device's scores, relabelled to file sites
    ctx = inst._fitted_context()
    for apc, method in ((False, inst.compute_sorted_FN), (True, inst.compute_sorted_FN_APC)):
        by_file = ardca.file_pair_scores(ctx.ar_epistatic_scores(wt_codes[perm], apc=apc), perm)
        ranked = method()
        iu, ju = np.triu_indices(L, k=1)
        order = np.argsort(-by_file, kind='stable')
        assert [p for p, _s in ranked] == [(int(iu[n]), int(ju[n])) for n in order]
        assert np.array_equal(np.array([s for _p, s in ranked]), by_file[order])

        class Mapper:
            def map_to_reference_sequence(self):
                return {i: 100 + 2 * i for i in range(L) if i % 3}
        mapped = method(seqbackmapper=Mapper())
        assert mapped == PlmDCA(path, bio).get_mapped_site_pairs_dca_scores(ranked, Mapper())
        assert 0 < len(mapped) < len(ranked)


def test_natural_order_ranks_with_the_device_order():
    inst = ArDCA(data_file("toy_rna.fa"), 'rna', order='natural', max_iterations=40)
    L = inst.sequences_len
    ranked = inst.compute_sorted_FN_APC()
    ctx = inst._fitted_context()
    scores = ctx.ar_epistatic_scores(inst._wildtype(None), apc=True)
    iu, ju = np.triu_indices(L, k=1)
    order = np.argsort(-scores, kind='stable')
    assert [p for p, _s in ranked] == [(int(iu[n]), int(ju[n])) for n in order]
    assert np.array_equal(np.array([s for _p, s in ranked]), scores[order])


def test_planted_contacts_lead_the_ranking(tmp_path):
    L, q = 20, 5
    planted = [(0, 7), (2, 11), (4, 15), (9, 18), (12, 19)]
    rng = np.random.default_rng(31)
    x = np.zeros(L * q + L * (L - 1) // 2 * q * q)
    x[:L * q] = rng.normal(0.0, 0.3, L * q)
    for k, l in planted:
        p = pair_index(L, k, l)
        x[L * q + p * q * q: L * q + (p + 1) * q * q] = (2.0 * np.eye(q) + rng.normal(0.0, 0.1, (q, q))).reshape(-1)
    ctx = model_context(x, L, q)
    codes = ctx.ar_sample(2000, seed=5)
    # the generating model itself: the planted pairs must lead its numpy ranking with a clear gap
    eps_gen, _d = epistasis_ref(x, L, q, codes[0])
    gen = scores_ref(eps_gen, L, q, True)
    top = np.argsort(-gen, kind='stable')
    planted_idx = sorted(pair_index(L, k, l) for k, l in planted)
    assert sorted(top[:5].tolist()) == planted_idx and gen[top[4]] > 10.0 * max(gen[top[5]], 1e-300)
    path = os.path.join(str(tmp_path), "planted.fa")
    with open(path, "w") as fh:
        for n, row in enumerate(codes):
            fh.write(">s%d\n%s\n" % (n, ''.join(LETTERS[q][c] for c in row)))
    inst = ArDCA(path, 'rna', order='natural')
    ranked = inst.compute_sorted_FN_APC()
    print("planted: top 8 %s" % (ranked[:8],))
    assert sorted(p for p, _s in ranked[:5]) == planted


def test_a_shape_that_crosses_several_tiles():
    L, q = 120, 21                                     # 2520 flattened rows: 20 row tiles, 40 column tiles, both ragged
    x = random_model(L, q, 41, scale=0.3)
    w = random_wildtype(L, q, 42)
    ctx = model_context(x, L, q)
    t0 = time.perf_counter()
    eps, d = ctx.ar_epistasis(w)
    seconds = time.perf_counter() - t0
    rng = np.random.default_rng(43)
    pairs = set()
    for k, l in ((0, 1), (0, L - 1), (L - 2, L - 1), (5, 6), (6, 7), (60, 61)):      # tile edges and the diagonal
        pairs.add((k, l))
    while len(pairs) < 50:
        k, l = sorted(int(v) for v in rng.choice(L, size=2, replace=False))
        pairs.add((k, l))
    pairs = sorted(pairs)
    scale = [0.0]

    def logp(X):
        lp = ctx.ar_log_probabilities(X)
        scale[0] = max(scale[0], np.abs(lp).max())
        return lp
    eps_b, d_b = epistasis_brute(logp, L, q, w, pairs)
    got = np.stack([eps[pair_index(L, k, l)] for k, l in pairs])
    print("L 120 q 21: %.3f s; eps vs brute %.3g, d vs brute %.3g, max |log P| %.3g, max |eps| %.3g" % (
        seconds, np.abs(got - eps_b).max(), np.abs(d - d_b).max(), scale[0], np.abs(got).max()))
    # the brute force subtracts four log P of this size: its own rounding is of the order 1e-16 * L * |log P|
    assert np.abs(got - eps_b).max() <= 1e-12 * (1.0 + scale[0])
    assert np.abs(d - d_b).max() <= 1e-12 * (1.0 + scale[0])
    assert seconds < 30.0
    assert np.array_equal(ctx.ar_epistasis(w, single=False)[0], eps)


def test_subcommands_write_their_files(tmp_path):
    path = data_file("toy_rna.fa")
    L = ArDCA(path, 'rna').sequences_len
    npairs = L * (L - 1) // 2
    out = str(tmp_path)
    for apc, name in ((False, 'ARDCA_fn_toy_rna.txt'), (True, 'ARDCA_fn_apc_toy_rna.txt')):
        f = ardca_main.execute_from_command_line('rna', path, the_command='compute_fn', apc=apc, output_dir=out, max_iterations=30)
        assert os.path.basename(f) == name
        rows = [ln.split() for ln in open(f) if not ln.startswith('#')]
        assert len(rows) == npairs and all(len(r) == 3 for r in rows)
        scores = [float(r[2]) for r in rows]
        assert scores == sorted(scores, reverse=True)
    files = ardca_main.execute_from_command_line('rna', path, the_command='compute_epistasis', output_dir=out, max_iterations=30)
    assert [os.path.basename(f) for f in files] == ['ARDCA_epistasis_toy_rna.npy', 'ARDCA_double_mutant_effects_toy_rna.npy']
    eps, eff = np.load(files[0]), np.load(files[1])
    assert eps.shape == eff.shape == (npairs, 5, 5) and eps.dtype == np.float64
    assert np.any(eps != 0.0) and np.any(eff != eps)


def test_state_and_argument_errors():
    L, q = 4, 5
    ctx = _lib.Context(0, _lib.DCA_F64)
    w = np.zeros(L, dtype=np.uint8)
    ctx.set_msa(random_alignment(8, L, q, 1), q)
    for call in (lambda: ctx.ar_epistasis(w), lambda: ctx.ar_epistatic_scores(w)):
        with pytest.raises(_lib.DcaBackendError) as e:
            call()
        assert e.value.code == _lib.DCA_ERR_STATE
    ctx.set_weights(np.ones(8))
    ctx.ar_configure(0.01, 0.01)
    ctx.ar_set_x(random_model(L, q, 7))
    bad = w.copy()
    bad[2] = q
    for call in (lambda: ctx.ar_epistasis(bad), lambda: ctx.ar_epistatic_scores(bad), lambda: ctx.ar_epistasis(w, eps=False, single=False)):
        with pytest.raises(_lib.DcaBackendError) as e:
            call()
        assert e.value.code == _lib.DCA_ERR_ARG
    lib, out = _lib.lib(), np.zeros(L * q)
    assert lib.dca_ar_epistasis(ctx._h, None, None, out.ctypes.data) == _lib.DCA_ERR_ARG
    assert lib.dca_ar_epistatic_scores(ctx._h, None, 1, out.ctypes.data) == _lib.DCA_ERR_ARG
    assert lib.dca_ar_epistatic_scores(ctx._h, w.ctypes.data, 1, None) == _lib.DCA_ERR_ARG
    with pytest.raises(ValueError):
        ctx.ar_epistasis(np.zeros(L + 1, dtype=np.uint8))
    ctx.set_weights(np.ones(8))                        # the weights changed: the entries need x alone and still answer
    assert ctx.ar_epistasis(w)[0].shape == (L * (L - 1) // 2, q, q)
    ctx.ar_release()
    with pytest.raises(_lib.DcaBackendError) as e:
        ctx.ar_epistasis(w)
    assert e.value.code == _lib.DCA_ERR_STATE
