"""Site conditionals and pseudo-log-likelihoods on the GPU (dca_plm_pseudo_likelihood, dca_mf_pseudo_likelihood, the class
methods and the command lines), checked against the float64 numpy restatement of tests/test_pseudo_likelihood_host.py, the
plm objective, the mutation scan and themselves (bitwise invariance)."""
import os

import numpy as np
import pytest

from conftest import data_file, golden, perturbed
from test_pseudo_likelihood_host import conditionals_ref, mf_model, plm_model
from pydca_amd import _lib, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

pytestmark = pytest.mark.gpu


def plm_context(X, q, precision, seed):
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, precision)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_init_x()
    L = X.shape[1]
    dt = np.float64 if precision == _lib.DCA_F64 else np.float32
    x = perturbed(ctx.plm_get_x(dt), L, q)
    x[:L * q] += np.random.default_rng(seed).normal(0, 0.3, L * q).astype(dt)
    ctx.plm_set_x(x)
    return ctx, ctx.plm_get_x(dt)


def mf_context(X, q, pc=0.5):
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.mf_corr_mat(pc, want=False)
    J = ctx.mf_couplings()
    return ctx, J, ctx.mf_fields()


def check_against_ref(out, h, Jp, X, tol=1e-12):
    pll, site, cond = out
    rp, rs, rc, umax = conditionals_ref(h, Jp, X)
    n, L = X.shape
    assert pll.shape == (n,) and site.shape == (n, L) and cond.shape == (n, L, h.shape[1])
    s = umax[:, None]
    assert (np.abs(site - rs) / s).max() <= tol
    assert (np.abs(cond - rc) / s[:, :, None]).max() <= tol
    assert (np.abs(pll - rp) / umax).max() <= tol * 10
    # the PLL is the ascending-i sum of the site values, in the same order: the same bits
    assert np.array_equal(np.cumsum(site, axis=1)[:, -1].view(np.uint64), pll.view(np.uint64))
    assert np.array_equal(site, cond[np.arange(n)[:, None], np.arange(L)[None, :], X.astype(np.int64)])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("tag,prec", [("plm_toy_rna", _lib.DCA_F32), ("plm_toy_rna", _lib.DCA_F64),
                                      ("plm_toy_protein", _lib.DCA_F32), ("plm_toy_protein", _lib.DCA_F64)])
def test_plm_matches_restatement(tag, prec):
    G = golden(tag)
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    ctx, x = plm_context(X, q, prec, 1)
    h, Jp = plm_model(x, L, q)
    check_against_ref(ctx.plm_pseudo_likelihood(X, per_site=True, conditionals=True), h, Jp, X)
    pll = ctx.plm_pseudo_likelihood(X)
    assert isinstance(pll, np.ndarray) and pll.dtype == np.float64
    p2, site = ctx.plm_pseudo_likelihood(X, per_site=True)
    p3, cond = ctx.plm_pseudo_likelihood(X, conditionals=True)
    assert np.array_equal(bits(pll), bits(p2)) and np.array_equal(bits(pll), bits(p3))
    assert site.shape == (X.shape[0], L) and cond.shape == (X.shape[0], L, q)
    ctx.close()


@pytest.mark.parametrize("tag", ["mf_toy_rna", "mf_toy_protein"])
def test_mf_matches_restatement(tag):
    G = golden(tag)
    X, q = (G["X"] - 1).astype(np.uint8), int(G["q"])
    L = X.shape[1]
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    with pytest.raises(_lib.DcaBackendError) as ei:              # before the couplings exist
        ctx.mf_pseudo_likelihood(X)
    assert ei.value.code == _lib.DCA_ERR_STATE
    ctx.mf_corr_mat(0.5, want=False)
    J = ctx.mf_couplings()
    h, Jp = mf_model(J, ctx.mf_fields(), L, q)
    check_against_ref(ctx.mf_pseudo_likelihood(X, per_site=True, conditionals=True), h, Jp, X)
    ctx.close()


@pytest.mark.parametrize("q,prec", [(5, _lib.DCA_F32), (21, _lib.DCA_F64)])
def test_random_models_match_restatement(q, prec):
    rng = np.random.default_rng(q)
    L = 13
    ctx = _lib.Context(0, prec)
    ctx.set_msa(rng.integers(0, q, size=(20, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, prec)
    ctx.plm_configure(1.0, 1.0)
    dt = np.float64 if prec == _lib.DCA_F64 else np.float32
    x = rng.normal(0, 0.7, ctx.num_params()).astype(dt)
    ctx.plm_set_x(x)
    Q = rng.integers(0, q, size=(300, L), dtype=np.uint8)
    h, Jp = plm_model(x, L, q)
    check_against_ref(ctx.plm_pseudo_likelihood(Q, per_site=True, conditionals=True), h, Jp, Q)
    ctx.close()


# ---------------------------------------------------------------- 2. the plm objective
def test_objective_identity(oracle_plm):
    G = golden("plm_toy_protein")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.plm_configure(0.5, 0.5, carry_mode=_lib.CARRY_EXACT, add_regulariser=0)
    ctx.plm_init_x()
    x = perturbed(ctx.plm_get_x(np.float64), L, q)
    x[:L * q] += np.random.default_rng(4).normal(0, 0.3, L * q)
    ctx.plm_set_x(x)
    w = ctx.weights()
    target = -float(np.dot(w, ctx.plm_pseudo_likelihood(X)))
    fx = ctx.plm_gradient()
    assert abs(fx - target) <= 1e-11 * abs(target), (fx, target)
    fo, _g = oracle_plm.gradient(X, w, q, 0.0, 0.0, x, carry=False)
    assert abs(fo - target) <= 1e-11 * abs(target), (fo, target)
    ctx.close()


# ---------------------------------------------------------------- 3. the mutation scan
def test_conditionals_agree_with_the_scan():
    G = golden("plm_toy_protein")
    X, q = G["X"], int(G["q"])
    for prec in (_lib.DCA_F32, _lib.DCA_F64):
        ctx, _x = plm_context(X, q, prec, 3)
        w = X[5]
        _p, cond = ctx.plm_pseudo_likelihood(w[None, :], conditionals=True)
        dE = ctx.plm_mutation_scan(w)
        ref = dE - np.log(np.exp(dE - dE.max(1, keepdims=True)).sum(1, keepdims=True)) - dE.max(1, keepdims=True)
        assert np.abs(cond[0] - ref).max() <= 1e-12 * max(1.0, np.abs(dE).max())
        ctx.close()
    M = golden("mf_toy_protein")
    Xm = (M["X"] - 1).astype(np.uint8)
    mctx, _J, _f = mf_context(Xm, 21)
    w = Xm[2]
    _p, cond = mctx.mf_pseudo_likelihood(w[None, :], conditionals=True)
    dE = mctx.mf_mutation_scan(w)
    ref = dE - np.log(np.exp(dE - dE.max(1, keepdims=True)).sum(1, keepdims=True)) - dE.max(1, keepdims=True)
    assert np.abs(cond[0] - ref).max() <= 1e-12 * max(1.0, np.abs(dE).max())
    mctx.close()


# ---------------------------------------------------------------- 4. bitwise invariance
def test_bitwise_invariance_positions_repeats_and_passes(monkeypatch):
    G = golden("plm_rf71")
    X, q = G["X"], int(G["q"])
    ctx, _x = plm_context(X, q, _lib.DCA_F32, 2)
    target = X[7]
    alone = ctx.plm_pseudo_likelihood(target[None, :], per_site=True, conditionals=True)
    B = X[np.random.default_rng(0).integers(0, X.shape[0], 1500)]            # duplicates included
    for pos in (0, 700, 1499):
        Bp = B.copy()
        Bp[pos] = target
        out = ctx.plm_pseudo_likelihood(Bp, per_site=True, conditionals=True)
        for a, b in zip(out, alone):
            assert a[pos].tobytes() == b[0].tobytes(), pos
    one = ctx.plm_pseudo_likelihood(B, per_site=True, conditionals=True)
    two = ctx.plm_pseudo_likelihood(B, per_site=True, conditionals=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    monkeypatch.setenv("DCA_PLL_PASS", "512")                               # 1500 queries in three passes
    for kw in (dict(), dict(per_site=True, conditionals=True)):
        split = ctx.plm_pseudo_likelihood(B, **kw)
        split = split if isinstance(split, tuple) else (split,)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(split, one))
    ctx.close()


# ---------------------------------------------------------------- 5. shapes
# ... and the edges of the accumulator count QM (8 for q <= 8, 24 for q <= 24, else 32) and of its chunks: (17, 8) 16 blocks per
# chunk and one into a second chunk, (19, 9) the first q of QM = 24, (8, 24) q = QM, (7, 25) the first q of QM = 32, (5, 32)
# q = QM = 32.  The plm engine holds models of q = 5 and q = 21 only, so these five reach the site kernel through the
# mean-field source, which is float64: no entry of the library feeds it a float32 model of another q.
@pytest.mark.parametrize("L,q,prec", [(2, 5, _lib.DCA_F32), (2, 21, _lib.DCA_F64), (7, 21, _lib.DCA_F32), (67, 5, _lib.DCA_F64),
                                      (700, 5, _lib.DCA_F32), (17, 8, _lib.DCA_F64), (19, 9, _lib.DCA_F64), (8, 24, _lib.DCA_F64),
                                      (7, 25, _lib.DCA_F64), (5, 32, _lib.DCA_F64)])
def test_edge_shapes(L, q, prec):
    rng = np.random.default_rng(L * q)
    if q in (5, 21):
        ctx, x = plm_context(rng.integers(0, q, size=(16, L), dtype=np.uint8), q, prec, L)
        h, Jp = plm_model(x, L, q)
        entry = ctx.plm_pseudo_likelihood
    else:
        ctx, J, fields = mf_context(rng.integers(0, q, size=(64, L), dtype=np.uint8), q)
        h, Jp = mf_model(J, fields, L, q)
        entry = ctx.mf_pseudo_likelihood
    Q = rng.integers(0, q, size=(600, L), dtype=np.uint8)
    pll, site, cond = entry(Q, per_site=True, conditionals=True)
    idx = np.arange(0, 600, 7 if L > 100 else 1)
    check_against_ref((pll[idx], site[idx], cond[idx]), h, Jp, Q[idx])
    assert entry(Q[:0]).shape == (0,)
    ctx.close()


def test_config_d_size_model():
    """L = 500, q = 21, float32, random x, a few thousand queries spot-checked."""
    rng = np.random.default_rng(5)
    L, q = 500, 21
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(rng.integers(0, q, size=(32, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    x = rng.normal(0, 0.05, ctx.num_params()).astype(np.float32)
    ctx.plm_set_x(x)
    Q = rng.integers(0, q, size=(3000, L), dtype=np.uint8)
    pll, site = ctx.plm_pseudo_likelihood(Q, per_site=True)
    h, Jp = plm_model(x, L, q)
    idx = np.array([0, 1, 511, 512, 1777, 2999])
    _p, _s, cond = ctx.plm_pseudo_likelihood(Q[idx], per_site=True, conditionals=True)
    check_against_ref((pll[idx], site[idx], cond), h, Jp, Q[idx])
    ctx.close()


# ---------------------------------------------------------------- 6. untouched state
def test_training_state_untouched_and_refined_model():
    G = golden("plm_toy_protein")
    X, q = G["X"], int(G["q"])
    ctx, _x = plm_context(X, q, _lib.DCA_F32, 6)
    x0, g0 = ctx.plm_get_x(np.float32), ctx.plm_get_g(np.float32)
    s0 = ctx.plm_scores(True)
    ctx.plm_pseudo_likelihood(X, per_site=True, conditionals=True)
    assert np.array_equal(bits(ctx.plm_get_x(np.float32).astype(np.float64)), bits(x0.astype(np.float64)))
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert np.array_equal(bits(ctx.plm_scores(True)), bits(s0))
    fx0 = ctx.plm_gradient()
    ctx.plm_pseudo_likelihood(X)
    assert ctx.plm_gradient() == fx0
    # during an L-BFGS run
    ctx.plm_lbfgs_begin(20)
    ctx.plm_lbfgs_iterate(2)
    xr = ctx.plm_get_x(np.float32)
    h, Jp = plm_model(xr, X.shape[1], q)
    check_against_ref(ctx.plm_pseudo_likelihood(X[:40], per_site=True, conditionals=True), h, Jp, X[:40])
    ctx.plm_lbfgs_iterate(1)
    ctx.plm_lbfgs_end()
    ctx.close()
    M = golden("mf_toy_protein")
    Xm = (M["X"] - 1).astype(np.uint8)
    mctx, _J, _f = mf_context(Xm, 21)
    m0 = mctx.mf_scores(True)
    mctx.mf_pseudo_likelihood(Xm, per_site=True, conditionals=True)
    assert np.array_equal(bits(mctx.mf_scores(True)), bits(m0))
    mctx.close()
    # after fit_boltzmann the class scores the refined x
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    before = inst.compute_sequence_pseudo_log_likelihoods()
    fit = inst.fit_boltzmann(iterations=3, num_chains=64, sweeps_per_iteration=2, equilibration_sweeps=5)
    after = inst.compute_sequence_pseudo_log_likelihoods()
    X_r = _lib.encode_sequences(fasta_reader.get_alignment_from_fasta_file(path), _lib.DCA_BIOMOLECULE_RNA, 10, 0)
    h, Jp = plm_model(fit["fields_and_couplings"], 10, 5)
    rp, _rs, _rc, umax = conditionals_ref(h, Jp, X_r)
    assert (np.abs(after - rp) / umax).max() <= 1e-11
    assert not np.array_equal(before, after)


# ---------------------------------------------------------------- 7. errors and profiling
def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    with pytest.raises(_lib.DcaBackendError) as ei:               # not configured yet
        ctx.plm_pseudo_likelihood(X)
    assert ei.value.code == _lib.DCA_ERR_STATE
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_init_x()
    bad = X[:2].copy()
    bad[1, 3] = q
    with pytest.raises(_lib.DcaBackendError) as ei:
        ctx.plm_pseudo_likelihood(bad, conditionals=True)
    assert ei.value.code == _lib.DCA_ERR_ARG
    assert ctx.plm_pseudo_likelihood(X[:0], per_site=True, conditionals=True)[2].shape == (0, X.shape[1], q)
    ctx.set_profiling(True)
    ctx.plm_pseudo_likelihood(X)
    ctx.plm_pseudo_likelihood(X, per_site=True)
    assert ctx.kernel_time("pll")[1] == 2
    ctx.close()


# ---------------------------------------------------------------- 8. classes and command lines
def _parse_rows(path):
    return [ln.split() for ln in open(path).read().splitlines() if not ln.startswith("#")]


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    pll, site = inst.compute_sequence_pseudo_log_likelihoods(per_site=True)
    assert pll.shape == (len(seqs),) and site.shape == (len(seqs), 10)
    assert np.array_equal(inst.compute_sequence_pseudo_log_likelihoods(seqs[:3]), pll[:3])
    cond = inst.compute_conditional_log_probabilities(seqs[0])
    assert cond.shape == (10, 5)
    assert inst.compute_conditional_log_probabilities(seqs[:2]).shape == (2, 10, 5)
    ctx = inst._fitted_context()
    Xa = _lib.read_msa(path, _lib.DCA_BIOMOLECULE_RNA, 10)[0]
    ref = float(np.dot(ctx.weights(), ctx.plm_pseudo_likelihood(Xa))) / ctx.meff()
    assert inst.compute_pseudo_log_likelihood() == pytest.approx(ref, rel=1e-14)
    with pytest.raises(PlmDCAException, match="record 2"):
        inst.compute_sequence_pseudo_log_likelihoods([seqs[0], "AC1GUACGUA"])
    out = str(tmp_path / "plm_out")
    f = plmdca_main.run_plm_dca(["compute_pseudo_log_likelihood", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8",
                                 "--max_iterations", "5", "--output_dir", out])
    assert os.path.basename(f) == "PLMDCA_pseudo_log_likelihoods_toy_rna.txt"
    rows = _parse_rows(f)
    assert [int(r[0]) for r in rows] == list(range(1, len(seqs) + 1))
    assert np.allclose([float(r[1]) for r in rows], pll, rtol=1e-6, atol=1e-6)
    assert any("Weighted pseudo-log-likelihood" in ln for ln in open(f))
    multi = PlmDCA(path, "rna", devices=[0, 1])
    with pytest.raises(PlmDCAException, match="one GPU"):
        multi.compute_pseudo_log_likelihood()


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    pll = inst.compute_sequence_pseudo_log_likelihoods()
    L = inst.sequences_len
    h, Jp = mf_model(inst.get_couplings(), np.array([v for _k, v in sorted(inst.compute_fields().items())]), L, 21)
    X = _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_PROTEIN, L, 1)
    rp, _rs, rc, umax = conditionals_ref(h, Jp, X)
    assert (np.abs(pll - rp) / umax).max() <= 1e-10
    cond = inst.compute_conditional_log_probabilities(seqs[2])
    assert cond.shape == (L, 21)
    assert (np.abs(cond - rc[2]) / umax[2]).max() <= 1e-10
    X0 = (np.array(inst.alignment, dtype=np.int64) - 1).astype(np.uint8)     # the instance's own alignment (codes from 0)
    ref = float(np.dot(inst.sequences_weight, conditionals_ref(h, Jp, X0)[0])) / inst.effective_num_sequences
    assert inst.compute_pseudo_log_likelihood() == pytest.approx(ref, rel=1e-9)
    with pytest.raises(MeanFieldDCAException, match="record 2"):
        inst.compute_sequence_pseudo_log_likelihoods([seqs[0], seqs[1][:-1]])
    out = str(tmp_path / "mf_out")
    f = mfdca_main.run_meanfield_dca(["compute_pseudo_log_likelihood", "protein", path, "--output_dir", out, "--query_file", path])
    assert os.path.basename(f) == "MFDCA_pseudo_log_likelihoods_toy_protein.txt"
    rows = _parse_rows(f)
    assert len(rows) == len(seqs)
    assert np.allclose([float(r[1]) for r in rows], pll, rtol=1e-12, atol=1e-12)
    assert not any("Weighted pseudo-log-likelihood" in ln for ln in open(f))
