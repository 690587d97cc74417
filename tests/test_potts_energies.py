"""Potts energies and single-mutant scans on the GPU (dca_plm_energies / _mutation_scan, dca_mf_energies / _mutation_scan,
the class methods and the command lines), checked against a float64 numpy restatement kept in this file."""
import os

import numpy as np
import pytest

from conftest import data_file, golden, perturbed
from pydca_amd import _lib, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- numpy float64 restatement
def _terms(h, J, X):
    """h: L x q, J: pairs x q x q (pair order (0,1),(0,2)...), X: n x L -> (energies, sum of |terms|) in float64."""
    L = h.shape[0]
    iu, ju = np.triu_indices(L, 1)
    p = np.arange(iu.size)
    E = np.empty(X.shape[0])
    S = np.empty(X.shape[0])
    for a in range(0, X.shape[0], 64):
        x = X[a:a + 64].astype(np.int64)
        hf = h[np.arange(L)[None, :], x]
        jt = J[p[None, :], x[:, iu], x[:, ju]]
        E[a:a + 64] = hf.sum(1) + jt.sum(1)
        S[a:a + 64] = np.abs(hf).sum(1) + np.abs(jt).sum(1)
    return E, S


def plm_model(x, L, q):
    x = np.asarray(x, dtype=np.float64)
    return x[:L * q].reshape(L, q), x[L * q:].reshape(-1, q, q)


def mf_model(J, fields, L, q):
    """Dense -inv(C) (L(q-1) square) and fields (L x (q-1)) -> h, J with zero gap rows / columns."""
    qm = q - 1
    h = np.zeros((L, q))
    h[:, :qm] = fields
    J4 = np.asarray(J).reshape(L, qm, L, qm)
    iu, ju = np.triu_indices(L, 1)
    Jp = np.zeros((iu.size, q, q))
    Jp[:, :qm, :qm] = J4[iu, :, ju, :]
    return h, Jp


def mutation_ref(h, Jp, w):
    L, q = h.shape
    iu, ju = np.triu_indices(L, 1)
    pidx = np.full((L, L), -1)
    pidx[iu, ju] = np.arange(iu.size)
    dE = np.zeros((L, q))
    for i in range(L):
        s = np.zeros(q)
        for j in range(L):
            if j > i:
                s += Jp[pidx[i, j], :, w[j]]
            elif j < i:
                s += Jp[pidx[j, i], w[j], :]
        dE[i] = (h[i] - h[i, w[i]]) + (s - s[w[i]])
    return dE


def assert_rel(E, ref, scale, tol):
    err = np.abs(E - ref) / np.maximum(scale, 1e-300)
    assert err.max() <= tol, (err.max(), tol)


# ---------------------------------------------------------------- helpers
def plm_context(X, q, precision, seed, lh=1.0, lJ=1.0):
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, precision)
    ctx.plm_configure(lh, lJ)
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


GOLDEN_PLM = [("plm_toy_rna", _lib.DCA_F32), ("plm_toy_rna", _lib.DCA_F64), ("plm_toy_protein", _lib.DCA_F32),
              ("plm_toy_protein", _lib.DCA_F64), ("plm_rf71", _lib.DCA_F32)]


@pytest.mark.parametrize("tag,prec", GOLDEN_PLM)
def test_plm_energies_and_scan_match_restatement(tag, prec):
    G = golden(tag)
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    ctx, x = plm_context(X, q, prec, 1)
    h, Jp = plm_model(x, L, q)
    E = ctx.plm_energies(X)
    ref, scale = _terms(h, Jp, X)
    assert E.dtype == np.float64 and E.shape == (X.shape[0],)
    assert_rel(E, ref, scale, 1e-12)
    # mutation scan: restatement, explicit mutants scored by the energy entry, exact zeros at the wild type
    w = X[3]
    dE = ctx.plm_mutation_scan(w)
    assert dE.shape == (L, q)
    assert np.all(dE[np.arange(L), w] == 0.0)
    assert_rel(dE, mutation_ref(h, Jp, w), scale[3], 1e-12)
    if L <= 20:
        M = np.repeat(w[None, :], L * q, axis=0)
        M[np.arange(L * q), np.repeat(np.arange(L), q)] = np.tile(np.arange(q), L)
        Em = ctx.plm_energies(M).reshape(L, q) - ctx.plm_energies(w[None, :])[0]
        assert np.abs(Em - dE).max() <= 1e-9 * scale[3]
    ctx.close()


@pytest.mark.parametrize("tag", ["mf_toy_rna", "mf_toy_protein"])
def test_mf_energies_and_scan_match_restatement(tag):
    G = golden(tag)
    X, q = (G["X"] - 1).astype(np.uint8), int(G["q"])
    L = X.shape[1]
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    for call in (lambda: ctx.mf_energies(X), lambda: ctx.mf_mutation_scan(X[0])):
        with pytest.raises(_lib.DcaBackendError) as ei:       # before the couplings exist
            call()
        assert ei.value.code == _lib.DCA_ERR_STATE
    ctx.mf_corr_mat(0.5, want=False)
    J = ctx.mf_couplings()
    h, Jp = mf_model(J, ctx.mf_fields(), L, q)
    E = ctx.mf_energies(X)
    ref, scale = _terms(h, Jp, X)
    assert_rel(E, ref, scale, 1e-10)
    w = X[1]
    dE = ctx.mf_mutation_scan(w)
    assert np.all(dE[np.arange(L), w] == 0.0)
    assert_rel(dE, mutation_ref(h, Jp, w), scale[1], 1e-10)
    M = np.repeat(w[None, :], L * q, axis=0)
    M[np.arange(L * q), np.repeat(np.arange(L), q)] = np.tile(np.arange(q), L)
    Em = ctx.mf_energies(M).reshape(L, q) - ctx.mf_energies(w[None, :])[0]
    assert np.abs(Em - dE).max() <= 1e-9 * scale[1]
    ctx.close()


@pytest.mark.parametrize("q", [5, 21])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_edge_shapes_and_batch_invariance(q, prec):
    rng = np.random.default_rng(q + prec)
    for L in (2, 3, 9, 65, 130):
        Xt = rng.integers(0, q, size=(40, L), dtype=np.uint8)
        ctx, x = plm_context(Xt, q, prec, L)
        h, Jp = plm_model(x, L, q)
        Q = rng.integers(0, q, size=(1025, L), dtype=np.uint8)
        full = ctx.plm_energies(Q)
        ref, scale = _terms(h, Jp, Q)
        assert_rel(full, ref, scale, 1e-12)
        for n in (1, 63, 64, 65):
            part = ctx.plm_energies(Q[-n:])
            assert np.array_equal(part.view(np.uint64), full[-n:].view(np.uint64)), (L, n)
        assert ctx.plm_energies(Q[:0]).shape == (0,)
        ctx.close()


def test_config_d_size_model():
    """L = 500, q = 21, float32, random x: the tiles span many groups."""
    rng = np.random.default_rng(5)
    L, q = 500, 21
    Xt = rng.integers(0, q, size=(32, L), dtype=np.uint8)
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(Xt, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    x = rng.normal(0, 0.05, ctx.num_params()).astype(np.float32)
    ctx.plm_set_x(x)
    Q = rng.integers(0, q, size=(2000, L), dtype=np.uint8)
    E = ctx.plm_energies(Q)
    h, Jp = plm_model(x, L, q)
    idx = np.arange(0, 2000, 50)                 # the restatement on a sample (every 50th) keeps the test short
    ref, scale = _terms(h, Jp, Q[idx])
    assert_rel(E[idx], ref, scale, 1e-12)
    assert np.array_equal(ctx.plm_energies(Q[idx]).view(np.uint64), E[idx].view(np.uint64))
    ctx.close()


def test_bitwise_invariance_and_training_state_untouched():
    G = golden("plm_rf71")
    X, q = G["X"], int(G["q"])
    ctx, _x = plm_context(X, q, _lib.DCA_F32, 2)
    s0 = ctx.plm_scores(True)
    fx0 = ctx.plm_gradient()
    target = X[7]
    alone = ctx.plm_energies(target[None, :])
    B = X[np.random.default_rng(0).integers(0, X.shape[0], 3000)]         # duplicates included
    for pos in (0, 1, 2999):
        Bp = B.copy()
        Bp[pos] = target
        E = ctx.plm_energies(Bp)
        assert E[pos].tobytes() == alone[0].tobytes(), pos
    E1, E2 = ctx.plm_energies(B), ctx.plm_energies(B)
    assert E1.tobytes() == E2.tobytes()
    assert np.array_equal(ctx.plm_scores(True).view(np.uint64), s0.view(np.uint64))
    assert ctx.plm_gradient() == fx0
    ctx.close()
    M = golden("mf_toy_protein")
    mctx, _J, _f = mf_context((M["X"] - 1).astype(np.uint8), 21)
    m0 = mctx.mf_scores(True)
    mctx.mf_energies((M["X"] - 1).astype(np.uint8))
    mctx.mf_mutation_scan((M["X"][0] - 1).astype(np.uint8))
    assert np.array_equal(mctx.mf_scores(True).view(np.uint64), m0.view(np.uint64))
    mctx.close()


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    with pytest.raises(_lib.DcaBackendError) as ei:               # no configured parameters yet
        ctx.plm_energies(X)
    assert ei.value.code == _lib.DCA_ERR_STATE
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_init_x()
    bad = X[:2].copy()
    bad[1, 3] = q
    with pytest.raises(_lib.DcaBackendError) as ei:
        ctx.plm_energies(bad)
    assert ei.value.code == _lib.DCA_ERR_ARG
    with pytest.raises(_lib.DcaBackendError) as ei:
        ctx.plm_mutation_scan(bad[1])
    assert ei.value.code == _lib.DCA_ERR_ARG
    ctx.set_profiling(True)
    ctx.plm_energies(X)
    ctx.plm_mutation_scan(X[0])
    assert ctx.kernel_time("energies")[1] >= 1 and ctx.kernel_time("mutation_scan")[1] >= 1
    ctx.close()


# ---------------------------------------------------------------- classes and command lines
def _records_with(path, tmp_path, bad_index, bad_seq):
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    seqs[bad_index] = bad_seq
    out = tmp_path / "bad.fa"
    out.write_text("".join(">r{}\n{}\n".format(k, s) for k, s in enumerate(seqs)))
    return str(out)


def _parse_rows(path):
    return [ln.split() for ln in open(path).read().splitlines() if not ln.startswith("#")]


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    n_rec = len(fasta_reader.get_alignment_from_fasta_file(path))
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    E = inst.compute_sequence_energies()
    assert E.shape == (n_rec,) and np.all(np.isfinite(E))
    assert np.array_equal(inst.compute_sequence_energies(path), E)                    # the model held is reused
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    assert np.array_equal(inst.compute_sequence_energies(seqs[:3]), E[:3])
    dE = inst.compute_single_mutant_effects(seqs[0])
    assert dE.shape == (10, 5)
    assert len(inst.compute_sorted_FN()) == 45
    with pytest.raises(PlmDCAException, match="record 4"):
        inst.compute_sequence_energies(_records_with(path, tmp_path, 3, "ACG"))
    with pytest.raises(PlmDCAException, match="record 2"):
        inst.compute_sequence_energies([seqs[0], "AC1GUACGUA"])
    out = str(tmp_path / "plm_out")
    f = plmdca_main.execute_from_command_line("rna", path, the_command="compute_energies", lambda_h=1.8, lambda_J=1.8,
                                              max_iterations=5, output_dir=out)
    assert os.path.basename(f) == "PLMDCA_energies_toy_rna.txt"
    rows = _parse_rows(f)
    assert [int(r[0]) for r in rows] == list(range(1, n_rec + 1))
    assert np.allclose([float(r[1]) for r in rows], E, rtol=1e-6, atol=1e-6)
    wt = tmp_path / "wt.fa"
    wt.write_text(">wt\n{}\n".format(seqs[0]))
    f = plmdca_main.run_plm_dca(["compute_mutation_effects", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8",
                                 "--max_iterations", "5", "--output_dir", out, "--wildtype_file", str(wt)])
    assert os.path.basename(f) == "PLMDCA_mutation_effects_toy_rna.txt"
    rows = _parse_rows(f)
    assert len(rows) == 10 * 5
    assert [r[1] for r in rows[:5]] == [seqs[0][0].upper()] * 5 and [r[2] for r in rows[:5]] == list("ACGU-")
    assert np.allclose(np.array([float(r[3]) for r in rows]).reshape(10, 5), dE, rtol=1e-6, atol=1e-6)


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    E = inst.compute_sequence_energies()                     # the couplings are computed here
    assert E.shape == (len(seqs),)
    L = inst.sequences_len
    h, Jp = mf_model(inst.get_couplings(), np.array([v for _k, v in sorted(inst.compute_fields().items())]), L, 21)
    X = _lib.encode_sequences(seqs, _lib.DCA_BIOMOLECULE_PROTEIN, L, 1)
    ref, scale = _terms(h, Jp, X)
    assert_rel(E, ref, scale, 1e-10)
    dE = inst.compute_single_mutant_effects(seqs[2])
    assert dE.shape == (L, 21)
    assert len(inst.compute_sorted_FN()) == L * (L - 1) // 2
    with pytest.raises(MeanFieldDCAException, match="record 2"):
        inst.compute_sequence_energies([seqs[0], seqs[1][:-1]])
    out = str(tmp_path / "mf_out")
    f = mfdca_main.execute_from_command_line(path, "protein", the_command="compute_energies", output_dir=out,
                                             query_file=path)
    assert os.path.basename(f) == "MFDCA_energies_toy_protein.txt"
    rows = _parse_rows(f)
    assert len(rows) == len(seqs)
    assert np.allclose([float(r[1]) for r in rows], E, rtol=1e-12, atol=1e-12)
    wt = tmp_path / "wt.fa"
    wt.write_text(">wt\n{}\n".format(seqs[2]))
    f = mfdca_main.run_meanfield_dca(["compute_mutation_effects", "protein", path, "--output_dir", out, "--wildtype_file", str(wt)])
    assert os.path.basename(f) == "MFDCA_mutation_effects_toy_protein.txt"
    rows = _parse_rows(f)
    assert len(rows) == L * 21
    assert np.allclose(np.array([float(r[3]) for r in rows]).reshape(L, 21), dE, rtol=1e-12, atol=1e-12)
