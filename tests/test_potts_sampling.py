"""Gibbs sampling on the GPU (dca_plm_sample, dca_mf_sample, the class methods and the command lines), checked against a
float64 numpy restatement kept in this file: the same Philox4x32-10 stream, the same draw rule, the model read back from
plm_get_x or mf_couplings + mf_fields."""
import math
import os

import numpy as np
import pytest

from conftest import data_file, golden
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from test_potts_sampling_host import philox_np

pytestmark = pytest.mark.gpu

MARGIN = [np.inf]          # smallest |cumsum - r| / T the restatement met (every test checks its own draws against 1e-12)


# ---------------------------------------------------------------- numpy float64 restatement
def plm_model(x, L, q):
    x = np.asarray(x, dtype=np.float64)
    return x[:L * q].reshape(L, q), x[L * q:].reshape(-1, q, q)


def mf_model(J, fields, L, q):
    qm = q - 1
    h = np.zeros((L, q))
    h[:, :qm] = fields
    J4 = np.asarray(J).reshape(L, qm, L, qm)
    iu, ju = np.triu_indices(L, 1)
    Jp = np.zeros((iu.size, q, q))
    Jp[:, :qm, :qm] = J4[iu, :, ju, :]
    return h, Jp


def uniforms(seed, chains, sweep, site, tag):
    ctr = np.zeros((len(chains), 4), dtype=np.uint64)
    ctr[:, 0] = np.asarray(chains, dtype=np.uint64) & np.uint64(0xffffffff)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = sweep & 0xffffffff, site, tag
    w = philox_np(ctr, (seed & 0xffffffff, seed >> 32))
    return ((w[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[:, 1] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


def random_start(seed, chains, L, q):
    return np.stack([np.floor(uniforms(seed, chains, 0, i, 1) * q).astype(np.uint8) for i in range(L)], axis=1)


def gibbs_ref(h, Jp, beta, seed, chains, first_sweep, sweeps, X0):
    """Systematic-scan Gibbs in float64; returns the final codes and the smallest relative margin of the draws."""
    L, q = h.shape
    iu, ju = np.triu_indices(L, 1)
    pidx = np.zeros((L, L), dtype=np.int64)
    pidx[iu, ju] = np.arange(iu.size)
    pidx[ju, iu] = np.arange(iu.size)
    S = X0.astype(np.int64).copy()
    n = S.shape[0]
    rows = np.arange(n)
    margin = np.inf
    for t in range(sweeps):
        for i in range(L):
            Jrow = Jp[pidx[i]].copy()                                  # L x q x q, block (min, max)
            Jrow[:i] = Jrow[:i].transpose(0, 2, 1)                   # j < i: J(a, b) = block(j, i)[b, a]
            Jrow[i] = 0.0
            u = h[i][None, :] + Jrow[np.arange(L)[None, :], :, S].sum(axis=1)          # n x q
            p = np.exp(beta * (u - u.max(axis=1, keepdims=True)))
            cum = np.cumsum(p, axis=1)
            T = cum[:, -1]
            r = uniforms(seed, chains, first_sweep + t, i, 0) * T
            above = cum > r[:, None]
            pick = np.where(above.any(axis=1), above.argmax(axis=1), q - 1 - np.argmax((p > 0)[:, ::-1], axis=1))
            margin = min(margin, float((np.abs(cum - r[:, None]) / T[:, None]).min()))
            S[rows, i] = pick
    MARGIN[0] = min(MARGIN[0], margin)
    return S.astype(np.uint8), margin


# ---------------------------------------------------------------- helpers
def plm_context(L, q, precision, seed, sigma=0.5, N=40):
    rng = np.random.default_rng(seed)
    ctx = _lib.Context(0, precision)
    ctx.set_msa(rng.integers(0, q, size=(N, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, precision)
    ctx.plm_configure(1.0, 1.0)
    dt = np.float64 if precision == _lib.DCA_F64 else np.float32
    ctx.plm_set_x(rng.normal(0, sigma, ctx.num_params()).astype(dt))
    h, Jp = plm_model(ctx.plm_get_x(dt), L, q)
    return ctx, h, Jp


def mf_context(tag="mf_toy_protein"):
    G = golden(tag)
    X, q = (G["X"] - 1).astype(np.uint8), int(G["q"])
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.mf_corr_mat(0.5, want=False)
    J = ctx.mf_couplings()
    h, Jp = mf_model(J, ctx.mf_fields(), X.shape[1], q)
    return ctx, h, Jp, X


def mf_random_context(L, q, seed, N=200):
    """an mf model of any alphabet: random columns, each with its own state frequencies"""
    rng = np.random.default_rng([seed, L, q])
    X = np.stack([rng.choice(q, size=N, p=rng.dirichlet(np.ones(q))).astype(np.uint8) for _ in range(L)], axis=1)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.mf_corr_mat(0.5, want=False)
    h, Jp = mf_model(ctx.mf_couplings(), ctx.mf_fields(), L, q)
    return ctx, h, Jp


# ---------------------------------------------------------------- 1. exact trajectories
@pytest.mark.parametrize("q,L", [(5, 23), (21, 37)])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_plm_trajectories_match_restatement(q, L, prec):
    ctx, h, Jp = plm_context(L, q, prec, 10 * q + prec)
    n = 300
    chains = np.arange(n)
    rng = np.random.default_rng(q)
    for beta, given in ((1.0, False), (0.5, True), (2.0, False)):
        X0 = rng.integers(0, q, size=(n, L), dtype=np.uint8) if given else None
        out = ctx.plm_sample(n, 5, seed=1234, beta=beta, initial=X0)
        start = X0 if given else random_start(1234, chains, L, q)
        ref, margin = gibbs_ref(h, Jp, beta, 1234, chains, 0, 5, start)
        assert margin > 1e-12, margin
        assert out.shape == (n, L) and out.dtype == np.uint8
        assert np.array_equal(out, ref), (beta, int((out != ref).sum()))
    ctx.close()


@pytest.mark.parametrize("tag", ["mf_toy_protein", "mf_toy_rna"])
def test_mf_trajectories_match_restatement(tag):
    ctx, h, Jp, X = mf_context(tag)
    L, q = h.shape
    n = 256
    chains = np.arange(7, 7 + n)
    for beta, X0 in ((1.0, None), (0.5, X[np.arange(n) % X.shape[0]]), (2.0, None)):
        out = ctx.mf_sample(n, 5, seed=99, beta=beta, initial=X0, first_chain=7, first_sweep=3)
        start = random_start(99, chains, L, q) if X0 is None else X0
        ref, margin = gibbs_ref(h, Jp, beta, 99, chains, 3, 5, start)
        assert margin > 1e-12, margin
        assert np.array_equal(out, ref), (beta, int((out != ref).sum()))
    ctx.close()


# ---------------------------------------------------------------- 2. the stationary distribution
def _chi2_sf(x, df):
    """Wilson-Hilferty upper tail of chi^2(df)."""
    z = ((x / df) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * df))) / math.sqrt(2.0 / (9.0 * df))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def _g_test(counts, expected):
    small = expected < 5.0                    # bins expecting fewer than 5 are pooled
    O = np.append(counts[~small], counts[small].sum())
    E = np.append(expected[~small], expected[small].sum())
    keep = E > 0
    O, E = O[keep], E[keep]
    G = 2.0 * np.sum(np.where(O > 0, O * np.log(np.maximum(O, 1) / E), 0.0))
    return _chi2_sf(G, O.size - 1)


def test_distribution_of_final_states():
    L, q = 4, 5
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F64, 77)
    states = np.array(np.unravel_index(np.arange(q ** L), (q,) * L)).T.astype(np.uint8)
    E = ctx.plm_energies(states)
    n = 200000
    for beta in (1.0, 0.5, 0.0):
        out = ctx.plm_sample(n, 30, seed=2024 + int(10 * beta), beta=beta)
        idx = np.ravel_multi_index(out.T.astype(np.int64), (q,) * L)
        counts = np.bincount(idx, minlength=q ** L).astype(np.float64)
        w = np.exp(beta * (E - E.max()))
        P = w / w.sum()
        p = _g_test(counts, n * P)
        assert p > 1e-6, (beta, p)
        mean, var = float(np.dot(P, E)), float(np.dot(P, (E - np.dot(P, E)) ** 2))
        if var > 0:
            assert abs(E[idx].mean() - mean) <= 5.0 * math.sqrt(var / n), beta
        if beta == 0.0:
            for i in range(L):
                assert _g_test(np.bincount(out[:, i], minlength=q).astype(np.float64), np.full(q, n / q)) > 1e-6
    ctx.close()


# ---------------------------------------------------------------- 3. bitwise invariances
def test_batch_split_and_continuation_invariance():
    ctx, _h, _Jp = plm_context(60, 21, _lib.DCA_F32, 5)
    n = 5000
    full = ctx.plm_sample(n, 3, seed=42)
    a = ctx.plm_sample(2000, 3, seed=42)
    b = ctx.plm_sample(n - 2000, 3, seed=42, first_chain=2000)
    assert np.array_equal(np.vstack([a, b]), full)
    for k in (0, 63, 64, 4999):
        assert np.array_equal(ctx.plm_sample(1, 3, seed=42, first_chain=k)[0], full[k]), k
    X0 = np.random.default_rng(1).integers(0, 21, size=(300, 60), dtype=np.uint8)
    ten = ctx.plm_sample(300, 10, seed=8, beta=0.7, initial=X0)
    four = ctx.plm_sample(300, 4, seed=8, beta=0.7, initial=X0)
    assert np.array_equal(ctx.plm_sample(300, 6, seed=8, beta=0.7, initial=four, first_sweep=4), ten)
    ctx.close()


# ---------------------------------------------------------------- 4. large shapes
@pytest.mark.parametrize("L,q", [(500, 21), (1200, 5)])
def test_large_shapes_match_restatement(L, q):
    """(500, 21): config D's size, many chunks of row i per site; (1200, 5): the chain codes beyond LDS, kept in global memory."""
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F32, L, sigma=0.05, N=16)
    n = 16
    out = ctx.plm_sample(n, 2, seed=3, beta=1.0)
    ref, margin = gibbs_ref(h, Jp, 1.0, 3, np.arange(n), 0, 2, random_start(3, np.arange(n), L, q))
    assert margin > 1e-12, margin
    assert np.array_equal(out, ref), int((out != ref).sum())
    ctx.close()


# ---------------------------------------------------------------- 5. state untouched, errors
def test_training_state_untouched():
    G = golden("plm_rf71")
    X, q = G["X"], int(G["q"])
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_init_x()
    ctx.plm_set_x(ctx.plm_get_x(np.float32) + np.random.default_rng(0).normal(0, 0.1, ctx.num_params()).astype(np.float32))
    fx0 = ctx.plm_gradient()
    x0, g0 = ctx.plm_get_x(np.float32), ctx.plm_get_g(np.float32)
    E0 = ctx.plm_energies(X[:50])
    ctx.plm_sample(500, 3, seed=1)
    assert ctx.plm_get_x(np.float32).tobytes() == x0.tobytes()
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.plm_energies(X[:50]).tobytes() == E0.tobytes()
    assert ctx.plm_gradient() == fx0
    ctx.close()
    mctx, _h, _Jp, MX = mf_context()
    J0 = mctx.mf_couplings()
    mctx.mf_sample(300, 3, seed=1)
    assert mctx.mf_couplings().tobytes() == J0.tobytes()
    mctx.close()


def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_sample(4, 1)) == _lib.DCA_ERR_STATE
    assert _code(lambda: ctx.mf_sample(4, 1)) == _lib.DCA_ERR_STATE
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_init_x()
    bad = X[:2].copy()
    bad[1, 3] = q
    for call in (lambda: ctx.plm_sample(-1, 1), lambda: ctx.plm_sample(2, -1), lambda: ctx.plm_sample(2, 1, beta=-0.5),
                 lambda: ctx.plm_sample(2, 1, beta=float("nan")), lambda: ctx.plm_sample(2, 1, initial=bad)):
        assert _code(call) == _lib.DCA_ERR_ARG
    lib = _lib.lib()
    assert lib.dca_plm_sample(ctx._h, 2, 1, 0, 0, 0, 1.0, None, None) == _lib.DCA_ERR_ARG
    assert lib.dca_plm_sample(ctx._h, 0, 1, 0, 0, 0, 1.0, None, None) == _lib.DCA_OK
    assert ctx.plm_sample(0, 3).shape == (0, L)
    assert np.array_equal(ctx.plm_sample(2, 0, initial=X[:2]), X[:2])                 # sweeps = 0: the start
    assert np.array_equal(ctx.plm_sample(70, 0, seed=5, first_chain=3), random_start(5, np.arange(3, 73), L, q))
    ctx.set_profiling(True)
    ctx.plm_sample(8, 3)
    assert ctx.kernel_time("sample")[1] == 3
    ctx.close()
    mctx, _h, _Jp, MX = mf_context("mf_toy_rna")
    bad = MX[:2].copy()
    bad[0, 0] = 5
    assert _code(lambda: mctx.mf_sample(2, 1, initial=bad)) == _lib.DCA_ERR_ARG
    assert _code(lambda: mctx.mf_sample(2, 1, beta=-1.0)) == _lib.DCA_ERR_ARG
    assert mctx.mf_sample(0, 1).shape == (0, MX.shape[1])
    mctx.close()
    assert MARGIN[0] > 1e-12


# ---------------------------------------------------------------- 6. classes and command lines
def _read_samples(path):
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    heads = [ln for ln in open(path).read().splitlines() if ln.startswith(">")]
    assert [h.split()[0] for h in heads] == [">sample_%d" % (k + 1) for k in range(len(heads))]
    return seqs, np.array([float(h.split("energy=")[1]) for h in heads])


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    S = inst.sample_sequences(40, num_sweeps=20, seed=4)
    assert len(S) == 40 and all(len(s) == 10 and set(s) <= set("ACGU-") for s in S)
    assert inst.sample_sequences(40, num_sweeps=20, seed=4) == S
    codes = inst.sample_sequences(40, num_sweeps=20, seed=4, return_codes=True)
    assert codes.shape == (40, 10) and ["".join("ACGU-"[c] for c in row) for row in codes] == S
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    start = "".join("ACGU-"[c] for c in _lib.encode_sequences([seqs[0]], _lib.DCA_BIOMOLECULE_RNA, 10, 0)[0])
    assert inst.sample_sequences(3, num_sweeps=0, initial=seqs[0]) == [start] * 3
    with pytest.raises(PlmDCAException, match="record 2"):
        inst.sample_sequences(2, initial=[seqs[0], "AC1GUACGUA"])
    with pytest.raises(PlmDCAException):
        inst.sample_sequences(2, temperature=0.0)
    out = str(tmp_path / "plm_out")
    f = _potts.run_subcommand(inst, "sample_sequences", "PLMDCA", path, out, None, _lib.DCA_BIOMOLECULE_RNA, 0, PlmDCAException,
                              sampling={"num_sequences": 25, "num_sweeps": 10, "seed": 2})
    got, E = _read_samples(f)
    assert got == inst.sample_sequences(25, num_sweeps=10, seed=2)
    assert inst.compute_sequence_energies(got).tobytes() == E.tobytes()
    f = plmdca_main.run_plm_dca(["sample_sequences", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                 "--output_dir", out, "--num_sequences", "12", "--num_sweeps", "5", "--temperature", "2"])
    assert os.path.basename(f) == "PLMDCA_samples_toy_rna.fa"
    got, E = _read_samples(f)
    assert len(got) == 12 and np.all(np.isfinite(E))


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    S = inst.sample_sequences(30, num_sweeps=15, seed=9)                  # the couplings are computed here
    L = inst.sequences_len
    assert len(S) == 30 and all(len(s) == L and set(s) <= set(_potts.state_letters(_lib.DCA_BIOMOLECULE_PROTEIN)) for s in S)
    wt = tmp_path / "start.fa"
    wt.write_text(">s\n{}\n".format(seqs[1]))
    letters = _potts.state_letters(_lib.DCA_BIOMOLECULE_PROTEIN)
    start = "".join(letters[c] for c in _lib.encode_sequences([seqs[1]], _lib.DCA_BIOMOLECULE_PROTEIN, L, 1)[0])
    assert inst.sample_sequences(2, num_sweeps=0, initial=str(wt)) == [start] * 2
    with pytest.raises(MeanFieldDCAException, match="records"):
        inst.sample_sequences(3, initial=seqs[:2])
    out = str(tmp_path / "mf_out")
    f = _potts.run_subcommand(inst, "sample_sequences", "MFDCA", path, out, None, _lib.DCA_BIOMOLECULE_PROTEIN, 1,
                              MeanFieldDCAException, sampling={"num_sequences": 20, "num_sweeps": 8, "seed": 1})
    got, E = _read_samples(f)
    assert got == inst.sample_sequences(20, num_sweeps=8, seed=1)
    assert inst.compute_sequence_energies(got).tobytes() == E.tobytes()
    f = mfdca_main.run_meanfield_dca(["sample_sequences", "protein", path, "--output_dir", out, "--num_sequences", "6",
                                      "--num_sweeps", "4", "--initial_file", str(wt)])
    assert os.path.basename(f) == "MFDCA_samples_toy_protein.fa"
    got, E = _read_samples(f)
    assert len(got) == 6 and all(len(s) == L for s in got)
    assert np.allclose(E, MeanFieldDCA(path, "protein").compute_sequence_energies(got), rtol=1e-12, atol=1e-12)
