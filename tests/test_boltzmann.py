"""Boltzmann machine learning on the GPU (dca_plm_bm_*, PlmDCA.fit_boltzmann, plmdca fit_boltzmann), checked against a
float64 numpy restatement: the Gibbs restatement of tests/test_potts_sampling.py for the chains, integer counts for the model
statistics, and the update formula of include/dca_hip.h applied elementwise."""
import itertools
import os

import numpy as np
import pytest

from conftest import data_file, golden
from pydca_amd import _lib, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from test_potts_sampling import gibbs_ref, plm_model, random_start

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- numpy restatement
def pairs_of(L):
    return np.triu_indices(L, 1)


def data_stats(X, w, q, lam):
    """f^_i (L x q), f^_ij (pairs x q x q) of the weighted alignment"""
    L = X.shape[1]
    meff = w.sum()
    oh = np.eye(q)[X]
    fi = np.einsum("n,nia->ia", w, oh) / meff
    iu, ju = pairs_of(L)
    fij = np.einsum("n,npa,npb->pab", w, oh[:, iu, :], oh[:, ju, :]) / meff
    return (1.0 - lam) * fi + lam / q, (1.0 - lam) * fij + lam / q ** 2


def model_stats(S, q):
    """g_i, g_ij of the chains from integer counts"""
    n, L = S.shape
    S = S.astype(np.int64)
    ci = np.stack([np.bincount(S[:, i], minlength=q) for i in range(L)])
    iu, ju = pairs_of(L)
    code = (np.arange(iu.size)[None, :] * q * q + S[:, iu] * q + S[:, ju]).ravel()
    cij = np.bincount(code, minlength=iu.size * q * q).reshape(iu.size, q, q)
    return ci / float(n), cij / float(n)


def record(fi, fij, gi, gij, L):
    iu, ju = pairs_of(L)
    Cd = fij - fi[iu][:, :, None] * fi[ju][:, None, :]
    Cm = gij - gi[iu][:, :, None] * gi[ju][:, None, :]
    return np.array([np.abs(fi - gi).max(), np.abs(fij - gij).max(), np.corrcoef(Cd.ravel(), Cm.ravel())[0, 1]])


def update(x, fi, fij, gi, gij, eta_h, eta_J, mu_h, mu_J):
    """theta' = theta + eta ((f - g) - mu theta) in float64, rounded once to x's dtype"""
    th = x.astype(np.float64)
    f = np.concatenate([fi.ravel(), fij.ravel()])
    g = np.concatenate([gi.ravel(), gij.ravel()])
    nf = fi.size
    eta = np.where(np.arange(th.size) < nf, eta_h, eta_J)
    mu = np.where(np.arange(th.size) < nf, mu_h, mu_J)
    d = f - g
    r = mu * th
    s = d - r
    return (th + eta * s).astype(x.dtype)


def bm_ref(x, fi, fij, n, k, E, T, seed, rates, initial=None):
    """the run of dca_plm_bm_begin + T iterations -> per iteration (chains, x after the update, g_i, g_ij, record)"""
    L, q = fi.shape
    chains = np.arange(n)
    S = random_start(seed, chains, L, q) if initial is None else initial
    h, Jp = plm_model(x, L, q)
    S, m = gibbs_ref(h, Jp, 1.0, seed, chains, 0, E, S)
    assert m > 1e-12
    out = []
    for t in range(T):
        h, Jp = plm_model(x, L, q)
        S, m = gibbs_ref(h, Jp, 1.0, seed, chains, E + t * k, k, S)
        assert m > 1e-12, m
        gi, gij = model_stats(S, q)
        rec = record(fi, fij, gi, gij, L)
        x = update(x, fi, fij, gi, gij, *rates)
        out.append((S, x, gi, gij, rec))
    return out


# ---------------------------------------------------------------- helpers
def bm_context(L, q, precision, seed, N=60, sigma=0.3):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, q, size=(N, L), dtype=np.uint8)
    ctx = _lib.Context(0, precision)
    ctx.set_msa(X, q)
    ctx.set_weights(np.ones(N))
    ctx.plm_configure(1.0, 1.0)
    dt = np.float64 if precision == _lib.DCA_F64 else np.float32
    ctx.plm_set_x(rng.normal(0, sigma, ctx.num_params()).astype(dt))
    return ctx, X, dt


def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


# ---------------------------------------------------------------- 1. zero rates: the sampler
def test_zero_rates_equal_the_sampler():
    L, q, n, k, E, T, seed = 12, 21, 300, 3, 2, 3, 77
    ctx, X, dt = bm_context(L, q, _lib.DCA_F32, 1)
    x0 = ctx.plm_get_x(dt)
    X0 = np.random.default_rng(2).integers(0, q, size=(n, L), dtype=np.uint8)
    ctx.plm_bm_begin(n, k, E, seed=seed, mu_h=0.3, mu_J=0.2, pseudocount=0.05, initial=X0)
    fi, fij = ctx.plm_bm_freqs(0)
    recs = ctx.plm_bm_iterate(T)
    assert recs.shape == (T, 3)
    assert np.array_equal(ctx.plm_bm_chains(), ctx.plm_sample(n, E + T * k, seed=seed, initial=X0))
    assert ctx.plm_get_x(dt).tobytes() == x0.tobytes()
    for t in range(T):
        S = ctx.plm_sample(n, E + (t + 1) * k, seed=seed, initial=X0)
        gi, gij = model_stats(S, q)
        want = record(fi, fij, gi, gij, L)
        assert recs[t, :2].tobytes() == want[:2].tobytes()
        assert abs(recs[t, 2] - want[2]) <= 1e-12, (recs[t, 2], want[2])
    ctx.plm_bm_end()
    ctx.close()


# ---------------------------------------------------------------- 2. exact trajectory
@pytest.mark.parametrize("L,q", [(7, 5), (9, 21)])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_trajectory_matches_restatement(L, q, prec):
    n, k, E, T, seed, lam = 200, 2, 3, 4, 31 + q, 0.02
    rates = (0.3, 0.2, 0.01, 0.02)
    ctx, X, dt = bm_context(L, q, prec, 10 * q + prec)
    x = ctx.plm_get_x(dt)
    fi, fij = data_stats(X, np.ones(X.shape[0]), q, lam)
    ref = bm_ref(x, fi, fij, n, k, E, T, seed, rates)
    ctx.plm_bm_begin(n, k, E, seed=seed, eta_h=rates[0], eta_J=rates[1], mu_h=rates[2], mu_J=rates[3], pseudocount=lam)
    dfi, dfij = ctx.plm_bm_freqs(0)
    assert dfi.tobytes() == fi.tobytes() and dfij.tobytes() == fij.tobytes()
    for t in range(T):
        rec = ctx.plm_bm_iterate(1)[0]
        S, xr, gi, gij, want = ref[t]
        assert np.array_equal(ctx.plm_bm_chains(), S), t
        assert ctx.plm_get_x(dt).tobytes() == xr.tobytes(), t
        ggi, ggij = ctx.plm_bm_freqs(1)
        assert ggi.tobytes() == gi.tobytes() and ggij.tobytes() == gij.tobytes(), t
        assert rec[:2].tobytes() == want[:2].tobytes(), (t, rec, want)
        assert abs(rec[2] - want[2]) <= 1e-12, (t, rec, want)
    ctx.close()


# ---------------------------------------------------------------- 3. resumable
def test_iterate_is_resumable():
    L, q, n = 10, 21, 130
    args = dict(seed=5, eta_h=0.1, eta_J=0.1, mu_h=1e-3, mu_J=1e-3, pseudocount=0.01)
    runs = []
    for split in ((2, 3), (5,)):
        ctx, X, dt = bm_context(L, q, _lib.DCA_F32, 3)
        ctx.plm_bm_begin(n, 2, 1, **args)
        recs = np.concatenate([ctx.plm_bm_iterate(s) for s in split])
        runs.append((ctx.plm_get_x(dt), ctx.plm_bm_chains(), recs))
        ctx.close()
    (xa, ca, ra), (xb, cb, rb) = runs
    assert xa.tobytes() == xb.tobytes() and np.array_equal(ca, cb) and ra.tobytes() == rb.tobytes()


# ---------------------------------------------------------------- 4. general weights
def test_data_statistics_with_general_weights():
    L, q, lam = 15, 21, 0.03
    rng = np.random.default_rng(4)
    X = rng.integers(0, q, size=(30, L), dtype=np.uint8)[rng.integers(0, 30, 90)]       # near-duplicates: weights below 1
    X[rng.random(X.shape) < 0.1] = 0
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.plm_configure(1.0, 1.0)
    w = ctx.weights()
    assert not np.all(w == 1.0)
    ctx.plm_bm_begin(8, 1, 0, pseudocount=lam)
    fi, fij = ctx.plm_bm_freqs(0)
    rfi, rfij = data_stats(X, w, q, lam)
    assert np.max(np.abs(fi - rfi) / rfi) <= 1e-14
    assert np.max(np.abs(fij - rfij)) <= 1e-14 * np.max(rfij)           # relative to the largest frequency
    ctx.close()


# ---------------------------------------------------------------- 5. large shapes
@pytest.mark.parametrize("L,q,prec", [(520, 21, _lib.DCA_F32), (1200, 5, _lib.DCA_F64)])
def test_large_shapes_counts_and_update(L, q, prec):
    n = 70
    ctx, X, dt = bm_context(L, q, prec, L, N=20, sigma=0.05)
    rates = (0.2, 0.1, 0.01, 0.03)
    ctx.plm_bm_begin(n, 1, 1, seed=9, eta_h=rates[0], eta_J=rates[1], mu_h=rates[2], mu_J=rates[3], pseudocount=0.1)
    x0 = ctx.plm_get_x(dt)
    fi, fij = ctx.plm_bm_freqs(0)
    ctx.plm_bm_iterate(1)
    S = ctx.plm_bm_chains()
    gi, gij = model_stats(S, q)
    ggi, ggij = ctx.plm_bm_freqs(1)
    assert ggi.tobytes() == gi.tobytes() and ggij.tobytes() == gij.tobytes()
    assert ctx.plm_get_x(dt).tobytes() == update(x0, fi, fij, gi, gij, *rates).tobytes()
    ctx.close()


# ---------------------------------------------------------------- 6. it learns (enumerable model)
def exact_marginals(x, L, q):
    h, Jp = plm_model(x, L, q)
    S = np.array(list(itertools.product(range(q), repeat=L)))
    iu, ju = pairs_of(L)
    E = h[np.arange(L)[None, :], S].sum(axis=1) + Jp[np.arange(iu.size)[None, :], S[:, iu], S[:, ju]].sum(axis=1)
    p = np.exp(E - E.max())
    p /= p.sum()
    return data_stats(S.astype(np.uint8), p, q, 0.0)


def test_learns_an_enumerable_model():
    # n = 20000 chains, k = 2 sweeps, T = 600 iterations, eta = 0.2, mu = 0, pseudocount 1 / N, from x = 0
    L, q, N = 6, 5, 4000
    rng = np.random.default_rng(2024)
    iu, _ju = pairs_of(L)
    x_true = np.concatenate([rng.normal(0, 0.6, L * q), rng.normal(0, 0.6, iu.size * q * q)])
    S_all = np.array(list(itertools.product(range(q), repeat=L)), dtype=np.uint8)
    h, Jp = plm_model(x_true, L, q)
    E = h[np.arange(L)[None, :], S_all].sum(axis=1) + Jp[np.arange(iu.size)[None, :], S_all[:, iu], S_all[:, pairs_of(L)[1]]].sum(axis=1)
    p = np.exp(E - E.max())
    X = S_all[rng.choice(S_all.shape[0], size=N, p=p / p.sum())]
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X, q)
    ctx.set_weights(np.ones(N))
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(np.zeros(ctx.num_params()))
    ctx.plm_bm_begin(20000, 2, 20, seed=11, eta_h=0.2, eta_J=0.2, pseudocount=1.0 / N)
    fi, fij = ctx.plm_bm_freqs(0)
    hist = ctx.plm_bm_iterate(600)
    x = ctx.plm_get_x(np.float64)
    ctx.close()
    mi, mij = exact_marginals(x, L, q)
    zi, zij = exact_marginals(np.zeros_like(x), L, q)
    rec = record(fi, fij, mi, mij, L)
    zero = (np.abs(fi - zi).max(), np.abs(fij - zij).max())          # the uniform model: no connected correlations at all
    assert rec[1] <= 0.01 and rec[0] <= 0.01, (rec, zero)
    assert rec[2] >= 0.99, (rec, zero)
    assert rec[1] <= 0.25 * zero[1] and rec[0] <= 0.25 * zero[0], (rec, zero)
    assert hist[-1, 1] < hist[0, 1] and hist[-1, 2] > hist[0, 2]


# ---------------------------------------------------------------- 7. state and errors
def test_state_and_argument_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_bm_begin(10, 1, 0)) == _lib.DCA_ERR_STATE          # before dca_plm_configure
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert _code(lambda: ctx.plm_bm_begin(10, 1, 0)) == _lib.DCA_ERR_STATE          # L-BFGS run in progress
    ctx.plm_lbfgs_end()
    for call in (ctx.plm_bm_chains, lambda: ctx.plm_bm_iterate(1), lambda: ctx.plm_bm_freqs(0)):
        assert _code(call) == _lib.DCA_ERR_STATE                                    # no run
    bad = X[:3].copy()
    bad[2, 1] = q
    for kw in (dict(chains=0), dict(sweeps=0), dict(equilibration_sweeps=-1), dict(eta_h=-0.1), dict(eta_J=float("inf")),
               dict(mu_h=float("nan")), dict(mu_J=-1.0), dict(pseudocount=1.0), dict(pseudocount=-0.01),
               dict(chains=3, initial=bad)):
        a = dict(chains=10, sweeps=1, equilibration_sweeps=0)
        a.update(kw)
        assert _code(lambda: ctx.plm_bm_begin(**a)) == _lib.DCA_ERR_ARG, kw
    assert _lib.lib().dca_plm_bm_begin(ctx._h, None) == _lib.DCA_ERR_ARG
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_bm_begin(10, 1, 0)) == _lib.DCA_ERR_STATE          # multi-GPU hooks
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_bm_begin(10, 1, 0)) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)

    fx = ctx.plm_gradient()
    g0, w0, f0 = ctx.plm_get_g(np.float32), ctx.weights(), ctx.mf_single_site_freqs()
    ctx.plm_bm_begin(64, 2, 3, seed=1, eta_h=0.05, eta_J=0.05, pseudocount=0.01)
    assert _code(lambda: ctx.plm_bm_freqs(1)) == _lib.DCA_ERR_STATE                 # no iteration yet
    assert _code(lambda: ctx.plm_bm_freqs(2)) == _lib.DCA_ERR_ARG
    assert _code(lambda: ctx.plm_bm_iterate(-1)) == _lib.DCA_ERR_ARG
    assert ctx.plm_bm_iterate(0).shape == (0, 3)
    ctx.set_profiling(True)
    ctx.plm_bm_iterate(2)
    assert ctx.kernel_time("sample")[1] == 4 and ctx.kernel_time("bm_stats")[1] == 2
    x1 = ctx.plm_get_x(np.float32)
    ctx.plm_set_x(np.zeros_like(x1))                                                 # allowed during a run
    ctx.plm_bm_iterate(1)
    assert np.abs(ctx.plm_get_x(np.float32)).max() <= 0.05 * 1.0 + 1e-7
    ctx.plm_set_x(x1)
    ctx.plm_bm_iterate(1)
    ctx.plm_bm_end()
    assert _code(ctx.plm_bm_chains) == _lib.DCA_ERR_STATE
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.weights().tobytes() == w0.tobytes() and ctx.mf_single_site_freqs().tobytes() == f0.tobytes()
    x = ctx.plm_get_x(np.float32)
    h, Jp = plm_model(x, L, q)
    iu, ju = pairs_of(L)
    Xq = X[:25].astype(np.int64)
    E = h[np.arange(L)[None, :], Xq].sum(axis=1) + Jp[np.arange(iu.size)[None, :], Xq[:, iu], Xq[:, ju]].sum(axis=1)
    assert np.allclose(ctx.plm_energies(X[:25]), E, rtol=1e-12, atol=1e-12)
    for end in (lambda: ctx.set_weights(ctx.weights()), lambda: ctx.plm_configure(1.8, 1.8), lambda: ctx.plm_lbfgs_begin(5),
                ctx.plm_release, lambda: ctx.set_msa(X, q)):                          # each of these ends a run
        ctx.plm_configure(1.8, 1.8)
        ctx.plm_init_x()
        ctx.plm_lbfgs_end()
        ctx.plm_bm_begin(16, 1, 0)
        end()
        assert _code(lambda: ctx.plm_bm_iterate(1)) == _lib.DCA_ERR_STATE
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    ctx.plm_lbfgs_begin(3)
    st = ctx.plm_lbfgs_iterate(3)                                                    # a later L-BFGS run works
    assert np.isfinite(st.fx) and st.iterations >= 1 and np.isfinite(fx)
    ctx.close()


# ---------------------------------------------------------------- 8. class and command line
def test_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    before = inst.sample_sequences(30, num_sweeps=10, seed=3, return_codes=True)
    fit = inst.fit_boltzmann(iterations=40, num_chains=500, sweeps_per_iteration=2, equilibration_sweeps=10, learning_rate=0.1)
    H, x = fit["history"], fit["fields_and_couplings"]
    assert H.shape == (40, 3) and H.dtype == np.float64 and x.dtype == np.float32
    assert H[-1, 1] < H[0, 1]
    after = inst.sample_sequences(30, num_sweeps=10, seed=3, return_codes=True)
    L, q = inst.sequences_len, 5
    h, Jp = plm_model(x, L, q)
    ref, m = gibbs_ref(h, Jp, 1.0, 3, np.arange(30), 0, 10, random_start(3, np.arange(30), L, q))
    assert m > 1e-12 and np.array_equal(after, ref) and not np.array_equal(after, before)
    with pytest.raises(PlmDCAException):
        PlmDCA(path, "rna", devices=[0, 1]).fit_boltzmann(iterations=1)
    out = str(tmp_path / "bm_out")
    files = plmdca_main.run_plm_dca(["fit_boltzmann", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                     "--output_dir", out, "--iterations", "6", "--num_chains", "200", "--sweeps_per_iteration", "2",
                                     "--equilibration_sweeps", "4", "--learning_rate", "0.1", "--init", "zero", "--num_samples", "7",
                                     "--num_sweeps", "3", "--seed", "4"])
    assert [os.path.basename(f) for f in files] == ["PLMDCA_boltzmann_toy_rna.txt", "PLMDCA_boltzmann_params_toy_rna.npy",
                                                    "PLMDCA_boltzmann_samples_toy_rna.fa"]
    rows = [ln.split() for ln in open(files[0]).read().splitlines() if not ln.startswith("#")]
    assert len(rows) == 6 and [int(r[0]) for r in rows] == list(range(6)) and all(len(r) == 4 for r in rows)
    curve = np.array([[float(v) for v in r[1:]] for r in rows])
    assert np.all(np.isfinite(curve)) and np.all(curve[:, :2] >= 0)
    params = np.load(files[1])
    assert params.shape == x.shape and params.dtype == np.float32
    seqs = fasta_reader.get_alignment_from_fasta_file(files[2])
    assert len(seqs) == 7 and all(len(s) == L for s in seqs)
