"""log Z by annealed importance sampling on the GPU (dca_plm_ais, dca_mf_ais, the class methods and the command lines), checked
against a float64 numpy restatement kept in this file (Philox tags 0 and 2, the interpolated conditionals, the energy sums),
exact identities, exact enumeration of small models, and bitwise invariances."""
import math
import os

import numpy as np
import pytest

from conftest import data_file, golden
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from test_potts_sampling import mf_context, mf_model, plm_context, uniforms

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- numpy float64 restatement
def draw(p, r):
    """the samplers' draw rule on rows of p (n x q) with r = U * T; -> picks, smallest relative margin"""
    q = p.shape[1]
    cum = np.cumsum(p, axis=1)
    above = cum > r[:, None]
    pick = np.where(above.any(axis=1), above.argmax(axis=1), q - 1 - np.argmax((p > 0)[:, ::-1], axis=1))
    return pick, float((np.abs(cum - r[:, None]) / cum[:, -1:]).min())


def start_ref(h0, seed, chains):
    L, q = h0.shape
    X = np.zeros((len(chains), L), dtype=np.int64)
    margin = np.inf
    for i in range(L):
        p = np.exp(h0[i] - h0[i].max())[None, :].repeat(len(chains), axis=0)
        X[:, i], m = draw(p, uniforms(seed, chains, 0, i, 2) * p.sum(axis=1))
        margin = min(margin, m)
    return X, margin


def energy_ref(h, Jp, X):
    L = h.shape[0]
    iu, ju = np.triu_indices(L, 1)
    E = h[np.arange(L)[None, :], X].sum(axis=1)
    return E + Jp[np.arange(iu.size)[None, :], X[:, iu], X[:, ju]].sum(axis=1)


def sweeps_ref(h, Jp, h0, bk, seed, chains, first_sweep, sweeps, S):
    L, q = h.shape
    iu, ju = np.triu_indices(L, 1)
    pidx = np.zeros((L, L), dtype=np.int64)
    pidx[iu, ju] = np.arange(iu.size)
    pidx[ju, iu] = np.arange(iu.size)
    rows = np.arange(S.shape[0])
    margin = np.inf
    for t in range(sweeps):
        for i in range(L):
            Jrow = Jp[pidx[i]].copy()
            Jrow[:i] = Jrow[:i].transpose(0, 2, 1)
            Jrow[i] = 0.0
            u = h[i][None, :] + Jrow[np.arange(L)[None, :], :, S].sum(axis=1)
            c = h0[i][None, :] + bk * (u - h0[i][None, :])
            p = np.exp(c - c.max(axis=1, keepdims=True))
            pick, m = draw(p, uniforms(seed, chains, first_sweep + t, i, 0) * p.sum(axis=1))
            margin = min(margin, m)
            S[rows, i] = pick
    return margin


def ais_ref(h, Jp, h0, K, s, seed, chains, betas=None):
    """-> final chains, log weights, log Z0, smallest draw margin"""
    L, q = h.shape
    b = np.arange(K + 1) / K if betas is None else np.asarray(betas)
    X, margin = start_ref(h0, seed, chains)
    logw = np.zeros(len(chains))
    for k in range(1, K + 1):
        E0 = h0[np.arange(L)[None, :], X].sum(axis=1)
        logw = logw + (b[k] - b[k - 1]) * (energy_ref(h, Jp, X) - E0)
        if k < K:
            margin = min(margin, sweeps_ref(h, Jp, h0, b[k], seed, chains, (k - 1) * s, s, X))
    lz0 = sum(m + math.log(np.exp(h0[i] - m).sum()) for i, m in enumerate(h0.max(axis=1)))
    return X.astype(np.uint8), logw, lz0, margin


def e0_exact(h0, X):
    """E0 in the entries' order: double sums over ascending sites"""
    e = np.zeros(X.shape[0])
    for i in range(X.shape[1]):
        e = e + h0[i, X[:, i]]
    return e


def check_restatement(run, h, Jp, h0, K, s, seed, chains, betas=None):
    logw, lz0, X = run(len(chains), K, sweeps_per_temperature=s, seed=seed, first_chain=int(chains[0]), betas=betas,
                       base_fields=h0, return_chains=True)
    Xr, wr, zr, margin = ais_ref(h, Jp, h if h0 is None else h0, K, s, seed, chains, betas)
    assert margin > 1e-12, margin
    assert np.array_equal(X, Xr), int((X != Xr).sum())
    assert np.allclose(logw, wr, rtol=1e-12, atol=1e-12 * np.abs(wr).max()), np.abs(logw - wr).max()
    assert abs(lz0 - zr) <= 1e-12 * abs(zr)
    return logw, X


# ---------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("q,L", [(5, 23), (21, 37)])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_plm_matches_restatement(q, L, prec):
    ctx, h, Jp = plm_context(L, q, prec, 3 * q + prec, sigma=0.3)
    rng = np.random.default_rng(q + prec)
    h0 = rng.normal(0, 1.0, (L, q))
    check_restatement(ctx.plm_ais, h, Jp, h0, 4, 2, 77, np.arange(5, 205))
    check_restatement(ctx.plm_ais, h, Jp, None, 3, 1, 78, np.arange(0, 130), betas=[0.0, 0.1, 0.7, 1.0])
    ctx.close()


@pytest.mark.parametrize("tag", ["mf_toy_protein", "mf_toy_rna"])
def test_mf_matches_restatement(tag):
    ctx, h, Jp, _X = mf_context(tag)
    L, q = h.shape
    h0 = np.random.default_rng(1).normal(0, 1.0, (L, q))
    check_restatement(ctx.mf_ais, h, Jp, h0, 4, 2, 5, np.arange(3, 163))
    check_restatement(ctx.mf_ais, h, Jp, None, 2, 3, 6, np.arange(0, 64))
    ctx.close()


# ---------------------------------------------------------------- 2. exact identities
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_single_temperature_is_energy_difference(prec):
    ctx, h, Jp = plm_context(29, 21, prec, 4, sigma=0.4)
    h0 = np.random.default_rng(2).normal(0, 1.0, h.shape)
    logw, _lz0, X0 = ctx.plm_ais(300, 1, sweeps_per_temperature=5, seed=8, first_chain=11, base_fields=h0, return_chains=True)
    assert np.array_equal(X0, start_ref(h0, 8, np.arange(11, 311))[0])
    assert logw.tobytes() == (ctx.plm_energies(X0) - e0_exact(h0, X0)).tobytes()
    ctx.close()
    mctx, h, Jp, _X = mf_context()
    logw, _lz0, X0 = mctx.mf_ais(100, 1, seed=3, return_chains=True)
    assert logw.tobytes() == (mctx.mf_energies(X0) - e0_exact(h, X0)).tobytes()
    mctx.close()


@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_independent_sites_are_exact(prec):
    ctx, h, Jp = plm_context(17, 5, prec, 5)
    dt = np.float64 if prec == _lib.DCA_F64 else np.float32
    x = ctx.plm_get_x(dt)
    x[17 * 5:] = 0
    ctx.plm_set_x(x)
    n, K, s = 200, 4, 3
    logw, lz0, X = ctx.plm_ais(n, K, sweeps_per_temperature=s, seed=21, first_chain=4, return_chains=True)
    assert np.all(logw == 0.0)
    log_z, ess, se = _lib.ais_estimate(logw, lz0)
    assert ess == n and se == 0.0
    assert log_z == (lz0 + math.log(n)) - math.log(n) and abs(log_z - lz0) <= 4e-16 * abs(lz0)    # log Z0 up to the rounding of + log n - log n
    _w, _z, X0 = ctx.plm_ais(n, 1, seed=21, first_chain=4, return_chains=True)
    assert np.array_equal(X, ctx.plm_sample(n, (K - 1) * s, seed=21, first_chain=4, first_sweep=0, beta=1.0, initial=X0))
    ctx.close()


# ---------------------------------------------------------------- 3. accuracy on enumerable models
def all_states(L, q):
    return np.stack(np.meshgrid(*[np.arange(q)] * L, indexing="ij"), axis=-1).reshape(-1, L).astype(np.uint8)


def check_accuracy(run_ais, energies, L, q, base, far=True):
    E = energies(all_states(L, q))
    exact = E.max() + math.log(np.exp(E - E.max()).sum())
    logw, lz0, _ = run_ais(2048, 200, sweeps_per_temperature=1, seed=13, base_fields=base)
    log_z, ess, se = _lib.ais_estimate(logw, lz0)
    tol = 4 * se + 1e-3
    assert abs(log_z - exact) <= tol, (log_z, exact, se, ess)
    if far:
        assert abs(lz0 - exact) > 3 * tol                   # the base model is far from the model
    total = np.exp(E - log_z).sum()
    assert abs(total - 1.0) <= math.expm1(tol) + 1e-12, total


@pytest.mark.parametrize("L,q", [(4, 5), (3, 21)])
def test_plm_log_z_matches_enumeration(L, q):
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F64, 100 + q, sigma=1.0)
    check_accuracy(ctx.plm_ais, ctx.plm_energies, L, q, np.zeros((L, q)))
    check_accuracy(ctx.plm_ais, ctx.plm_energies, L, q, None, far=False)
    ctx.close()


@pytest.mark.parametrize("L,q", [(4, 5), (3, 21)])
def test_mf_log_z_matches_enumeration(L, q):
    rng = np.random.default_rng(L * q)
    base = rng.integers(0, q, size=(1, L))
    X = np.repeat(base, 60, axis=0)
    flip = rng.random(X.shape) < 0.3
    X[flip] = rng.integers(0, q, size=int(flip.sum()))
    X[:30, 1] = X[:30, 0]                                      # a strongly coupled pair
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(X.astype(np.uint8), q)
    ctx.set_weights(np.ones(X.shape[0]))
    ctx.mf_corr_mat(0.2, want=False)
    ctx.mf_couplings(want=False)
    check_accuracy(ctx.mf_ais, ctx.mf_energies, L, q, np.zeros((L, q)))
    ctx.close()


# ---------------------------------------------------------------- 4. batch invariance
def test_batch_split_invariance():
    ctx, h, Jp = plm_context(31, 21, _lib.DCA_F32, 9, sigma=0.3)
    one = ctx.plm_ais(300, 5, sweeps_per_temperature=2, seed=4, return_chains=True)
    a = ctx.plm_ais(130, 5, sweeps_per_temperature=2, seed=4, return_chains=True)
    b = ctx.plm_ais(170, 5, sweeps_per_temperature=2, seed=4, first_chain=130, return_chains=True)
    assert one[0].tobytes() == np.concatenate([a[0], b[0]]).tobytes()
    assert np.array_equal(one[2], np.concatenate([a[2], b[2]]))
    assert one[1] == a[1] == b[1]
    ctx.close()
    mctx, h, Jp, _X = mf_context()
    one = mctx.mf_ais(200, 4, seed=2, return_chains=True)
    a = mctx.mf_ais(1, 4, seed=2, return_chains=True)
    b = mctx.mf_ais(199, 4, seed=2, first_chain=1, return_chains=True)
    assert one[0].tobytes() == np.concatenate([a[0], b[0]]).tobytes()
    assert np.array_equal(one[2], np.concatenate([a[2], b[2]]))
    mctx.close()


# ---------------------------------------------------------------- 5. large shapes
def test_large_shapes_match_restatement():
    L, q = 500, 21
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F32, L, sigma=0.05, N=16)
    h0 = np.random.default_rng(0).normal(0, 0.5, (L, q))
    check_restatement(ctx.plm_ais, h, Jp, h0, 3, 1, 31, np.arange(64))
    ctx.close()
    del Jp
    rng = np.random.default_rng(1)
    X = rng.integers(0, q, size=(120, L), dtype=np.uint8)
    mctx = _lib.Context(0, _lib.DCA_F64)
    mctx.set_msa(X, q)
    mctx.set_weights(np.ones(X.shape[0]))
    mctx.mf_corr_mat(0.5, want=False)
    J = mctx.mf_couplings()
    h, Jp = mf_model(J, mctx.mf_fields(), L, q)
    del J
    check_restatement(mctx.mf_ais, h, Jp, None, 3, 1, 32, np.arange(64))
    mctx.close()


# ---------------------------------------------------------------- 6. untouched state
def test_training_state_and_bm_run_untouched():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])

    def setup():
        ctx = _lib.Context(0, _lib.DCA_F32)
        ctx.set_msa(X, q)
        ctx.compute_weights(0.8, _lib.DCA_F32)
        ctx.plm_configure(1.8, 1.8)
        ctx.plm_init_x()
        ctx.plm_set_x(ctx.plm_get_x(np.float32) + np.random.default_rng(0).normal(0, 0.1, ctx.num_params()).astype(np.float32))
        ctx.plm_gradient()
        ctx.plm_bm_begin(128, 2, 3, seed=1, eta_h=0.05, eta_J=0.05, pseudocount=0.01)
        ctx.plm_bm_iterate(2)
        return ctx
    ref = setup()
    rec_ref = ref.plm_bm_iterate(1)
    x_ref, ch_ref = ref.plm_get_x(np.float32), ref.plm_bm_chains()
    ref.close()
    ctx = setup()
    x0, g0, w0 = ctx.plm_get_x(np.float32), ctx.plm_get_g(np.float32), ctx.weights()
    ctx.plm_ais(300, 6, sweeps_per_temperature=2, seed=5)
    ctx.plm_ais(64, 3, seed=5, base_fields=np.zeros((X.shape[1], q)))
    assert ctx.plm_get_x(np.float32).tobytes() == x0.tobytes()
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.weights().tobytes() == w0.tobytes()
    assert ctx.plm_bm_iterate(1).tobytes() == rec_ref.tobytes()
    assert ctx.plm_get_x(np.float32).tobytes() == x_ref.tobytes()
    assert np.array_equal(ctx.plm_bm_chains(), ch_ref)
    ctx.close()
    mctx, _h, _Jp, _MX = mf_context()
    J0 = mctx.mf_couplings()
    mctx.mf_ais(100, 3, seed=1)
    assert mctx.mf_couplings().tobytes() == J0.tobytes()
    mctx.close()


# ---------------------------------------------------------------- 7. errors
def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def _raw(ctx, fn, n=4, K=2, s=1, betas=None, base=None, out=True):
    import ctypes as C
    args = _lib.AisArgs(n, K, None if betas is None else betas.ctypes.data, s, 0, 0, None if base is None else base.ctypes.data)
    w = np.zeros(max(n, 1))
    return fn(ctx._h, C.byref(args), w.ctypes.data if out else None, None, None)


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    lib = _lib.lib()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_ais(4, 2)) == _lib.DCA_ERR_STATE                     # before dca_plm_configure
    assert _code(lambda: ctx.mf_ais(4, 2)) == _lib.DCA_ERR_STATE                      # before dca_mf_couplings
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert ctx.plm_ais(4, 2)[0].shape == (4,)                                        # allowed during an L-BFGS run, as sampling
    ctx.plm_lbfgs_end()
    fn = lib.dca_plm_ais
    ok = np.array([0.0, 0.5, 1.0])
    assert _raw(ctx, fn, betas=ok) == _lib.DCA_OK
    for kw in (dict(n=0), dict(n=(1 << 24) + 1), dict(K=0), dict(s=-1), dict(out=False),
               dict(betas=np.array([0.0, 0.5, 0.9])), dict(betas=np.array([0.1, 0.5, 1.0])), dict(betas=np.array([0.0, 0.6, 0.5])),
               dict(betas=np.array([0.0, 0.0, 1.0])), dict(betas=np.array([0.0, np.nan, 1.0])),
               dict(K=1, betas=np.array([0.0, np.inf])),
               dict(base=np.full((L, q), np.nan)), dict(base=np.full((L, q), -np.inf))):
        assert _raw(ctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    assert fn(ctx._h, None, np.zeros(1).ctypes.data, None, None) == _lib.DCA_ERR_ARG
    with pytest.raises(ValueError):
        ctx.plm_ais(4, 2, betas=[0.0, 1.0])
    ctx.set_profiling(True)
    ctx.plm_ais(8, 4, sweeps_per_temperature=2)
    assert ctx.kernel_time("sample")[1] == 6 and ctx.kernel_time("ais")[1] == 5
    ctx.set_profiling(False)
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_ais(4, 2)) == _lib.DCA_ERR_STATE                     # multi-GPU hooks
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_ais(4, 2)) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)
    assert ctx.plm_ais(4, 2)[0].shape == (4,)
    ctx.close()
    mctx, _h, _Jp, MX = mf_context("mf_toy_rna")
    fn = lib.dca_mf_ais
    assert _raw(mctx, fn) == _lib.DCA_OK
    for kw in (dict(n=0), dict(K=0), dict(s=-1), dict(out=False), dict(betas=np.array([0.0, 1.0, 2.0])),
               dict(base=np.full((MX.shape[1], 5), np.inf))):
        assert _raw(mctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    mctx.close()


# ---------------------------------------------------------------- 8. classes and command lines
def _read_ll(path):
    lines = open(path).read().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    rows = [ln for ln in lines if not ln.startswith("#")]
    assert rows[0].startswith("average_log_likelihood ")
    log_z = float([ln for ln in head if "log Z (annealed" in ln][0].split(": ")[1])
    return log_z, float(rows[0].split()[1]), np.array([float(v) for v in rows[1:]])


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    res = inst.compute_log_partition_function(num_chains=256, num_temperatures=20, seed=3)
    assert set(res) == {"log_z", "log_z_stderr", "ess", "log_z_base", "log_weights"}
    assert res["log_weights"].shape == (256,) and 1.0 <= res["ess"] <= 256 and math.isfinite(res["log_z"])
    again = inst.compute_log_partition_function(num_chains=256, num_temperatures=20, seed=3)
    assert again["log_weights"].tobytes() == res["log_weights"].tobytes()
    fields = inst.compute_log_partition_function(num_chains=256, num_temperatures=20, seed=3, base="fields")
    assert fields["log_z_base"] != res["log_z_base"]
    lp = inst.compute_sequence_log_probabilities(log_z=res["log_z"])
    assert lp.tobytes() == (inst.compute_sequence_energies() - res["log_z"]).tobytes()
    ll = inst.compute_log_likelihood(log_z=res["log_z"])
    assert math.isfinite(ll)
    assert inst.compute_log_likelihood(num_chains=256, num_temperatures=20, seed=3) == ll
    out = str(tmp_path / "plm_out")
    f = _potts.run_subcommand(inst, "compute_log_likelihood", "PLMDCA", path, out, None, _lib.DCA_BIOMOLECULE_RNA, 0, PlmDCAException,
                              ais={"num_chains": 256, "num_temperatures": 20, "seed": 3})
    log_z, avg, logp = _read_ll(f)
    assert log_z == res["log_z"] and avg == ll
    assert logp.tobytes() == (inst.compute_sequence_energies() - log_z).tobytes()
    f = plmdca_main.run_plm_dca(["compute_log_likelihood", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                 "--output_dir", out, "--num_chains", "256", "--num_temperatures", "20", "--seed", "3"])
    assert os.path.basename(f) == "PLMDCA_log_likelihood_toy_rna.txt"
    log_z, avg, logp2 = _read_ll(f)
    assert np.allclose([log_z, avg], [res["log_z"], ll], rtol=1e-9, atol=1e-9)
    assert np.allclose(logp2, logp, rtol=1e-9, atol=1e-9)


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    inst = MeanFieldDCA(path, "protein")
    res = inst.compute_log_partition_function(num_chains=128, num_temperatures=10, seed=1)
    assert res["log_weights"].shape == (128,) and math.isfinite(res["log_z"])
    lp = inst.compute_sequence_log_probabilities(num_chains=128, num_temperatures=10, seed=1)
    assert lp.tobytes() == (inst.compute_sequence_energies() - res["log_z"]).tobytes()
    ll = inst.compute_log_likelihood(log_z=res["log_z"])
    assert math.isfinite(ll)
    with pytest.raises(MeanFieldDCAException):
        inst.compute_log_partition_function(base=np.zeros((2, 2)))
    out = str(tmp_path / "mf_out")
    f = _potts.run_subcommand(inst, "compute_log_likelihood", "MFDCA", path, out, None, _lib.DCA_BIOMOLECULE_PROTEIN, 1,
                              MeanFieldDCAException, ais={"num_chains": 128, "num_temperatures": 10, "seed": 1})
    log_z, avg, logp = _read_ll(f)
    assert log_z == res["log_z"] and avg == ll
    assert logp.tobytes() == (inst.compute_sequence_energies() - log_z).tobytes()
    f = mfdca_main.run_meanfield_dca(["compute_log_likelihood", "protein", path, "--output_dir", out, "--num_chains", "128",
                                      "--num_temperatures", "10", "--seed", "1"])
    assert os.path.basename(f) == "MFDCA_log_likelihood_toy_protein.txt"
    log_z, avg, logp2 = _read_ll(f)
    assert np.allclose([log_z, avg], [res["log_z"], ll], rtol=1e-9, atol=1e-9)
    assert np.allclose(logp2, logp, rtol=1e-9, atol=1e-9)
