"""Replica-exchange Gibbs sampling on the GPU (dca_plm_sample_tempered, dca_mf_sample_tempered, sample_sequences_tempered and the
sample_tempered sub-command) against the plain sampler (no exchange: the same bits), the float64
restatement of tempered_reference.py (whole trajectories, levels, counters and the energy trace) and exact enumeration.

A device exp may differ from numpy's in the last bit, so every exact comparison first checks, on the restatement alone, that
every Gibbs draw keeps a relative margin above 1e-12 (the project's bound, test_potts_sampling.py) and every exchange decision
with d < 0 a margin |U - exp(d)| above 1e-12: conditions on the inputs; a seed that fails one is changed, never the bound.  The
seeds below were checked on the CPU with tempered_reference.energies_np in the place of the context's energies (the two differ
by rounding only; the smallest margins met were 2e-8 for the draws and 5e-5 for the exchanges); the tests check again with the
context's own energies."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import data_file, golden
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from tempered_reference import exact_distribution, other_basin_share, tempered_ref, two_basin_model
from test_potts_sampling import _g_test, mf_context, mf_random_context, plm_context

pytestmark = pytest.mark.gpu

KEYS = ("codes", "levels", "energies", "attempts", "accepts", "trace")


def same(a, b, keys=KEYS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and a["rounds"] == b["rounds"]


# ---------------------------------------------------------------- 1. no exchange: the plain sampler's bits
def check_no_exchange(tempered, plain, L):
    betas = np.array([0.0, 0.7, 1.3])
    M, R = 50, 3                                                 # 150 walkers: R does not divide 64, beta is mixed in every workgroup
    res = tempered(M, betas, 4, swap_interval=0, seed=17, first_ladder=5, first_sweep=3, trace=True)
    assert res["rounds"] == 0 and res["trace"].shape == (0, M, R) and not res["attempts"].any() and not res["accepts"].any()
    assert res["levels"].tolist() == list(range(R)) * M
    for r in range(R):                                           # row m R + r is chain (5 + m) R + r under betas[r]
        want = plain(M * R, 4, seed=17, beta=betas[r], first_chain=5 * R, first_sweep=3)
        assert np.array_equal(res["codes"][r::R], want[r::R]), r
    X0 = np.random.default_rng(L).integers(0, 5, size=(M * R, L), dtype=np.uint8)
    res = tempered(M, betas, 3, swap_interval=0, seed=2, initial=X0)
    for r in range(R):
        assert np.array_equal(res["codes"][r::R], plain(M * R, 3, seed=2, beta=betas[r], initial=X0)[r::R]), r


@pytest.mark.parametrize("q,L", [(5, 23), (21, 37)])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_plm_without_exchange_is_the_plain_sampler(q, L, prec):
    ctx, _h, _Jp = plm_context(L, q, prec, 10 * q + prec)
    check_no_exchange(ctx.plm_sample_tempered, ctx.plm_sample, L)
    res = ctx.plm_sample_tempered(7, [0.5, 1.0], 2, swap_interval=0, seed=1)
    assert res["energies"].tobytes() == ctx.plm_energies(res["codes"]).tobytes()
    ctx.close()


def test_mf_without_exchange_is_the_plain_sampler():
    ctx, _h, _Jp, X = mf_context("mf_toy_rna")
    check_no_exchange(ctx.mf_sample_tempered, ctx.mf_sample, X.shape[1])
    ctx.close()


def test_mf_largest_alphabet_without_exchange_is_the_plain_sampler():
    """q = 32: the tempered sweep with 32 accumulators per lane, which no other case reaches"""
    ctx, _h, _Jp = mf_random_context(10, 32, 5)
    check_no_exchange(ctx.mf_sample_tempered, ctx.mf_sample, 10)
    ctx.close()


# ---------------------------------------------------------------- 2. exact trajectories with exchange
def check_against_restatement(tempered, energies, h, Jp, betas, M, sweeps, I, seed, first_ladder, first_sweep):
    ref = tempered_ref(h, Jp, betas, M, sweeps, I, seed, first_ladder=first_ladder, first_sweep=first_sweep, energy=energies)
    print("L %d, q %d, R %d, M %d, I %d: smallest draw margin %.3g, smallest exchange margin %.3g, acceptance %s"
          % (h.shape[0], h.shape[1], len(betas), M, I, ref["gibbs_margin"], ref["swap_margin"],
             (ref["accepts"] / np.maximum(ref["attempts"], 1)).round(3).tolist()))
    assert ref["gibbs_margin"] > 1e-12 and ref["swap_margin"] > 1e-12, "change the seed"
    res = tempered(M, betas, sweeps, swap_interval=I, seed=seed, first_ladder=first_ladder, first_sweep=first_sweep, trace=True)
    assert res["rounds"] == ref["rounds"] == (first_sweep + sweeps) // I - first_sweep // I
    assert np.array_equal(res["codes"], ref["codes"]), int((res["codes"] != ref["codes"]).sum())
    assert np.array_equal(res["levels"], ref["levels"])
    assert res["attempts"].dtype == np.uint64 and np.array_equal(res["attempts"], ref["attempts"])
    assert np.array_equal(res["accepts"], ref["accepts"])
    assert res["trace"].tobytes() == ref["trace"].tobytes()
    assert res["energies"].tobytes() == np.asarray(energies(res["codes"])).tobytes()
    return res


@pytest.mark.parametrize("R,I", [(4, 1), (5, 3), (5, 1), (4, 3)])
@pytest.mark.parametrize("q,L,prec", [(5, 23, _lib.DCA_F64), (21, 37, _lib.DCA_F32)])
def test_plm_trajectories_with_exchange_match_restatement(q, L, prec, R, I):
    """R = 5 leaves a level unpaired in alternate rounds; betas[0] = 0; first_sweep = 2 is no multiple of I = 3."""
    ctx, h, Jp = plm_context(L, q, prec, 10 * q + prec, sigma=0.15)
    betas = np.array([0.0, 0.5, 1.0, 1.6, 2.4][:R])
    res = check_against_restatement(ctx.plm_sample_tempered, ctx.plm_energies, h, Jp, betas, 40, 12, I, 31 + R, 7, 2)
    assert res["accepts"].sum() > 0 and (res["accepts"] < res["attempts"]).any()       # both outcomes were met
    ctx.close()


def test_mf_trajectories_with_exchange_match_restatement():
    ctx, h, Jp, _X = mf_context("mf_toy_rna")
    check_against_restatement(ctx.mf_sample_tempered, ctx.mf_energies, h, Jp, np.array([0.0, 0.3, 0.6, 1.0]), 40, 12, 3, 8, 7, 2)
    ctx.close()


@pytest.mark.parametrize("L,q,R,M", [(1200, 5, 2, 33), (500, 21, 3, 22)])
def test_large_shapes_match_restatement(L, q, R, M):
    """(1200, 5): the chain codes beyond LDS, kept in global memory; (500, 21): many chunks of row i per site."""
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F32, L, sigma=0.05, N=16)
    check_against_restatement(ctx.plm_sample_tempered, ctx.plm_energies, h, Jp, np.array([0.9, 0.95, 1.0][:R]), M, 2, 1, 3, 0, 0)
    ctx.close()


# ---------------------------------------------------------------- 3. bitwise invariances
def test_split_single_ladder_continuation_and_passes(monkeypatch):
    ctx, _h, _Jp = plm_context(30, 21, _lib.DCA_F32, 5, sigma=0.2)
    betas = np.array([0.0, 0.4, 0.8, 1.2, 1.7])
    M, R, I = 37, 5, 3
    run = ctx.plm_sample_tempered
    full = run(M, betas, 11, swap_interval=I, seed=42, first_ladder=4, first_sweep=2, trace=True)
    assert full["rounds"] == 4 and full["accepts"].sum() > 0
    a = run(15, betas, 11, swap_interval=I, seed=42, first_ladder=4, first_sweep=2, trace=True)
    b = run(M - 15, betas, 11, swap_interval=I, seed=42, first_ladder=19, first_sweep=2, trace=True)
    for k in ("codes", "levels", "energies"):
        assert np.concatenate([a[k], b[k]]).tobytes() == full[k].tobytes(), k
    assert np.array_equal(a["attempts"] + b["attempts"], full["attempts"]) and np.array_equal(a["accepts"] + b["accepts"], full["accepts"])
    assert np.concatenate([a["trace"], b["trace"]], axis=1).tobytes() == full["trace"].tobytes()
    for m in (0, 12, M - 1):                                     # one ladder alone
        one = run(1, betas, 11, swap_interval=I, seed=42, first_ladder=4 + m, first_sweep=2, trace=True)
        assert np.array_equal(one["codes"], full["codes"][m * R:(m + 1) * R]) and np.array_equal(one["levels"], full["levels"][m * R:(m + 1) * R])
        assert one["trace"].tobytes() == full["trace"][:, m:m + 1].tobytes()
    # 4 + 7 sweeps: the continuation starts at first_sweep = 6, no multiple of I
    head = run(M, betas, 4, swap_interval=I, seed=42, first_ladder=4, first_sweep=2, trace=True)
    tail = run(M, betas, 7, swap_interval=I, seed=42, first_ladder=4, first_sweep=6, initial=head["codes"], initial_levels=head["levels"],
               trace=True)
    assert head["rounds"] == 2 and tail["rounds"] == 2
    for k in ("codes", "levels", "energies"):
        assert tail[k].tobytes() == full[k].tobytes(), k
    assert np.array_equal(head["attempts"] + tail["attempts"], full["attempts"]) and np.array_equal(head["accepts"] + tail["accepts"], full["accepts"])
    assert np.concatenate([head["trace"], tail["trace"]]).tobytes() == full["trace"].tobytes()
    # blocks of 10 ladders, the trace flushed every 3 rounds (4 rounds: a full and a partial flush per block)
    monkeypatch.setenv("DCA_PT_PASS", "10")
    monkeypatch.setenv("DCA_PT_TRACE_ROUNDS", "3")
    before = _lib.device_blocks_in_use()
    assert same(run(M, betas, 11, swap_interval=I, seed=42, first_ladder=4, first_sweep=2, trace=True), full)
    assert _lib.device_blocks_in_use() == before
    monkeypatch.setenv("DCA_PT_TRACE_ROUNDS", "1")
    assert same(run(M, betas, 11, swap_interval=I, seed=42, first_ladder=4, first_sweep=2, trace=True), full)
    ctx.close()


# ---------------------------------------------------------------- 4. the stationary distribution at every level
def test_distribution_of_final_states_at_every_level():
    """test_tempered_sampling_host's enumerated case on the device: L = 4, q = 5, betas (0, 0.5, 1, 2), 50 000 ladders, 30 sweeps,
    an exchange round after every sweep; per level test_distribution_of_final_states' criteria."""
    L, q, M = 4, 5, 50000
    ctx, _h, _Jp = plm_context(L, q, _lib.DCA_F64, 77)
    states = np.array(np.unravel_index(np.arange(q ** L), (q,) * L)).T.astype(np.uint8)
    E = ctx.plm_energies(states)
    betas = np.array([0.0, 0.5, 1.0, 2.0])
    R = betas.size
    res = ctx.plm_sample_tempered(M, betas, 30, swap_interval=1, seed=2024)
    assert res["rounds"] == 30 and res["attempts"].tolist() == [15 * M, 15 * M, 15 * M]
    at = np.argsort(res["levels"].reshape(M, R), axis=1)
    codes = res["codes"].reshape(M, R, L)
    for k, beta in enumerate(betas):
        out = codes[np.arange(M), at[:, k]]
        idx = np.ravel_multi_index(out.T.astype(np.int64), (q,) * L)
        w = np.exp(beta * (E - E.max()))
        P = w / w.sum()
        p = _g_test(np.bincount(idx, minlength=q ** L).astype(np.float64), M * P)
        assert p > 1e-6, (beta, p)
        mean, var = float(np.dot(P, E)), float(np.dot(P, (E - np.dot(P, E)) ** 2))
        if var > 0:
            assert abs(E[idx].mean() - mean) <= 5.0 * math.sqrt(var / M), beta
    ctx.close()


# ---------------------------------------------------------------- 5. what the feature is for
def test_tempering_reaches_the_basin_plain_gibbs_does_not():
    """tempered_reference.two_basin_model at L = 8 with strength 1.0 and bias 0.05 (set by plm_set_x): the basins of all-0 and
    all-1 sequences, with a barrier of 16 units of energy between them.  dca_plm_configure takes q = 5 and q = 21 only, so the
    model has q = 5 states of which the model's fields push the last three down by the strength; its 5^8 states are enumerated.
    At beta = 1 the exact weight of the sequences with more 1s than 0s is 0.5984.  1000 chains started at all-0: on the CPU with
    the restatements, plain Gibbs at beta = 1 leaves a share of 0.001 there after 100 sweeps (5 binomial sigma: 0.0775), the
    tempered run over betas (0, 0.2, 0.4, 0.7, 1) with an exchange round per sweep 0.600.  The device must reproduce both
    outcomes."""
    L, q, M, sweeps = 8, 5, 1000, 100
    betas = np.array([0.0, 0.2, 0.4, 0.7, 1.0])
    R = betas.size
    h, Jp, x = two_basin_model(L, q, 1.0, 0.05)
    states, _E, P = exact_distribution(h, Jp, betas[-1])
    exact = float(P[(states == 1).sum(axis=1) > (states == 0).sum(axis=1)].sum())
    bound = 5.0 * math.sqrt(exact * (1.0 - exact) / M)
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(np.random.default_rng(0).integers(0, q, size=(20, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.plm_configure(1.0, 1.0)
    ctx.plm_set_x(x)
    plain = other_basin_share(ctx.plm_sample(M, sweeps, seed=11, beta=betas[-1], initial=np.zeros((M, L), dtype=np.uint8)))
    res = ctx.plm_sample_tempered(M, betas, sweeps, swap_interval=1, seed=11, initial=np.zeros((M * R, L), dtype=np.uint8))
    cold = res["codes"].reshape(M, R, L)[np.arange(M), np.argsort(res["levels"].reshape(M, R), axis=1)[:, -1]]
    tempered = other_basin_share(cold)
    print("exact %.4f, 5 sigma %.4f, plain %.4f, tempered %.4f" % (exact, bound, plain, tempered))
    assert abs(plain - exact) > bound
    assert abs(tempered - exact) <= bound
    ctx.close()


# ---------------------------------------------------------------- 6. errors and state
def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def _raw(ctx, fn, M=2, betas=(0.5, 1.0), R=None, sweeps=1, I=1, first_sweep=0, X0=None, levels=None, out=True, levels_out=True, args=True):
    L = ctx.L
    b = None if betas is None else np.asarray(betas, dtype=np.float64)
    R = (0 if b is None else b.size) if R is None else R
    n = max(M, 1) * max(R, 1) if M < 1000 else 1                # (the refused walker count needs no buffers)
    lv = None if levels is None else np.asarray(levels, dtype=np.int32)
    a = _lib.PtArgs(M, R, None if b is None else b.ctypes.data, sweeps, I, 0, 0, first_sweep, None if X0 is None else X0.ctypes.data,
                    None if lv is None else lv.ctypes.data)
    o = np.zeros((n, L), dtype=np.uint8)
    lo = np.zeros(n, dtype=np.int32)
    return fn(ctx._h, ctypes.byref(a) if args else None, o.ctypes.data if out else None, lo.ctypes.data if levels_out else None, None, None,
              None, None, None)


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    lib = _lib.lib()
    before = _lib.device_blocks_in_use()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_sample_tempered(2, [0.5, 1.0], 1)) == _lib.DCA_ERR_STATE          # before dca_plm_configure
    assert _code(lambda: ctx.mf_sample_tempered(2, [0.5, 1.0], 1)) == _lib.DCA_ERR_STATE           # before the mf couplings
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    fn = lib.dca_plm_sample_tempered
    assert _raw(ctx, fn) == _lib.DCA_OK
    whole = _lib.device_blocks_in_use()
    bad = np.zeros((4, L), dtype=np.uint8)
    bad[3, 3] = q
    for kw in (dict(args=False), dict(M=-1), dict(R=0), dict(betas=(), R=0), dict(sweeps=-1), dict(I=-1), dict(betas=None, R=2),
               dict(betas=(0.5, 0.5)), dict(betas=(1.0, 0.5)), dict(betas=(-0.1, 0.5)), dict(betas=(0.5, float("nan"))),
               dict(betas=(0.5, float("inf"))), dict(out=False), dict(levels_out=False), dict(levels=(0, 1, 1, 1)),
               dict(levels=(0, 1, 0, 2)), dict(levels=(0, 1, -1, 0)), dict(levels=(1, 1, 0, 1)), dict(X0=bad),
               dict(M=1 << 23, betas=(0.1, 0.2, 0.3)), dict(first_sweep=2 ** 64 - 1, sweeps=1)):
        assert _raw(ctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
        assert _lib.device_blocks_in_use() == whole, kw              # a refused call leaves nothing behind
    assert _raw(ctx, fn, M=0, out=False, levels_out=False) == _lib.DCA_OK
    assert _raw(ctx, fn, levels=(1, 0, 0, 1)) == _lib.DCA_OK
    assert _raw(ctx, fn, betas=(0.0,)) == _lib.DCA_OK                                               # R = 1: nothing to exchange
    empty = ctx.plm_sample_tempered(0, [0.5, 1.0], 3, trace=True)
    assert empty["codes"].shape == (0, L) and empty["rounds"] == 3 and empty["trace"].shape == (3, 0, 2) and not empty["attempts"].any()
    single = ctx.plm_sample_tempered(70, [0.7], 2, seed=5, first_ladder=3, trace=True)
    assert np.array_equal(single["codes"], ctx.plm_sample(70, 2, seed=5, beta=0.7, first_chain=3)) and single["rounds"] == 2
    assert single["trace"].shape == (2, 70, 1) and single["trace"][-1, :, 0].tobytes() == single["energies"].tobytes()
    start = ctx.plm_sample_tempered(35, [0.5, 1.0], 0, seed=5, first_ladder=3)                     # sweeps = 0: the random start
    assert np.array_equal(start["codes"], ctx.plm_sample(70, 0, seed=5, first_chain=6)) and start["rounds"] == 0

    # device ownership: the entry balances, with and without trace, passes and flushes
    for kw in (dict(), dict(trace=True), dict(swap_interval=0)):
        ctx.plm_sample_tempered(9, [0.2, 0.5, 1.0], 4, seed=3, **kw)
        first = _lib.device_blocks_in_use()
        ctx.plm_sample_tempered(9, [0.2, 0.5, 1.0], 4, seed=3, **kw)
        assert _lib.device_blocks_in_use() == first, kw

    ctx.set_profiling(True)
    ctx.plm_sample_tempered(8, [0.2, 0.5, 1.0], 7, swap_interval=2, first_sweep=1)                 # rounds after sweeps 1, 3, 5, 7
    assert ctx.kernel_time("sample")[1] == 7 and ctx.kernel_time("pt_energy")[1] == 5 and ctx.kernel_time("pt_swap")[1] == 4
    ctx.set_profiling(False)

    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert ctx.plm_sample_tempered(4, [0.5, 1.0], 2)["codes"].shape == (8, L)                       # allowed during an L-BFGS run
    ctx.plm_lbfgs_end()
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_sample_tempered(2, [0.5, 1.0], 1)) == _lib.DCA_ERR_STATE          # one GPU only
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_sample_tempered(2, [0.5, 1.0], 1)) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)
    assert ctx.plm_sample_tempered(2, [0.5, 1.0], 1)["codes"].shape == (4, L)
    ctx.close()
    assert _lib.device_blocks_in_use() == before
    mctx, _h, _Jp, MX = mf_context("mf_toy_rna")
    fn = lib.dca_mf_sample_tempered
    assert _raw(mctx, fn) == _lib.DCA_OK
    bad = np.zeros((4, MX.shape[1]), dtype=np.uint8)
    bad[0, 0] = 5
    for kw in (dict(M=-1), dict(betas=(1.0, 1.0)), dict(levels=(0, 0, 0, 1)), dict(out=False), dict(X0=bad)):
        assert _raw(mctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    mctx.close()


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
    E0 = ctx.plm_energies(X[:50])
    ctx.plm_sample_tempered(60, [0.0, 0.5, 1.0], 5, seed=5, trace=True)
    ctx.plm_sample_tempered(20, [0.5, 1.0], 2, swap_interval=0, seed=5, initial=X[np.arange(40) % X.shape[0]])
    assert ctx.plm_get_x(np.float32).tobytes() == x0.tobytes()
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.weights().tobytes() == w0.tobytes()
    assert ctx.plm_energies(X[:50]).tobytes() == E0.tobytes()
    assert ctx.plm_bm_iterate(1).tobytes() == rec_ref.tobytes()
    assert ctx.plm_get_x(np.float32).tobytes() == x_ref.tobytes()
    assert np.array_equal(ctx.plm_bm_chains(), ch_ref)
    ctx.close()
    mctx, _h, _Jp, _MX = mf_context()
    J0 = mctx.mf_couplings()
    mctx.mf_sample_tempered(30, [0.5, 1.0], 3, seed=1)
    assert mctx.mf_couplings().tobytes() == J0.tobytes()
    mctx.close()


# ---------------------------------------------------------------- 7. classes and command lines
def check_result(res, T, n, L, letters):
    assert sorted(res) == sorted(["temperatures", "sequences", "energies", "swap_acceptance", "swap_attempts", "mean_energy",
                                  "heat_capacity", "num_rounds"])
    R = len(set(T))
    assert res["temperatures"].tolist() == list(T) and len(res["sequences"]) == len(T)
    assert all(len(S) == n and all(len(s) == L and set(s) <= set(letters) for s in S) for S in res["sequences"])
    assert res["energies"].shape == (len(T), n) and res["swap_acceptance"].shape == (R - 1,) and res["swap_attempts"].shape == (R - 1,)
    assert res["mean_energy"].shape == (len(T),) and res["heat_capacity"].shape == (len(T),)
    assert np.all(np.isfinite(res["mean_energy"])) and np.all(res["heat_capacity"] >= 0)


def _read_tempered(path):
    heads = [ln for ln in open(path).read().splitlines() if ln.startswith(">")]
    return (fasta_reader.get_alignment_from_fasta_file(path), [h.split()[0] for h in heads],
            [float(h.split("temperature=")[1].split()[0]) for h in heads], np.array([float(h.split("energy=")[1]) for h in heads]))


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    T = [1.0, 0.5, 2.0, 0.7]                                    # the caller's order, not the ladder's
    res = inst.sample_sequences_tempered(25, T, num_sweeps=20, seed=4)
    check_result(res, T, 25, 10, "ACGU-")
    assert res["num_rounds"] == 20 and res["swap_attempts"].tolist() == [250, 250, 250]
    for t in range(len(T)):
        assert inst.compute_sequence_energies(res["sequences"][t]).tobytes() == res["energies"][t].tobytes()
    order = np.argsort(T)                                        # colder samples lie higher in energy on average
    assert res["mean_energy"][order[0]] > res["mean_energy"][order[-1]]
    again = inst.sample_sequences_tempered(25, T[::-1], num_sweeps=20, seed=4)
    assert again["sequences"] == res["sequences"][::-1] and again["mean_energy"].tolist() == res["mean_energy"][::-1].tolist()
    codes = inst.sample_sequences_tempered(25, T, num_sweeps=20, seed=4, return_codes=True)["sequences"]
    assert [["".join("ACGU-"[c] for c in row) for row in block] for block in codes] == res["sequences"]
    plain = inst.sample_sequences_tempered(25, T, num_sweeps=6, swap_interval=0, seed=4)
    beta_order = np.argsort(-np.array(T))                        # walker r of ladder m is chain m R + r at level r
    for t in range(len(T)):
        r = int(np.where(beta_order == t)[0][0])
        assert plain["sequences"][t] == inst.sample_sequences(100, num_sweeps=6, seed=4, temperature=T[t])[r::4]
    with pytest.raises(PlmDCAException, match="temperature"):
        inst.sample_sequences_tempered(2, [1.0, -1.0])
    out = str(tmp_path / "plm_out")
    fa, txt = plmdca_main.run_plm_dca(["sample_tempered", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                       "--output_dir", out, "--num_sequences", "25", "--temperatures", "1,0.5,2,0.7", "--num_sweeps", "20",
                                       "--seed", "4"])
    assert os.path.basename(fa) == "PLMDCA_tempered_samples_toy_rna.fa" and os.path.basename(txt) == "PLMDCA_tempered_sampling_toy_rna.txt"
    seqs, names, temps, E = _read_tempered(fa)
    assert temps == [t for t in T for _ in range(25)] and names == [">sample_%d" % (k + 1) for _ in T for k in range(25)]
    assert seqs == [s for S in res["sequences"] for s in S] and E.tobytes() == res["energies"].reshape(-1).tobytes()
    rows = [ln.split() for ln in open(txt).read().splitlines() if not ln.startswith("#")]
    assert [float(r[0]) for r in rows] == T and [float(r[1]) for r in rows] == res["mean_energy"].tolist()
    acc = {2.0: res["swap_acceptance"][0], 1.0: res["swap_acceptance"][1], 0.7: res["swap_acceptance"][2]}
    assert all((r[3] == "nan") if float(r[0]) == 0.5 else float(r[3]) == acc[float(r[0])] for r in rows)


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    L = inst.sequences_len
    letters = _potts.state_letters(_lib.DCA_BIOMOLECULE_PROTEIN)
    T = [float("inf"), 1.0, 3.0]
    res = inst.sample_sequences_tempered(12, T, num_sweeps=10, swap_interval=2, seed=9, initial=seqs[1])       # the couplings are computed here
    check_result(res, T, 12, L, letters)
    assert res["num_rounds"] == 5
    with pytest.raises(MeanFieldDCAException, match="records"):
        inst.sample_sequences_tempered(3, T, initial=seqs[:2])
    out = str(tmp_path / "mf_out")
    fa, txt = mfdca_main.run_meanfield_dca(["sample_tempered", "protein", path, "--output_dir", out, "--num_sequences", "6",
                                            "--temperatures", "inf,1,3", "--num_sweeps", "4", "--swap_interval", "2"])
    assert os.path.basename(fa) == "MFDCA_tempered_samples_toy_protein.fa" and os.path.basename(txt) == "MFDCA_tempered_sampling_toy_protein.txt"
    got, _names, temps, E = _read_tempered(fa)
    assert len(got) == 18 and temps == [t for t in T for _ in range(6)]
    assert np.allclose(E, inst.compute_sequence_energies(got), rtol=1e-12, atol=1e-12)
    assert len([ln for ln in open(txt).read().splitlines() if not ln.startswith("#")]) == 3
