"""Conditional Gibbs sampling on the GPU (dca_plm_sample_conditional, dca_mf_sample_conditional, sample_sequences_conditional
and the sample_conditional sub-command) against the plain sampler (all sites free: the same bits) and the
masked float64 restatement of test_conditional_sampling_host.py, at the smallest shapes where the two kernels change path.

Geometry behind the shapes (potts_plan.h, cond_sample_geometry): the sweep's chunks hold CJ free positions and the field pass's
CJ / 2 clamped sites; CJ = 16 (q = 21, float32), 8 (q = 21, float64), 256 (q = 5, float32), 128 (q = 5, float64); the free
sites' codes leave LDS above 512 free sites.

A device exp may differ from numpy's in the last bit, so every exact comparison first checks, on the restatement alone, that the
smallest |cum - r| / T of its draws exceeds potts_audit_reference's bound MARGIN_FACTOR * eps_draw (a condition on the inputs;
a seed that fails it is changed, never the bound)."""
import math
import os

import numpy as np
import pytest

from conftest import data_file, golden
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException
from potts_audit_reference import MARGIN_FACTOR, eps_draw, model_sabs
from test_conditional_sampling_host import cond_gibbs_ref
from test_potts_sampling import _g_test, mf_context, mf_model, mf_random_context, plm_context

pytestmark = pytest.mark.gpu


def backgrounds(n, L, q, seed):
    """a different background per chain"""
    return np.random.default_rng([seed, n, L, q]).integers(0, q, size=(n, L), dtype=np.uint8)


def check_against_restatement(call, h, Jp, X0, free, sweeps, seed, beta=1.0, randomize=True, first_chain=0, first_sweep=0):
    n, L = X0.shape
    q = h.shape[1]
    free = np.asarray(free, dtype=np.int64)
    chains = np.arange(first_chain, first_chain + n)
    ref, margin = cond_gibbs_ref(h, Jp, beta, seed, chains, first_sweep, sweeps, X0, free, randomize)
    need = MARGIN_FACTOR * eps_draw(q, L, beta, model_sabs(h, Jp))
    print("F %d of L %d, q %d, n %d: smallest draw margin %.3g, needed %.3g" % (free.size, L, q, n, margin, need))
    assert margin >= need, "the smallest draw margin %.3g is below %.3g: change the seed" % (margin, need)
    out = call(X0, free, sweeps, seed=seed, beta=beta, random_start=randomize, first_chain=first_chain, first_sweep=first_sweep)
    assert out.shape == (n, L) and out.dtype == np.uint8
    clamped = np.setdiff1d(np.arange(L), free)
    assert np.array_equal(out[:, clamped], X0[:, clamped])
    assert np.array_equal(out, ref), int((out != ref).sum())
    return out


# ---------------------------------------------------------------- 1. all sites free: the plain sampler, bit for bit
@pytest.mark.parametrize("q,L", [(5, 23), (21, 37)])
@pytest.mark.parametrize("prec", [_lib.DCA_F32, _lib.DCA_F64])
def test_plm_all_sites_free_is_the_plain_sampler(q, L, prec):
    ctx, _h, _Jp = plm_context(L, q, prec, 10 * q + prec)
    n = 130
    X0 = backgrounds(n, L, q, 1)
    every = np.arange(L)
    for beta in (1.0, 0.6):
        plain = ctx.plm_sample(n, 4, seed=31, beta=beta, first_chain=5, first_sweep=2)
        assert np.array_equal(ctx.plm_sample_conditional(X0, every, 4, seed=31, beta=beta, random_start=True, first_chain=5,
                                                         first_sweep=2), plain)
        plain = ctx.plm_sample(n, 4, seed=31, beta=beta, initial=X0, first_chain=5, first_sweep=2)
        assert np.array_equal(ctx.plm_sample_conditional(X0, every, 4, seed=31, beta=beta, random_start=False, first_chain=5,
                                                         first_sweep=2), plain)
    ctx.close()


def test_mf_all_sites_free_is_the_plain_sampler():
    ctx, h, _Jp, X = mf_context("mf_toy_protein")
    L = h.shape[0]
    n = 130
    X0 = X[np.arange(n) % X.shape[0]]
    every = np.arange(L)
    assert np.array_equal(ctx.mf_sample_conditional(X0, every, 4, seed=8, random_start=True), ctx.mf_sample(n, 4, seed=8))
    assert np.array_equal(ctx.mf_sample_conditional(X0, every, 4, seed=8, beta=0.5, random_start=False, first_sweep=3),
                          ctx.mf_sample(n, 4, seed=8, beta=0.5, initial=X0, first_sweep=3))
    ctx.close()


# ---------------------------------------------------------------- 2. exact codes at the kernels' edges
# (free sites, chains, randomize) per model; L = 40: position 0 and L - 1, chunk firsts and lasts, one clamped site
def edge_lists(L, CJ):
    mid = list(range(12, 12 + CJ))
    return [([0], 65, True), ([L - 1], 1, False), ([0, L - 1], 63, True), ([5, 6, 30], 64, True), (mid, 65, False),
            ([0] + mid[:-1] + [L - 1], 65, True), ([j for j in range(L) if j != 20], 63, True)]


@pytest.mark.parametrize("prec,CJ", [(_lib.DCA_F32, 16), (_lib.DCA_F64, 8)])
def test_plm_q21_edges(prec, CJ):
    L, q = 40, 21
    ctx, h, Jp = plm_context(L, q, prec, 400 + prec)
    for k, (free, n, randomize) in enumerate(edge_lists(L, CJ)):
        check_against_restatement(ctx.plm_sample_conditional, h, Jp, backgrounds(n, L, q, k), free, 3, seed=100 + k,
                                  beta=(1.0, 0.5, 2.0)[k % 3], randomize=randomize, first_chain=7 * k, first_sweep=k)
    ctx.close()


def test_plm_q5_chunk_of_256():
    """F = CJ and CJ + 1 at q = 5 (float32), and two free sites with 298 clamped ones (three chunks of the field pass)"""
    L, q = 300, 5
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F32, 300, sigma=0.1, N=16)
    for k, free in enumerate((list(range(20, 276)), list(range(0, 256)) + [L - 1], [128, 255])):
        check_against_restatement(ctx.plm_sample_conditional, h, Jp, backgrounds(65, L, q, k), free, 3, seed=50 + k)
    ctx.close()


def test_plm_q5_float64_edges():
    L, q = 23, 5
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F64, 23)
    for k, (free, n) in enumerate((([11], 1), ([0, 22], 63), ([1, 2, 3, 5, 8, 13, 21], 65), (list(range(1, 23)), 64))):
        check_against_restatement(ctx.plm_sample_conditional, h, Jp, backgrounds(n, L, q, k), free, 4, seed=70 + k, beta=0.7,
                                  randomize=bool(k % 2))
    ctx.close()


def test_free_codes_beyond_lds():
    """520 free sites: their codes stay in the site-major state buffer"""
    L, q = 600, 5
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F32, 600, sigma=0.05, N=16)
    free = np.setdiff1d(np.arange(L), np.arange(3, 600, 7)[:80])
    assert free.size == 520 and free[0] == 0 and free[-1] == L - 1
    check_against_restatement(ctx.plm_sample_conditional, h, Jp, backgrounds(64, L, q, 0), free, 2, seed=3)
    ctx.close()


def test_free_codes_beyond_lds_float64():
    """the same list over a float64 model: the sweep kernel's other element type with the codes and the list in global memory"""
    L, q = 600, 5
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F64, 601, sigma=0.05, N=16)
    free = np.setdiff1d(np.arange(L), np.arange(3, 600, 7)[:80])
    check_against_restatement(ctx.plm_sample_conditional, h, Jp, backgrounds(64, L, q, 1), free, 2, seed=4)
    ctx.close()


@pytest.mark.parametrize("q,L", [(2, 12), (32, 10)])
def test_smallest_and_largest_alphabet(q, L):
    ctx, h, Jp = mf_random_context(L, q, 5)
    for k, (free, n) in enumerate((([0], 65), ([L - 1], 1), ([0, 3, 4, 5, L - 1], 63), ([j for j in range(L) if j != 4], 65))):
        check_against_restatement(ctx.mf_sample_conditional, h, Jp, backgrounds(n, L, q, k), free, 4, seed=20 + k, randomize=bool(k % 2),
                                  first_chain=k)
    ctx.close()


@pytest.mark.parametrize("tag", ["mf_toy_protein", "mf_toy_rna"])
def test_mf_goldens(tag):
    """the gap state's zero row and column"""
    ctx, h, Jp, X = mf_context(tag)
    L, q = h.shape
    n = 65
    X0 = X[(3 * np.arange(n)) % X.shape[0]]
    for k, free in enumerate(([0], [1, L - 1], list(range(1, L, 2)), list(range(L - 1)))):
        check_against_restatement(ctx.mf_sample_conditional, h, Jp, X0, free, 4, seed=40 + k, beta=(1.0, 0.5)[k % 2],
                                  randomize=bool(k % 2), first_sweep=2)
    ctx.close()


# ---------------------------------------------------------------- 3. invariances
def test_batch_pass_and_continuation_invariance(monkeypatch):
    L, q = 40, 21
    ctx, _h, _Jp = plm_context(L, q, _lib.DCA_F32, 5)
    free = [0] + list(range(12, 27)) + [L - 1]
    n = 200
    X0 = backgrounds(n, L, q, 9)
    full = ctx.plm_sample_conditional(X0, free, 5, seed=42, beta=0.8)
    a = ctx.plm_sample_conditional(X0[:77], free, 5, seed=42, beta=0.8)
    b = ctx.plm_sample_conditional(X0[77:], free, 5, seed=42, beta=0.8, first_chain=77)
    assert np.array_equal(np.vstack([a, b]), full)
    for k in (0, 63, 64, 199):
        assert np.array_equal(ctx.plm_sample_conditional(X0[k:k + 1], free, 5, seed=42, beta=0.8, first_chain=k)[0], full[k]), k
    ctx.set_profiling(True)
    monkeypatch.setenv("DCA_COND_PASS", "64")                   # four blocks of chains, one after another
    assert np.array_equal(ctx.plm_sample_conditional(X0, free, 5, seed=42, beta=0.8), full)
    assert ctx.kernel_time("cond_fields")[1] == 4 and ctx.kernel_time("sample_cond")[1] == 20
    monkeypatch.delenv("DCA_COND_PASS")
    ctx.reset_kernel_times()
    two = ctx.plm_sample_conditional(X0, free, 2, seed=42, beta=0.8)
    assert ctx.kernel_time("cond_fields")[1] == 1 and ctx.kernel_time("sample_cond")[1] == 2
    assert ctx.kernel_time("sample")[1] == 0                  # the plain sweep is not what runs
    assert np.array_equal(ctx.plm_sample_conditional(two, free, 3, seed=42, beta=0.8, random_start=False, first_sweep=2), full)
    ctx.close()


# ---------------------------------------------------------------- 4. the conditional distribution
def planted_alignment(L, q, N, seed):
    """neighbouring columns agree three times out of four: couplings strong enough that the context matters"""
    rng = np.random.default_rng(seed)
    X = np.zeros((N, L), dtype=np.uint8)
    X[:, 0] = rng.integers(0, q, N)
    for i in range(1, L):
        X[:, i] = np.where(rng.random(N) < 0.75, X[:, i - 1], rng.integers(0, q, N))
    return X


def test_distribution_given_two_contexts():
    """L = 5, q = 3 in float64, sites 1 and 3 clamped to two contexts, the 27 states of the free sites against the exact conditional
    distribution.  The model is a mean-field one: dca_plm_configure takes q = 5 and q = 21 only, so no plm vector has q = 3."""
    L, q, n, half = 5, 3, 16384, 8192
    ctx = _lib.Context(0, _lib.DCA_F64)
    ctx.set_msa(planted_alignment(L, q, 300, 1), q)
    ctx.compute_weights(0.8, _lib.DCA_F64)
    ctx.mf_corr_mat(0.5, want=False)
    ctx.mf_couplings()
    free, fixed = [0, 2, 4], [1, 3]
    contexts = ((0, 0), (2, 1))
    states = np.array(np.unravel_index(np.arange(q ** L), (q,) * L)).T.astype(np.uint8)
    E = ctx.mf_energies(states)
    exact = []
    for cx in contexts:
        rows = np.flatnonzero((states[:, fixed] == np.array(cx, dtype=np.uint8)).all(axis=1))
        assert rows.size == 27 and np.array_equal(np.ravel_multi_index(states[rows][:, free].T.astype(np.int64), (q,) * 3), np.arange(27))
        w = np.exp(E[rows] - E[rows].max())
        exact.append(w / w.sum())
    # the two contexts differ by far more than the test below can miss
    assert _g_test(half * exact[0], half * exact[1]) < 1e-12 and _g_test(half * exact[1], half * exact[0]) < 1e-12
    X0 = np.zeros((n, L), dtype=np.uint8)
    X0[:half, fixed], X0[half:, fixed] = contexts[0], contexts[1]
    out = ctx.mf_sample_conditional(X0, free, 50, seed=2025)
    assert np.array_equal(out[:, fixed], X0[:, fixed])
    for k, rows in enumerate((slice(0, half), slice(half, n))):
        idx = np.ravel_multi_index(out[rows][:, free].T.astype(np.int64), (q,) * 3)
        counts = np.bincount(idx, minlength=27).astype(np.float64)
        p = _g_test(counts, half * exact[k])
        print("context %r: G-test p = %.3g" % (contexts[k], p))
        assert p > 1e-6, (k, p)
        assert _g_test(counts, half * exact[1 - k]) < 1e-6
    ctx.close()


# ---------------------------------------------------------------- 5. state untouched
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
    ctx.plm_sample_conditional(X[np.arange(300) % X.shape[0]], [1, 4, 5, 8], 3, seed=5)
    ctx.plm_sample_conditional(X[:64], np.arange(X.shape[1]), 2, seed=5, random_start=False)
    assert ctx.plm_get_x(np.float32).tobytes() == x0.tobytes()
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.weights().tobytes() == w0.tobytes()
    assert ctx.plm_energies(X[:50]).tobytes() == E0.tobytes()
    assert ctx.plm_bm_iterate(1).tobytes() == rec_ref.tobytes()
    assert ctx.plm_get_x(np.float32).tobytes() == x_ref.tobytes()
    assert np.array_equal(ctx.plm_bm_chains(), ch_ref)
    ctx.close()
    mctx, _h, _Jp, MX = mf_context()
    J0 = mctx.mf_couplings()
    mctx.mf_sample_conditional(MX[:100], [0, 2], 3, seed=1)
    assert mctx.mf_couplings().tobytes() == J0.tobytes()
    mctx.close()


# ---------------------------------------------------------------- 6. errors
def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def _raw(ctx, fn, n=2, sweeps=1, beta=1.0, sites=(1, 3), F=None, initial=True, out=True, X0=None):
    L = ctx.L
    s = np.asarray([] if sites is None else sites, dtype=np.int32)
    X0 = np.zeros((max(n, 1), L), dtype=np.uint8) if X0 is None else X0
    o = np.zeros((max(n, 1), L), dtype=np.uint8)
    return fn(ctx._h, n, sweeps, 0, 0, 0, beta, s.ctypes.data if sites is not None else None, s.size if F is None else F,
              X0.ctypes.data if initial else None, 1, o.ctypes.data if out else None)


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    lib = _lib.lib()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_sample_conditional(X[:4], [1], 1)) == _lib.DCA_ERR_STATE          # before dca_plm_configure
    assert _code(lambda: ctx.mf_sample_conditional(X[:4], [1], 1)) == _lib.DCA_ERR_STATE           # before the mf couplings
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    fn = lib.dca_plm_sample_conditional
    assert _raw(ctx, fn) == _lib.DCA_OK
    bad = np.zeros((2, L), dtype=np.uint8)
    bad[1, 3] = q
    for kw in (dict(n=-1), dict(sweeps=-1), dict(beta=-0.5), dict(beta=float("nan")), dict(beta=float("inf")), dict(initial=False),
               dict(out=False), dict(F=-1), dict(sites=list(range(L)) + [0], F=L + 1), dict(sites=None, F=2), dict(sites=(1, L)),
               dict(sites=(-1, 2)), dict(sites=(3, 1)), dict(sites=(2, 2)), dict(X0=bad)):
        assert _raw(ctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    assert _raw(ctx, fn, n=0, initial=False, out=False) == _lib.DCA_OK
    assert _raw(ctx, fn, sites=None, F=0) == _lib.DCA_OK
    assert ctx.plm_sample_conditional(np.zeros((0, L), dtype=np.uint8), [1], 3).shape == (0, L)
    X70 = X[np.arange(70) % X.shape[0]]
    assert np.array_equal(ctx.plm_sample_conditional(X70, [], 3), X70)                            # F = 0: the start
    assert np.array_equal(ctx.plm_sample_conditional(X70, [2, 5], 0, random_start=False), X70)
    start = ctx.plm_sample_conditional(X70, [2, 5], 0, seed=5, first_chain=3)                      # sweeps = 0: the random start
    want = X70.copy()
    want[:, [2, 5]] = ctx.plm_sample(70, 0, seed=5, first_chain=3)[:, [2, 5]]
    assert np.array_equal(start, want)
    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert ctx.plm_sample_conditional(X[:4], [1, 2], 2).shape == (4, L)                            # allowed during an L-BFGS run
    ctx.plm_lbfgs_end()
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_sample_conditional(X[:4], [1], 1)) == _lib.DCA_ERR_STATE          # one GPU only
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_sample_conditional(X[:4], [1], 1)) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)
    assert ctx.plm_sample_conditional(X[:4], [1], 1).shape == (4, L)
    ctx.close()
    mctx, _h, _Jp, MX = mf_context("mf_toy_rna")
    fn = lib.dca_mf_sample_conditional
    assert _raw(mctx, fn) == _lib.DCA_OK
    bad = np.zeros((2, MX.shape[1]), dtype=np.uint8)
    bad[0, 0] = 5
    for kw in (dict(n=-1), dict(beta=-1.0), dict(sites=(1, 1)), dict(sites=(0, MX.shape[1])), dict(initial=False), dict(X0=bad)):
        assert _raw(mctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    mctx.close()


# ---------------------------------------------------------------- 7. classes and command lines
def _read_conditional(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("# Conditional Gibbs samples") and lines[1].startswith("# Free sites (1-based): ")
    heads = [ln for ln in lines if ln.startswith(">")]
    assert [h.split()[0] for h in heads] == [">sample_%d" % (k + 1) for k in range(len(heads))]
    free = [int(v) - 1 for v in lines[1].split(": ")[1].split(",")]
    return fasta_reader.get_alignment_from_fasta_file(path), np.array([float(h.split("energy=")[1]) for h in heads]), free


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    templates = [s.replace(".", "-").replace("~", "-") for s in seqs[:6]]
    S = inst.sample_sequences_conditional(templates, free_sites=[7, 2, 3], num_sweeps=20, seed=4)
    assert len(S) == 6 and all(len(s) == 10 and set(s) <= set("ACGU-") for s in S)
    fixed = [0, 1, 4, 5, 6, 8, 9]
    assert all("".join(s[j] for j in fixed) == "".join(t[j] for j in fixed) for s, t in zip(S, templates))
    assert inst.sample_sequences_conditional(templates, fixed_sites=fixed, num_sweeps=20, seed=4) == S
    codes = inst.sample_sequences_conditional(templates, free_sites=[2, 3, 7], num_sweeps=20, seed=4, return_codes=True)
    assert codes.shape == (6, 10) and ["".join("ACGU-"[c] for c in row) for row in codes] == S
    assert inst.sample_sequences_conditional(templates[0], free_sites=[2], num_sequences=3, num_sweeps=0, randomize=False) == [templates[0]] * 3
    every = inst.sample_sequences_conditional(templates[0], fixed_sites=[], num_sequences=40, num_sweeps=10, seed=4)
    assert every == inst.sample_sequences(40, num_sweeps=10, seed=4)               # nothing clamped: the plain sampler
    with pytest.raises(PlmDCAException, match="twice"):
        inst.sample_sequences_conditional(templates, free_sites=[1, 1])
    tf = tmp_path / "templates.fa"
    tf.write_text("".join(">t%d\n%s\n" % (k, t) for k, t in enumerate(templates)))
    out = str(tmp_path / "plm_out")
    f = plmdca_main.run_plm_dca(["sample_conditional", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                 "--output_dir", out, "--template_file", str(tf), "--free_sites", "8,3-4", "--num_sweeps", "20",
                                 "--seed", "4"])
    assert os.path.basename(f) == "PLMDCA_conditional_samples_toy_rna.fa"
    got, E, free = _read_conditional(f)
    assert free == [2, 3, 7] and len(got) == 6 and np.all(np.isfinite(E))
    assert all("".join(s[j] for j in fixed) == "".join(t[j] for j in fixed) for s, t in zip(got, templates))
    assert got == PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5).sample_sequences_conditional(
        str(tf), free_sites=[2, 3, 7], num_sweeps=20, seed=4)


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    L = inst.sequences_len
    letters = _potts.state_letters(_lib.DCA_BIOMOLECULE_PROTEIN)
    template = "".join(letters[c] for c in _lib.encode_sequences([seqs[1]], _lib.DCA_BIOMOLECULE_PROTEIN, L, 1)[0])
    free = [0, L // 2, L - 1]
    fixed = [j for j in range(L) if j not in free]
    S = inst.sample_sequences_conditional(template, free_sites=free, num_sequences=30, num_sweeps=15, seed=9)   # the couplings are computed here
    assert len(S) == 30 and all(len(s) == L and set(s) <= set(letters) for s in S)
    assert all("".join(s[j] for j in fixed) == "".join(template[j] for j in fixed) for s in S)
    assert len(set(S)) > 1
    with pytest.raises(MeanFieldDCAException, match="records"):
        inst.sample_sequences_conditional(seqs[:2], free_sites=free, num_sequences=3)
    tf = tmp_path / "template.fa"
    tf.write_text(">t\n{}\n".format(template))
    out = str(tmp_path / "mf_out")
    f = mfdca_main.run_meanfield_dca(["sample_conditional", "protein", path, "--output_dir", out, "--template_file", str(tf),
                                      "--fixed_sites", "2-%d,%d-%d" % (L // 2, L // 2 + 2, L - 1), "--num_sequences", "8",
                                      "--num_sweeps", "6", "--keep_template_start"])
    assert os.path.basename(f) == "MFDCA_conditional_samples_toy_protein.fa"
    got, E, freed = _read_conditional(f)
    assert freed == free and len(got) == 8
    assert all("".join(s[j] for j in fixed) == "".join(template[j] for j in fixed) for s in got)
    assert np.allclose(E, inst.compute_sequence_energies(got), rtol=1e-12, atol=1e-12)
