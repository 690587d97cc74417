"""Greedy ascent on the GPU (dca_plm_ascend, dca_mf_ascend, find_local_maxima and the find_local_maxima sub-command; DESIGN.md
section 24) against the float64 restatement of tests/ascent_reference.py, bit for bit: codes, steps, converged, path, gains.

The plm models are the stored vectors tests/test_ascent_host.py checks the margin rule on; an mf model lives on the device, so
this file reads it back and checks the rule on that.  Every case runs with the table in LDS and again with DCA_ASCENT_LDS=0 (the
table in device memory).  The certificate tests use nothing of the new code but its output: the mutation scan and the energies.

Bounds (u = 2^-53, gamma(k) = k u / (1 - k u), Sabs = potts_audit_reference.model_sabs, an upper bound of sum|terms| of any
site sum):
  * a table entry after t steps is a sum of at most L + 2 t terms, so a gain is off by at most gamma(t + L + 3) Sabs against the
    mutation scan's own two sums (bounded alike): no free-site entry of the scan of a converged output may exceed
    min_gain + gamma(steps + L + 3) Sabs;
  * E_final - E_start against `gains`: two energies, each within gamma(L + L (L - 1) / 2 + 128) Eabs of the exact one (at most
    128 slabs; Eabs = sum_i max|h_i| + sum_{i<j} max|J_ij|), the difference's rounding u |E|, every applied gain within
    2 gamma(steps + L + 3) Sabs, and the sequential sum of the gains within gamma(steps) sum|g|."""
import os

import numpy as np
import pytest

import ascent_reference as R
from conftest import data_file, golden
from plm_eval_reference import gamma
from potts_audit_reference import U, model_sabs
from pydca_amd import _lib, _potts, mfdca_main, plmdca_main
from pydca_amd.fasta_reader import fasta_reader
from pydca_amd.meanfield_dca.meanfield_dca import MeanFieldDCA
from pydca_amd.plmdca.plmdca import PlmDCA, PlmDCAException

pytestmark = pytest.mark.gpu


class Case:
    """a model on the device with its restated (h, Jp), its starts and the references computed so far"""

    def __init__(self, m):
        self.m, self.refs = m, {}
        if m[0] == "plm":
            _, q, L, bits = m
            prec = _lib.DCA_F32 if bits == 32 else _lib.DCA_F64
            dt = np.float32 if bits == 32 else np.float64
            self.ctx = _lib.Context(0, prec)
            self.ctx.set_msa(R.plm_alignment(q, L), q)
            self.ctx.compute_weights(0.8, prec)
            self.ctx.plm_configure(1.0, 1.0)
            self.ctx.plm_set_x(R.plm_x(q, L, bits))
            self.h, self.Jp = R.plm_model(self.ctx.plm_get_x(dt), L, q)
            self.X = R.starts(R.N_CHAINS, L, q, 0)
            self.ascend, self.energies, self.scan = self.ctx.plm_ascend, self.ctx.plm_energies, self.ctx.plm_mutation_scan
            h, Jp, _X = R.cpu_model(m)
            assert np.array_equal(h, self.h) and np.array_equal(Jp, self.Jp)      # the model of the host file's margin check
            self.margins_checked = True
        else:
            if m[0] == "mf":
                _, q, L = m
                A, w = R.mf_alignment(q, L)
                self.X = R.starts(R.N_CHAINS, L, q, 0)
            else:
                A, q = R.golden_alignment(m[1])
                L, w = A.shape[1], None
                self.X = R.golden_starts(A, R.N_CHAINS)
            self.ctx = _lib.Context(0, _lib.DCA_F64)
            self.ctx.set_msa(A, q)
            if w is None:
                self.ctx.compute_weights(0.8, _lib.DCA_F64)
            else:
                self.ctx.set_weights(w)
            self.ctx.mf_corr_mat(0.5, want=False)
            self.h, self.Jp = R.mf_model(self.ctx.mf_couplings(), self.ctx.mf_fields(), L, q)
            self.ascend, self.energies, self.scan = self.ctx.mf_ascend, self.ctx.mf_energies, self.ctx.mf_mutation_scan
            self.margins_checked = False
        self.L, self.q = L, q

    def ref(self, free, max_steps, min_gain=0.0, X=None):
        """the restatement of the case's starts (computed once per argument set) or of other rows"""
        if X is not None:
            return R.ascend(self.h, self.Jp, X, free, max_steps, min_gain)
        key = (tuple(int(v) for v in free), max_steps, min_gain)
        if key not in self.refs:
            if not self.margins_checked:
                margin, drift = R.check_margins(self.h, self.Jp, self.X, np.asarray(free), max_steps, min_gain)
                print("%s, F %d: margin %.3g, drift %.3g on the device's model" % (R.model_id(self.m), len(free), margin, drift))
            self.refs[key] = R.ascend(self.h, self.Jp, self.X, free, max_steps, min_gain)
        return self.refs[key]


@pytest.fixture(scope="module", params=R.MODELS, ids=R.model_id)
def case(request):
    c = Case(request.param)
    yield c
    c.ctx.close()


def same_bits(got, ref, rows=slice(None)):
    assert np.array_equal(got["codes"], ref["codes"][rows])
    assert np.array_equal(got["steps"], ref["steps"][rows])
    assert np.array_equal(got["converged"], ref["converged"][rows])
    assert got["gains"].tobytes() == np.ascontiguousarray(ref["gains"][rows]).tobytes()
    if "path" in got:
        assert np.array_equal(got["path"], ref["path"][rows])
        assert got["path_gains"].tobytes() == np.ascontiguousarray(ref["path_gains"][rows]).tobytes()


def both_tables(monkeypatch, fn):
    """fn() with the table in LDS and with it in device memory"""
    monkeypatch.delenv("DCA_ASCENT_LDS", raising=False)
    fn()
    monkeypatch.setenv("DCA_ASCENT_LDS", "0")
    fn()
    monkeypatch.delenv("DCA_ASCENT_LDS")


# ---------------------------------------------------------------- 1. the same bits as the restatement
def test_every_site_list(case, monkeypatch):
    """F = L, 1, 2 and 0, free sites at 0 and L - 1, one clamped site; n = 1, 63 and 65; a different row per chain"""
    L = case.L
    for free in R.site_lists(L):
        ref = case.ref(free, 4 * free.size)
        clamped = np.setdiff1d(np.arange(L), free)

        def run():
            for n in ((1, 63, 65) if free.size == L else (65,)):
                got = case.ascend(case.X[:n], free, paths=True)
                same_bits(got, ref, slice(0, n))
                assert np.array_equal(got["codes"][:, clamped], case.X[:n, clamped])
            same_bits(case.ascend(case.X[:7], free), ref, slice(0, 7))          # without the optional outputs
        both_tables(monkeypatch, run)
        if free.size:
            assert ref["converged"].all()
        if free.size == L:
            assert ref["steps"].max() > 0


def test_step_caps_min_gain_and_restart(case, monkeypatch):
    """max_steps = 0, 1 and exactly a chain's step count (converged there, not one step earlier); min_gain above every gain; a
    start that is a previous output"""
    L = case.L
    free = np.arange(L)
    full = case.ref(free, 4 * L)
    k = int(np.argmax(full["steps"]))
    T = int(full["steps"][k])
    assert T >= 1
    rows = case.X[[k, 0, 1]]

    def run():
        for cap in sorted({0, 1, T - 1, T}):
            got = case.ascend(rows, free, max_steps=cap, paths=True)
            same_bits(got, case.ref(free, cap, X=rows))
            assert got["steps"][0] == cap and bool(got["converged"][0]) == (cap == T)
            assert got["path"].shape == (3, cap, 2) and np.array_equal(got["path"][0], full["path"][k, :cap])
        assert np.array_equal(case.ascend(rows, free, max_steps=0)["codes"], rows)
        high = case.ascend(case.X[:9], free, min_gain=1e6, paths=True)
        assert np.array_equal(high["codes"], case.X[:9]) and not high["steps"].any() and high["converged"].all()
        assert not high["gains"].any() and (high["path"] == -1).all() and not high["path_gains"].any()
        again = case.ascend(full["codes"], free, paths=True)
        assert np.array_equal(again["codes"], full["codes"]) and not again["steps"].any() and again["converged"].all()
    both_tables(monkeypatch, run)


# ---------------------------------------------------------------- 2. the certificate, independent of the new code
def test_certificate(case):
    L, q = case.L, case.q
    free = np.setdiff1d(np.arange(L), [L // 2]) if L > 2 else np.arange(L)
    n = 12
    X = case.X[:n]
    sabs = model_sabs(case.h, case.Jp)
    iu, ju = np.triu_indices(L, 1)
    eabs = np.abs(case.h).max(axis=1).sum() + (np.abs(case.Jp).max(axis=(1, 2)).sum() if iu.size else 0.0)
    bound_e = gamma(L + L * (L - 1) // 2 + 128, U) * eabs
    for min_gain in (0.0, 0.25):
        got = case.ascend(X, free, min_gain=min_gain, paths=True)
        assert got["converged"].all()
        for k in range(n):                                      # no single mutation of a free site gains more than min_gain
            dE = case.scan(got["codes"][k])
            assert dE[free].max() <= min_gain + gamma(int(got["steps"][k]) + L + 3, U) * sabs, k
        seqs, owner = [], []
        for k in range(n):                                      # the sequences along every path
            s = X[k].copy()
            seqs.append(s.copy())
            owner.append(k)
            for i, a in got["path"][k, :got["steps"][k]]:
                s[i] = a
                seqs.append(s.copy())
                owner.append(k)
            assert np.array_equal(s, got["codes"][k])
        E = case.energies(np.array(seqs, dtype=np.uint8))
        owner = np.array(owner)
        for k in range(n):
            Ek = E[owner == k]
            t = int(got["steps"][k])
            assert Ek.size == t + 1 and np.all(np.diff(Ek) > 0), k    # the existing energy entry increases strictly along the path
            tol = 2 * bound_e + U * abs(Ek[-1] - Ek[0]) + 2 * t * gamma(t + L + 3, U) * sabs + gamma(max(t, 1), U) * np.abs(got["path_gains"][k]).sum()
            assert abs((Ek[-1] - Ek[0]) - got["gains"][k]) <= tol, (k, Ek[-1] - Ek[0], got["gains"][k], tol)


# ---------------------------------------------------------------- 3. ties and more than one position per thread
def test_site_and_state_ties_across_the_workgroup(monkeypatch):
    """L = 300 sites with the same fields and no couplings (float32 values: every sum exact), all chains at one code: every site
    ties, the smallest wins, then the smallest state among the two best; positions 256 .. 299 are a thread's second."""
    L, q = 300, 5
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(np.random.default_rng(1).integers(0, q, size=(16, L), dtype=np.uint8), q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    ctx.plm_configure(1.0, 1.0)
    x = np.zeros(ctx.num_params(), dtype=np.float32)
    x[:L * q] = np.tile(np.array([0.25, 1.5, -0.5, 1.5, 0.0], dtype=np.float32), L)
    ctx.plm_set_x(x)
    h, Jp = R.plm_model(x, L, q)
    X = np.zeros((3, L), dtype=np.uint8)
    X[1, ::2] = 2
    X[2] = np.random.default_rng(2).integers(0, q, L)
    free = np.concatenate([np.arange(3, 130), np.arange(140, L)])

    def run():
        for sites in (np.arange(L), free):
            ref = R.ascend(h, Jp, X, sites, 4 * sites.size)
            got = ctx.plm_ascend(X, sites, paths=True)
            same_bits(got, ref)
            moved = sites[X[0, sites] != 1]
            assert np.array_equal(got["path"][0, :moved.size, 0], moved) and (got["path"][0, :moved.size, 1] == 1).all()
        cut = ctx.plm_ascend(X, np.arange(L), max_steps=270, paths=True)
        same_bits(cut, R.ascend(h, Jp, X, np.arange(L), 270))
        assert cut["steps"][0] == 270 and not cut["converged"][0]
    both_tables(monkeypatch, run)
    ctx.close()


# ---------------------------------------------------------------- 4. invariances
def test_batch_halves_and_passes(monkeypatch):
    c = Case(("plm", 21, 37, 32))
    ctx, L, q = c.ctx, c.L, c.q
    n = 150
    X = R.starts(n, L, q, 3)
    free = np.setdiff1d(np.arange(L), [4, 30])
    full = ctx.plm_ascend(X, free, paths=True)
    a, b = ctx.plm_ascend(X[:77], free, paths=True), ctx.plm_ascend(X[77:], free, paths=True)
    for key in full:
        assert np.array_equal(np.concatenate([a[key], b[key]]), full[key]), key
    one = ctx.plm_ascend(X[149:], free, paths=True)
    for key in full:
        assert np.array_equal(one[key][0], full[key][149]), key
    ctx.set_profiling(True)
    monkeypatch.setenv("DCA_ASCENT_PASS", "64")                 # three blocks of chains, one after another
    split = ctx.plm_ascend(X, free, paths=True)
    for key in full:
        assert np.array_equal(split[key], full[key]), key
    assert ctx.kernel_time("ascent_init")[1] == 3 and ctx.kernel_time("ascent")[1] == 3
    monkeypatch.delenv("DCA_ASCENT_PASS")
    ctx.reset_kernel_times()
    ctx.plm_ascend(X, free)
    assert ctx.kernel_time("ascent_init")[1] == 1 and ctx.kernel_time("ascent")[1] == 1       # one launch runs every step
    monkeypatch.setenv("DCA_ASCENT_LDS", "1000")                # 36 x 21 x 8 bytes do not fit under this cap, 5 x 21 x 8 do
    capped = ctx.plm_ascend(X, free, paths=True)
    for key in full:
        assert np.array_equal(capped[key], full[key]), key
    same_bits(ctx.plm_ascend(X[:20], [1, 2, 3, 5, 8], paths=True), R.ascend(c.h, c.Jp, X[:20], [1, 2, 3, 5, 8], 20))
    ctx.close()


# ---------------------------------------------------------------- 5. state untouched, ownership
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
    ctx.plm_ascend(X[np.arange(300) % X.shape[0]], [1, 4, 5, 8])
    ctx.plm_ascend(X[:64], np.arange(X.shape[1]), paths=True)
    assert ctx.plm_get_x(np.float32).tobytes() == x0.tobytes()
    assert ctx.plm_get_g(np.float32).tobytes() == g0.tobytes()
    assert ctx.weights().tobytes() == w0.tobytes()
    assert ctx.plm_energies(X[:50]).tobytes() == E0.tobytes()
    assert ctx.plm_bm_iterate(1).tobytes() == rec_ref.tobytes()
    assert ctx.plm_get_x(np.float32).tobytes() == x_ref.tobytes()
    assert np.array_equal(ctx.plm_bm_chains(), ch_ref)
    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert ctx.plm_ascend(X[:4], [1, 2])["codes"].shape == (4, X.shape[1])                      # allowed during an L-BFGS run
    ctx.plm_lbfgs_end()
    ctx.close()


def test_blocks_in_use_balance(monkeypatch):
    """test_device_ownership's check for the new entry: a second call leaves as many blocks in use as the first, a pass loop and
    a failing call give back what they took, and the closed context gives everything back"""
    L, q = 12, 5
    rng = np.random.default_rng(7)
    A = rng.integers(0, q, size=(60, L), dtype=np.uint8)
    Q = np.ascontiguousarray(rng.integers(0, q, size=(40, L), dtype=np.uint8))
    before = _lib.device_blocks_in_use()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(A, q)
    ctx.compute_weights(0.8)
    ctx.mf_run(0.5, True)
    ctx.mf_fields()
    ctx.plm_configure(1.0, 2.0)
    ctx.plm_init_x()
    ctx.plm_set_x((0.05 * rng.standard_normal(ctx.num_params())).astype(np.float32))
    for name, fn in (("plm_ascend", lambda: ctx.plm_ascend(Q, [0, 3, 11], paths=True)), ("mf_ascend", lambda: ctx.mf_ascend(Q, np.arange(L))),
                     ("plm_ascend with F = 0", lambda: ctx.plm_ascend(Q, []))):
        fn()
        first = _lib.device_blocks_in_use()
        fn()
        assert _lib.device_blocks_in_use() == first, name
    whole = _lib.device_blocks_in_use()
    monkeypatch.setenv("DCA_ASCENT_PASS", "16")
    ctx.plm_ascend(Q, np.arange(L), paths=True)
    assert _lib.device_blocks_in_use() == whole
    monkeypatch.delenv("DCA_ASCENT_PASS")
    bad = Q.copy()
    bad[33, L - 1] = q
    for fn in (ctx.plm_ascend, ctx.mf_ascend):
        with pytest.raises(_lib.DcaBackendError) as ei:
            fn(bad, [1, 2])
        assert ei.value.code == _lib.DCA_ERR_ARG
        with pytest.raises(_lib.DcaBackendError):
            fn(Q, [2, 1])
        assert _lib.device_blocks_in_use() == whole
    ctx.close()
    assert _lib.device_blocks_in_use() == before


# ---------------------------------------------------------------- 6. errors
def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def _raw(ctx, fn, n=2, sites=(1, 3), F=None, max_steps=4, min_gain=0.0, X=True, out=True, steps=True, conv=True, X0=None):
    L = ctx.L
    s = np.asarray([] if sites is None else sites, dtype=np.int32)
    X0 = np.zeros((max(n, 1), L), dtype=np.uint8) if X0 is None else X0
    o = np.zeros((max(n, 1), L), dtype=np.uint8)
    st = np.zeros(max(n, 1), dtype=np.int32)
    cv = np.zeros(max(n, 1), dtype=np.uint8)
    return fn(ctx._h, X0.ctypes.data if X else None, n, s.ctypes.data if sites is not None else None, s.size if F is None else F,
              max_steps, min_gain, o.ctypes.data if out else None, st.ctypes.data if steps else None, cv.ctypes.data if conv else None,
              None, None, None)


def test_argument_and_state_errors():
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    lib = _lib.lib()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_ascend(X[:4], [1])) == _lib.DCA_ERR_STATE          # before dca_plm_configure
    assert _code(lambda: ctx.mf_ascend(X[:4], [1])) == _lib.DCA_ERR_STATE           # before the mf couplings
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    fn = lib.dca_plm_ascend
    assert _raw(ctx, fn) == _lib.DCA_OK
    bad = np.zeros((2, L), dtype=np.uint8)
    bad[1, 3] = q
    for kw in (dict(n=-1), dict(max_steps=-1), dict(min_gain=-0.5), dict(min_gain=float("nan")), dict(min_gain=float("inf")),
               dict(X=False), dict(out=False), dict(steps=False), dict(conv=False), dict(F=-1), dict(sites=list(range(L)) + [0], F=L + 1),
               dict(sites=None, F=2), dict(sites=(1, L)), dict(sites=(-1, 2)), dict(sites=(3, 1)), dict(sites=(2, 2)), dict(X0=bad)):
        assert _raw(ctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    assert _raw(ctx, fn, n=0, X=False, out=False, steps=False, conv=False) == _lib.DCA_OK
    assert _raw(ctx, fn, sites=None, F=0) == _lib.DCA_OK                            # NULL + 0: no free site, not "all"
    assert ctx.plm_ascend(np.zeros((0, L), dtype=np.uint8), [1])["codes"].shape == (0, L)
    X70 = X[np.arange(70) % X.shape[0]]
    none = ctx.plm_ascend(X70, [], paths=True)
    assert np.array_equal(none["codes"], X70) and none["converged"].all() and not none["steps"].any() and none["path"].shape == (70, 0, 2)
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_ascend(X[:4], [1])) == _lib.DCA_ERR_STATE          # one GPU only
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_ascend(X[:4], [1])) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)
    assert ctx.plm_ascend(X[:4], [1])["codes"].shape == (4, L)
    ctx.close()
    M, mq = R.golden_alignment("mf_toy_rna")
    mctx = _lib.Context(0, _lib.DCA_F64)
    mctx.set_msa(M, mq)
    mctx.compute_weights(0.8, _lib.DCA_F64)
    mctx.mf_corr_mat(0.5, want=False)
    mctx.mf_couplings()
    fn = lib.dca_mf_ascend
    assert _raw(mctx, fn) == _lib.DCA_OK
    bad = np.zeros((2, M.shape[1]), dtype=np.uint8)
    bad[0, 0] = mq
    for kw in (dict(n=-1), dict(max_steps=-2), dict(min_gain=-1.0), dict(sites=(1, 1)), dict(sites=(0, M.shape[1])), dict(X=False), dict(X0=bad)):
        assert _raw(mctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    mctx.close()


# ---------------------------------------------------------------- 7. classes and command lines
def _check_result(res, inst, starts, free, L):
    n = len(starts)
    fixed = [j for j in range(L) if j not in free]
    assert len(res["sequences"]) == n and all(len(s) == L for s in res["sequences"])
    assert all("".join(s[j] for j in fixed) == "".join(t[j] for j in fixed) for s, t in zip(res["sequences"], starts))
    assert res["converged"].all() and res["num_steps"].shape == (n,)
    assert res["energies"].tobytes() == inst.compute_sequence_energies(res["sequences"]).tobytes()
    assert res["start_energies"].tobytes() == inst.compute_sequence_energies(starts).tobytes()
    assert np.all(res["energies"] >= res["start_energies"])
    assert np.all(res["energies"][res["num_steps"] == 0] == res["start_energies"][res["num_steps"] == 0])
    count = {}                                                  # basins against a plain dict count
    for s in res["sequences"]:
        count[s] = count.get(s, 0) + 1
    assert sorted(res["maxima"]) == sorted(count) and [count[s] for s in res["maxima"]] == res["basin_sizes"].tolist()
    assert [res["maxima"][b] for b in res["basin"]] == res["sequences"]
    first = [res["sequences"].index(s) for s in res["maxima"]]      # by descending energy, then lexicographic codes
    assert np.all(np.diff(res["energies"][first]) <= 0)


def _read_maxima(fa, txt):
    heads = [ln for ln in open(fa).read().splitlines() if ln.startswith(">")]
    assert [h.split()[0] for h in heads] == [">maximum_of_%d" % (k + 1) for k in range(len(heads))]
    rows = [ln.split() for ln in open(txt).read().splitlines() if not ln.startswith("#")]
    return fasta_reader.get_alignment_from_fasta_file(fa), np.array([float(h.split("energy=")[1]) for h in heads]), rows


def test_plm_class_and_cli(tmp_path):
    path = data_file("toy_rna.fa")
    seqs = [s.replace(".", "-").replace("~", "-") for s in fasta_reader.get_alignment_from_fasta_file(path)]
    inst = PlmDCA(path, "rna", seqid=0.8, lambda_h=1.8, lambda_J=1.8, max_iterations=5)
    L = 10
    res = inst.find_local_maxima()                              # the training alignment's rows, every site free
    _check_result(res, inst, seqs, list(range(L)), L)
    free = [2, 3, 7]
    part = inst.find_local_maxima(seqs[:6], free_sites=[7, 2, 3], return_paths=True)
    _check_result(part, inst, seqs[:6], free, L)
    assert inst.find_local_maxima(seqs[:6], fixed_sites=[0, 1, 4, 5, 6, 8, 9])["sequences"] == part["sequences"]
    for k, steps in enumerate(part["paths"]):                   # a path rebuilds its sequence
        s = list(seqs[k])
        for site, letter, gain in steps:
            assert site in free and gain > 0 and s[site] != letter
            s[site] = letter
        assert "".join(s) == part["sequences"][k] and len(steps) == part["num_steps"][k]
    capped = inst.find_local_maxima(seqs[:6], max_steps=0)
    assert capped["sequences"] == seqs[:6] and not capped["num_steps"].any()
    assert all(b == -1 for c, b in zip(capped["converged"], capped["basin"]) if not c) and not capped["converged"].all()
    assert inst.find_local_maxima(part["sequences"], free_sites=free)["num_steps"].tolist() == [0] * 6
    with pytest.raises(PlmDCAException, match="twice"):
        inst.find_local_maxima(seqs[:2], free_sites=[1, 1])
    qf = tmp_path / "starts.fa"
    qf.write_text("".join(">s%d\n%s\n" % (k, t) for k, t in enumerate(seqs[:6])))
    out = str(tmp_path / "plm_out")
    fa, txt = plmdca_main.run_plm_dca(["find_local_maxima", "rna", path, "--lambda_h", "1.8", "--lambda_J", "1.8", "--max_iterations", "5",
                                       "--output_dir", out, "--query_file", str(qf), "--free_sites", "8,3-4"])
    assert os.path.basename(fa) == "PLMDCA_local_maxima_toy_rna.fa" and os.path.basename(txt) == "PLMDCA_local_maxima_toy_rna.txt"
    got, E, rows = _read_maxima(fa, txt)
    assert got == part["sequences"] and E.tobytes() == part["energies"].tobytes()
    assert [int(r[3]) for r in rows] == part["num_steps"].tolist() and [int(r[4]) for r in rows] == [1] * 6
    assert [int(r[5]) - 1 for r in rows] == part["basin"].tolist()
    assert [float(r[1]) for r in rows] == part["start_energies"].tolist() and [float(r[2]) for r in rows] == part["energies"].tolist()


def test_mf_class_and_cli(tmp_path):
    path = data_file("toy_protein.fa")
    seqs = fasta_reader.get_alignment_from_fasta_file(path)
    inst = MeanFieldDCA(path, "protein")
    L = inst.sequences_len
    letters = _potts.state_letters(_lib.DCA_BIOMOLECULE_PROTEIN)
    starts = ["".join(letters[c] for c in row) for row in _lib.encode_sequences(seqs[:8], _lib.DCA_BIOMOLECULE_PROTEIN, L, 1)]
    free = [0, L // 2, L - 1]
    res = inst.find_local_maxima(starts, free_sites=free)       # the couplings are computed here
    _check_result(res, inst, starts, free, L)
    every = inst.find_local_maxima(starts)
    _check_result(every, inst, starts, list(range(L)), L)
    qf = tmp_path / "starts.fa"
    qf.write_text("".join(">s%d\n%s\n" % (k, t) for k, t in enumerate(starts)))
    out = str(tmp_path / "mf_out")
    fa, txt = mfdca_main.run_meanfield_dca(["find_local_maxima", "protein", path, "--output_dir", out, "--query_file", str(qf),
                                            "--fixed_sites", "2-%d,%d-%d" % (L // 2, L // 2 + 2, L - 1), "--min_gain", "0"])
    assert os.path.basename(fa) == "MFDCA_local_maxima_toy_protein.fa"
    got, E, rows = _read_maxima(fa, txt)
    assert got == res["sequences"] and E.tobytes() == res["energies"].tobytes() and len(rows) == 8
    assert [int(r[5]) - 1 for r in rows] == res["basin"].tolist()
