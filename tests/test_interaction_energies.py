"""Inter-protein energies on the GPU (dca_plm_interaction_energies, dca_mf_interaction_energies) against
the float64 restatement of tests/interaction_reference.py, bit for bit (tobytes() equality): the rule has only adds, divisions
by q and reads, so nothing rests on libm.  The shapes are interaction_reference.energy_cases: the four splits, one LB just past
the plan's single-tile limit and one LA just past a staging chunk (both read from the plan driver), group sizes 0, 1, 63, 64,
65 and 257 on either side in one call of many groups."""
import numpy as np
import pytest

from pydca_amd import _lib, parallel
import interaction_drivers as D
import interaction_reference as R
from test_conditional_sampling import mf_random_context
from test_potts_sampling import mf_context, plm_context

pytestmark = pytest.mark.gpu

MODELS = [("mf", 2, 64), ("mf", 5, 64), ("mf", 21, 64), ("mf", 32, 64), ("plm", 5, 32), ("plm", 5, 64), ("plm", 21, 32), ("plm", 21, 64)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return D.compile_plan_driver(tmp_path_factory.mktemp("interactionplan"))


def model_context(kind, q, prec, L, seed):
    """-> (ctx, h, Jp, energies entry, interaction entry)"""
    if kind == "mf":
        ctx, h, Jp = mf_random_context(L, q, seed)
        return ctx, h, Jp, ctx.mf_energies, ctx.mf_interaction_energies
    ctx, h, Jp = plm_context(L, q, _lib.DCA_F64 if prec == 64 else _lib.DCA_F32, seed, sigma=0.7, N=16)
    return ctx, h, Jp, ctx.plm_energies, ctx.plm_interaction_energies


def rows_for(groups, LA, LB, q, seed):
    rng = np.random.default_rng([seed, LA, LB, q])
    nA, nB = sum(a for a, _ in groups), sum(b for _, b in groups)
    return rng.integers(0, q, size=(nA, LA), dtype=np.uint8), rng.integers(0, q, size=(nB, LB), dtype=np.uint8)


def assert_blocks_equal(got, want):
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == np.float64, (g, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (g, a.shape, int((a != b).sum()), float(np.abs(a - b).max()) if a.size else 0.0)


# ---------------------------------------------------------------- 1. bits at every shape, both gauges
@pytest.mark.parametrize("kind,q,prec", MODELS)
def test_bits_match_restatement(kind, q, prec, plan):
    for k, (LA, LB, groups) in enumerate(R.energy_cases(plan, q)):
        L = LA + LB
        ctx, _h, Jp, _en, call = model_context(kind, q, prec, L, 100 * q + prec + k)
        XA, XB = rows_for(groups, LA, LB, q, k)
        oa, ob = R.offsets_of(groups)
        for gauge, name in ((0, "as_stored"), (1, "zero_sum")):
            want = R.interaction_energies(Jp, L, LA, XA, XB, gauge, oa, ob)
            assert_blocks_equal(call(XA, XB, LA, oa, ob, gauge=name), want)
        ctx.close()


# ---------------------------------------------------------------- 2. grouping, batch, call and block invariance
@pytest.mark.parametrize("kind,q,prec", [("mf", 21, 64), ("plm", 5, 32)])
def test_grouping_call_and_block_invariance(kind, q, prec, plan, monkeypatch):
    LA, LB = 6, 7
    L = LA + LB
    groups = R.MAIN_GROUPS
    ctx, _h, Jp, _en, call = model_context(kind, q, prec, L, 7 * q)
    XA, XB = rows_for(groups, LA, LB, q, 3)
    oa, ob = R.offsets_of(groups)
    whole = call(XA, XB, LA, oa, ob)
    dense = call(XA, XB, LA)                                   # G = 1: all against all
    assert dense.shape == (XA.shape[0], XB.shape[0])
    assert dense.tobytes() == R.interaction_energies(Jp, L, LA, XA, XB, 1).tobytes()
    for g, blk in enumerate(whole):                            # ... holds every group's block
        assert blk.tobytes() == np.ascontiguousarray(dense[oa[g]:oa[g + 1], ob[g]:ob[g + 1]]).tobytes()
    cut = 30                                                   # one call against two calls
    first = call(XA[:oa[cut]], XB[:ob[cut]], LA, oa[:cut + 1], ob[:cut + 1])
    second = call(XA[oa[cut]:], XB[ob[cut]:], LA, oa[cut:] - oa[cut], ob[cut:] - ob[cut])
    assert_blocks_equal(first + second, whole)
    for cap in (1, 37, 300):                                   # several blocks of A-rows, groups cut across blocks
        monkeypatch.setenv("DCA_CROSS_PASS", str(cap))
        assert len(plan(q, LB, R.row_counts(groups), cross_pass=cap)["blocks"]) > 1
        assert_blocks_equal(call(XA, XB, LA, oa, ob), whole)
    monkeypatch.delenv("DCA_CROSS_PASS")
    ctx.close()


# ---------------------------------------------------------------- 3. a golden model; the four-energy identity
def test_mf_golden_model_and_identity():
    ctx, h, Jp, X = mf_context("mf_toy_protein")
    L, q = h.shape
    LA = L // 2
    XA, XB = np.ascontiguousarray(X[:70, :LA]), np.ascontiguousarray(X[5:90, LA:])
    for gauge, name in ((0, "as_stored"), (1, "zero_sum")):
        assert ctx.mf_interaction_energies(XA, XB, LA, gauge=name).tobytes() == R.interaction_energies(Jp, L, LA, XA, XB, gauge).tobytes()
    check_identity(ctx.mf_energies, ctx.mf_interaction_energies, h, Jp, XA[:12], XB[:12], LA)
    ctx.close()


def check_identity(energies, call, h, Jp, XA, XB, LA):
    """E(a,b) - E(a,b') - E(a',b) + E(a',b') (gauge 0) = the same combination of full energies of the concatenated rows, within
    the addend-count bounds: a full energy sums T = L + L(L-1)/2 terms (T 2^-53 sum |terms| each), a cross energy LA LB"""
    L = h.shape[0]
    X = call(XA, XB, LA, gauge="as_stored")
    Jt = R.cross_couplings(Jp, L, LA, 0)
    xb = R.sum_bound(Jt, XA, XB)
    nA, nB = XA.shape[0], XB.shape[0]
    cat = np.concatenate([np.repeat(XA, nB, axis=0), np.tile(XB, (nA, 1))], axis=1)
    F = energies(cat).reshape(nA, nB)
    _, sabs = R.full_energies(h, Jp, cat)
    fb = (L + L * (L - 1) // 2) * 2.0 ** -53 * sabs.astype(np.float64).reshape(nA, nB)

    def comb(M):
        return M[:-1, :-1] - M[:-1, 1:] - M[1:, :-1] + M[1:, 1:]
    bound = (xb[:-1, :-1] + xb[:-1, 1:] + xb[1:, :-1] + xb[1:, 1:]) + (fb[:-1, :-1] + fb[:-1, 1:] + fb[1:, :-1] + fb[1:, 1:])
    diff = np.abs(comb(X) - comb(F))
    print("four-energy identity: largest difference %.3g, bound there %.3g" % (diff.max(), bound.ravel()[diff.argmax()]))
    assert np.all(diff <= bound + 4 * 2.0 ** -52 * (np.abs(comb(X)) + np.abs(comb(F))))


@pytest.mark.parametrize("prec", [32, 64])
def test_plm_identity(prec):
    L, q, LA = 13, 21, 6
    ctx, h, Jp, energies, call = model_context("plm", q, prec, L, 5)
    XA, XB = rows_for([(12, 12)], LA, L - LA, q, 2)
    check_identity(energies, call, h, Jp, XA, XB, LA)
    ctx.close()


# ---------------------------------------------------------------- 4. state untouched
def test_training_state_and_bm_run_untouched():
    from conftest import golden
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    LA = 4

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
    ctx.plm_interaction_energies(X[:100, :LA], X[:80, LA:], LA)
    ctx.plm_interaction_energies(X[:10, :LA], X[:10, LA:], LA, [0, 4, 10], [0, 5, 10], gauge="as_stored")
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
    mctx.mf_interaction_energies(MX[:50, :3], MX[:50, 3:], 3)
    assert mctx.mf_couplings().tobytes() == J0.tobytes()
    mctx.close()


# ---------------------------------------------------------------- 5. errors
def _code(call):
    with pytest.raises(_lib.DcaBackendError) as ei:
        call()
    return ei.value.code


def _raw(ctx, fn, split=4, nA=3, nB=2, oa=(0, 1, 3), ob=(0, 2, 2), G=2, gauge=1, XA=True, XB=True, out=True, codeA=None, codeB=None):
    L = ctx.L
    A = np.zeros((max(nA, 1), max(split, 1)), dtype=np.uint8)
    B = np.zeros((max(nB, 1), max(L - split, 1)), dtype=np.uint8)
    if codeA is not None:
        A[-1, -1] = codeA
    if codeB is not None:
        B[0, 0] = codeB
    a = None if oa is None else np.asarray(oa, dtype=np.int32)
    b = None if ob is None else np.asarray(ob, dtype=np.int32)
    o = np.zeros(64, dtype=np.float64)
    return fn(ctx._h, split, A.ctypes.data if XA else None, nA, B.ctypes.data if XB else None, nB, None if a is None else a.ctypes.data,
              None if b is None else b.ctypes.data, G, gauge, o.ctypes.data if out else None)


def test_argument_and_state_errors():
    from conftest import golden
    G = golden("plm_toy_rna")
    X, q = G["X"], int(G["q"])
    L = X.shape[1]
    lib = _lib.lib()
    ctx = _lib.Context(0, _lib.DCA_F32)
    ctx.set_msa(X, q)
    ctx.compute_weights(0.8, _lib.DCA_F32)
    assert _code(lambda: ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4)) == _lib.DCA_ERR_STATE      # before dca_plm_configure
    assert _code(lambda: ctx.mf_interaction_energies(X[:4, :4], X[:4, 4:], 4)) == _lib.DCA_ERR_STATE       # before the mf couplings
    ctx.plm_configure(1.8, 1.8)
    ctx.plm_init_x()
    for fn in (lib.dca_plm_interaction_energies,):
        assert _raw(ctx, fn) == _lib.DCA_OK
        for kw in (dict(split=0), dict(split=L), dict(split=-1), dict(nA=-1, oa=(0, 0, -1)), dict(nB=-1, ob=(0, 0, -1)), dict(G=0),
                   dict(G=-1), dict(oa=None), dict(ob=None), dict(oa=(1, 1, 3)), dict(ob=(0, 2, 1)), dict(oa=(0, 2, 1), nA=1),
                   dict(oa=(0, 1, 2)), dict(ob=(0, 3, 2)), dict(gauge=2), dict(gauge=-1), dict(XA=False), dict(XB=False), dict(out=False),
                   dict(codeA=q), dict(codeB=q)):
            assert _raw(ctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
        # no energies to form: DCA_OK whatever the arrays
        assert _raw(ctx, fn, nA=0, nB=0, oa=(0, 0, 0), ob=(0, 0, 0), XA=False, XB=False, out=False) == _lib.DCA_OK
        assert _raw(ctx, fn, nA=3, nB=2, oa=(0, 3, 3), ob=(0, 0, 2), XA=False, XB=False, out=False) == _lib.DCA_OK
    assert ctx.plm_interaction_energies(np.zeros((0, 4), dtype=np.uint8), X[:3, 4:], 4).shape == (0, 3)
    assert [b.shape for b in ctx.plm_interaction_energies(X[:3, :4], X[:2, 4:], 4, [0, 3, 3], [0, 0, 2])] == [(3, 0), (0, 2)]
    with pytest.raises(ValueError):
        ctx.plm_interaction_energies(X[:3, :4], X[:2, 4:], 4, gauge="other")
    ctx.plm_lbfgs_begin(50)
    ctx.plm_lbfgs_iterate(1)
    assert ctx.plm_interaction_energies(X[:4, :4], X[:5, 4:], 4).shape == (4, 5)                          # allowed during an L-BFGS run
    ctx.plm_lbfgs_end()
    ctx.plm_set_reduce_hook(lambda *a: 0)
    assert _code(lambda: ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4)) == _lib.DCA_ERR_STATE      # one GPU only
    ctx.plm_set_reduce_hook(None)
    ctx.plm_set_vector_sharding(0, 2, lambda *a: 0)
    assert _code(lambda: ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4)) == _lib.DCA_ERR_STATE
    ctx.plm_set_vector_sharding(0, 1, None)
    assert ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4).shape == (4, 4)
    parallel.init_native_comm(ctx, _lib, 0, 1)                                                             # the native-comm modes
    for mode in (1, 2, 3):
        ctx.plm_set_native_comm(mode)
        assert _code(lambda: ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4)) == _lib.DCA_ERR_STATE, mode
    ctx.plm_set_native_comm(0)
    assert ctx.plm_interaction_energies(X[:4, :4], X[:4, 4:], 4).shape == (4, 4)
    ctx.close()
    mctx, _h, _Jp, MX = mf_context("mf_toy_rna")
    fn = lib.dca_mf_interaction_energies
    assert _raw(mctx, fn) == _lib.DCA_OK
    for kw in (dict(split=0), dict(split=mctx.L), dict(G=0), dict(gauge=3), dict(oa=(0, 2, 1), nA=1), dict(codeA=5), dict(codeB=5),
               dict(out=False)):
        assert _raw(mctx, fn, **kw) == _lib.DCA_ERR_ARG, kw
    mctx.close()


def test_state_error_under_column_strips():
    """the column-strip decomposition exists from two ranks on: tests/interaction_strips_child.py runs them as threads"""
    import json
    import os
    import subprocess
    import sys
    child = os.path.join(D.ROOT, "tests", "interaction_strips_child.py")
    res = json.loads(subprocess.check_output([sys.executable, child], timeout=120).decode().strip().splitlines()[-1])
    assert len(res) == 2
    for r in res:
        assert r["code"] == _lib.DCA_ERR_STATE and "column strips" in r["message"], r
