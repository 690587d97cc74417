"""Every element of every L-BFGS step of the plmDCA optimiser (pydca_amd/csrc/plm_engine.hip, vec_kernels.h) against a
high-precision direction, in float32 (the shipped path) and float64, at the smallest shapes where the vector walk changes
path: every residue of P modulo the pack, fewer packs than one wave, and more than kVecBlocks x kVecThreads packs (the second
trip of the grid-stride loop).  The run is driven one iteration at a time through the public API and read back after each;
the reference (tests/lbfgs_step_reference.py, pinned on the CPU by tests/test_lbfgs_step_host.py) rebuilds the history from
the returned iterates and never reads the device's.  A failure names the iteration, the element and the loop of the walk
that handles it.  Every check prints its figures (pytest -s).

Run on an MI355X:  python -m pytest tests/test_lbfgs_step.py -q -m gpu"""
import functools

import numpy as np
import pytest

import lbfgs_step_reference as R

pytestmark = pytest.mark.gpu

K = R.K_STEPS


@pytest.fixture(scope="module")
def L_():
    from pydca_amd import _lib
    _lib.lib()
    return _lib


def drive(ctx, dtype, n=K):
    """begin (for K iterations), then n single iterations: iterates, gradients, steps, norms and the stats after each."""
    ctx.plm_lbfgs_begin(K)
    st = ctx.plm_lbfgs_iterate(0)                                   # the norms of the starting point
    xs, gs = [ctx.plm_get_x(dtype)], [ctx.plm_get_g(dtype)]
    steps, xn, gn, stats = [], [st.xnorm], [st.gnorm], []
    for k in range(1, n + 1):
        assert not st.finished, "stopped with status %d after %d iterations, before iteration %d" % (st.status, st.iterations, k)
        st = ctx.plm_lbfgs_iterate(1)
        assert st.iterations == k, "iteration %d did not complete: status %d, %d iterations" % (k, st.status, st.iterations)
        xs.append(ctx.plm_get_x(dtype))
        gs.append(ctx.plm_get_g(dtype))
        steps.append(st.step)
        xn.append(st.xnorm)
        gn.append(st.gnorm)
        stats.append((st.status, st.iterations, st.finished))
    return dict(xs=xs, gs=gs, steps=steps, xnorms=xn, gnorms=gn, stats=stats)


@functools.lru_cache(maxsize=None)
def audited(L_, name, bits):
    """One run of the case on the device and its audit; the reference of a case is built once per module."""
    case = R.BY_NAME[name]
    dtype = np.float32 if bits == 32 else np.float64
    prec = L_.DCA_F32 if bits == 32 else L_.DCA_F64
    ctx = L_.Context(0, prec)
    ctx.set_msa(R.alignment(case), case.q)
    ctx.compute_weights(0.8, prec)
    ctx.plm_configure(case.lam, case.lam)
    ctx.plm_init_x()
    try:
        run = drive(ctx, dtype)
    finally:
        ctx.close()
    a = R.audit(run["xs"], run["gs"], run["steps"], dtype, run["xnorms"], run["gnorms"])
    print("\n[lbfgs-step] %-8s %s" % (name, a.summary()))
    return run, a


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("case", R.CASES, ids=repr)
def test_every_element_of_every_step(L_, case, bits):
    """x_{k+1} = x_k + t d_ref within 1/2 ulp(x_{k+1}) + 2 u |t d_ref| + rho |t| max|d_ref| for every element of the eight
    steps (history slots 0 .. 4, the wrap to slot 0, five stored pairs), and the reported norms within P 2^-53."""
    vec = R.vec_width(np.float32 if bits == 32 else np.float64)
    assert case.P % 4 == R.P_MOD4[case.name]                                   # the planted edge
    if case.name in R.SECOND_TRIP:
        assert case.P > R.VEC_BLOCKS * R.VEC_THREADS * vec                      # kVecBlocks x kVecThreads packs do not cover it
    else:
        assert case.P < R.VEC_BLOCKS * R.VEC_THREADS * vec
    if case.name == "q5_L2":
        assert case.P // vec < 64                                              # fewer packs than one wave
    run, a = audited(L_, case.name, bits)
    for s in a.steps:
        print("[lbfgs-step]   %r" % s)
    assert [s.bound_pairs for s in a.steps] == [0, 1, 2, 3, 4, 5, 5, 5]
    assert all(not fin for _, _, fin in run["stats"][:K - 1]), run["stats"]     # no iteration before the eighth finished the run
    assert a.ok, "%s float%d: %s" % (case.name, bits, a.failures())


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["q5_L6", "q21_L2"])
def test_restart_on_the_same_context(L_, name, bits):
    """A second plm_lbfgs_begin after three iterations of a first run starts from empty history slots: from the same x_0 it
    audits clean from k = 0 and reproduces the first run's iterates bit for bit."""
    case = R.BY_NAME[name]
    dtype = np.float32 if bits == 32 else np.float64
    prec = L_.DCA_F32 if bits == 32 else L_.DCA_F64
    first, _ = audited(L_, name, bits)
    ctx = L_.Context(0, prec)
    ctx.set_msa(R.alignment(case), case.q)
    ctx.compute_weights(0.8, prec)
    ctx.plm_configure(case.lam, case.lam)
    ctx.plm_init_x()
    try:
        three = drive(ctx, dtype, 3)
        ctx.plm_set_x(first["xs"][0])
        again = drive(ctx, dtype)
    finally:
        ctx.close()
    a = R.audit(again["xs"], again["gs"], again["steps"], dtype, again["xnorms"], again["gnorms"])
    print("\n[lbfgs-step] %-8s restart: %s" % (name, a.summary()))
    assert all(np.array_equal(u, v) for u, v in zip(three["xs"], first["xs"]))
    assert np.array_equal(again["xs"][1], first["xs"][1])
    assert all(np.array_equal(u, v) for u, v in zip(again["xs"] + again["gs"], first["xs"] + first["gs"]))
    assert again["steps"] == first["steps"]
    assert a.ok, a.failures()
