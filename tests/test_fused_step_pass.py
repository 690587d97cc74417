"""The fused step pass of the plmDCA optimiser (lbfgs_dir_trial_expand_kernel, pydca_amd/csrc/lbfgs_kernels.h: direction, first
trial point and coupling table in one kernel) against the three kernels it replaces (DCA_PLM_FUSE_STEP=0), bit for bit.  No sum
moves and every element is computed by the same expression, so there is no tolerance: x, g and the optimiser's statistics after
each single iteration are compared with np.array_equal.  The shapes are the smallest at which the tiling changes path: one full
tile of sites plus a one-site tail, several tiles (the transposed runs cross a strip of W), the site-pair alphabet of q = 5 with
an odd L, and a q = 5 tile of 25 sites plus a tail.

Run on an MI355X:  python -m pytest tests/test_fused_step_pass.py -q -m gpu"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gen_msa  # noqa: E402

pytestmark = pytest.mark.gpu

KNOB = "DCA_PLM_FUSE_STEP"
ITERS = 6
# name -> (q, L, N, seed, lambda_h, lambda_J)
SHAPES = {
    "q21_L7": (21, 7, 70, 7001, 0.01, 0.01),        # one full 6-site tile + a 1-site tail (float64: 3-site tiles)
    "q21_L13": (21, 13, 130, 7002, 0.01, 0.01),     # two tiles + a tail
    "q5_L9": (5, 9, 200, 7003, 0.01, 0.01),         # site-pair alphabet, odd L
    "q5_L27": (5, 27, 200, 7004, 0.01, 0.01),       # a 25-site tile + a 2-site tail, two ranges of j
}
# the line search of this case needs a second evaluation in some iteration (tests/test_fused_step_pass_host.py holds the CPU
# oracle to that): the trials after the first run the three kernels
MULTI_EVAL = ("q21_L7_ls", (21, 7, 70, 7005, 5.0, 5.0))


def alignment(shape):
    q, L, N, seed = shape[:4]
    return gen_msa.generate(L, N, q, seed)


class knob:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get(KNOB)
        os.environ[KNOB] = str(self.value)

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = self.saved


def expands(run_):
    """launches of plm_expand_kernel up to each call (`same` leaves the keys with an underscore alone)"""
    return [r["_expands"] for r in run_]


def stats_tuple(st):
    return (st.status, st.iterations, st.evaluations, st.finished, st.fx, st.xnorm, st.gnorm, st.step)


def run(shape, bits, fused, schedule=(1,) * ITERS, probe=False):
    """The optimisation driven through `schedule` (iterations per call): x, g and the statistics after every call; with
    `probe` the API calls that read or rewrite engine state between the calls, and their outputs."""
    from pydca_amd import _lib
    q, lh, lJ = shape[0], shape[4], shape[5]
    dtype = np.float32 if bits == 32 else np.float64
    prec = _lib.DCA_F32 if bits == 32 else _lib.DCA_F64
    with knob(1 if fused else 0):           # read by plm_configure
        ctx = _lib.Context(0, prec)
        try:
            ctx.set_msa(alignment(shape), q)
            ctx.compute_weights(0.8, prec)
            ctx.plm_configure(lh, lJ)
            ctx.plm_init_x()
            ctx.set_profiling(True)         # counts the launches of the expand stage; the event records change no result
            ctx.plm_lbfgs_begin(sum(schedule) + 1)
            out = []
            for k, n in enumerate(schedule):
                st = ctx.plm_lbfgs_iterate(n)
                rec = dict(x=ctx.plm_get_x(dtype), g=ctx.plm_get_g(dtype), stats=stats_tuple(st))
                rec["_expands"] = ctx.kernel_time("plm_expand")[1]
                if probe:
                    if k % 2 == 0:
                        rec["fx"] = ctx.plm_gradient()          # rewrites W and g at the accepted point
                        rec["g2"] = ctx.plm_get_g(dtype)
                    rec["scores"] = ctx.plm_scores(True)
                    rec["x2"] = ctx.plm_get_x(dtype)
                out.append(rec)
            return out
        finally:
            ctx.close()


@functools.lru_cache(maxsize=None)
def plain(name, bits):
    """The three-kernel run of a shape, one iteration per call: made once per module, never modified."""
    return run(SHAPES[name] if name in SHAPES else MULTI_EVAL[1], bits, fused=False)


def same(a, b, what):
    assert len(a) == len(b)
    for k, (u, v) in enumerate(zip(a, b)):
        assert sorted(u) == sorted(v)
        for key in u:
            if key.startswith("_"):
                continue
            if key == "stats":
                print("[fused-step] %s call %d: stats %r | %r" % (what, k, u[key], v[key]))
                assert u[key] == v[key], "%s: stats after call %d differ: %r != %r" % (what, k, u[key], v[key])
            else:
                ua, va = np.asarray(u[key]), np.asarray(v[key])
                ndiff = int(np.sum(ua != va)) if ua.shape == va.shape else -1
                print("[fused-step] %s call %d: %s differs in %d elements" % (what, k, key, ndiff))
                assert np.array_equal(ua, va), "%s: %s after call %d differs in %d elements (first %s)" % (
                    what, key, k, ndiff, np.flatnonzero(ua.ravel() != va.ravel())[:4] if ndiff > 0 else "-")


@pytest.mark.parametrize("name,bits", [("q21_L7", 32), ("q21_L13", 32), ("q5_L9", 32), ("q5_L27", 32), ("q21_L7", 64), ("q21_L13", 64)])
def test_bit_identical_to_the_three_kernels(name, bits):
    fused = run(SHAPES[name], bits, fused=True)
    assert fused[-1]["stats"][1] == ITERS, fused[-1]["stats"]           # all six iterations ran: five fused passes were used
    same(fused, plain(name, bits), "%s float%d" % (name, bits))
    # the fused pass did run: from the second iteration on the first trial of every line search launches no expand
    print("[fused-step] %s float%d: expand launches %r | %r" % (name, bits, expands(fused), expands(plain(name, bits))))
    assert [a - b for a, b in zip(expands(plain(name, bits)), expands(fused))] == list(range(ITERS))


def test_later_trials_of_a_search_run_the_three_kernels():
    name, shape = MULTI_EVAL
    fused = run(shape, 32, fused=True)
    st = fused[-1]["stats"]
    assert st[1] == ITERS and st[2] > st[1] + 1, "no line search with a second trial: %r" % (st,)
    assert any(r["stats"][7] != 1.0 for r in fused[1:]), "every search after the first accepted its first trial"
    same(fused, plain(name, 32), name)


def test_api_calls_between_iterations():
    """get_x, get_g, gradient() and scores between the iterations: their outputs and the trajectory that continues."""
    shape = SHAPES["q21_L13"]
    fused = run(shape, 32, fused=True, probe=True)
    ref = run(shape, 32, fused=False, probe=True)
    same(fused, ref, "probe")
    # ... and the probes do not move the trajectory
    same([dict(x=r["x"], g=r["g"]) for r in fused], [dict(x=r["x"], g=r["g"]) for r in plain("q21_L13", 32)], "probe against plain")


def test_three_iterations_in_one_call():
    shape = SHAPES["q21_L13"]
    once = run(shape, 32, fused=True, schedule=(3,))
    ones = run(shape, 32, fused=True, schedule=(1, 1, 1))
    same(once[-1:], ones[-1:], "3 against 1+1+1")
    once0 = run(shape, 32, fused=False, schedule=(3,))
    same(once[-1:], once0[-1:], "3 fused against 3 plain")
