"""TEST INFRASTRUCTURE ONLY -- host reference for ONE L-BFGS step of the plmDCA optimiser (pydca_amd/csrc/plm_engine.hip,
vec_kernels.h), with no GPU dependency: tests/test_lbfgs_step.py and tests/native_comm_threads.py feed it what the device
returned, tests/test_lbfgs_step_host.py pins it on the CPU.

audit() takes the iterates x_0 .. x_K, the gradients g_0 .. g_K and the accepted steps t_1 .. t_K of a run and checks every
element of every step x_k -> x_{k+1} against x_k + t d_ref, where d_ref is the libLBFGS two-loop direction (m = 5, initial
scaling y.s / y.y of the newest pair) in np.longdouble with every dot product a math.fsum of its products.  The history is
rebuilt from the iterates alone, s_j = x_{j+1} - x_j and y_j = g_{j+1} - g_j as one subtraction in the engine's dtype -- the
device forms them the same way (vec_diff_gram_kernel), so nothing of the device's history is read.

Element bound, from the device's rounding sequence d = (T) v, p = (T)(t d), x' = (T)(x + p):

    bound[i] = 1/2 ulp_T(x_{k+1}[i]) + 2 u_T |t d_ref[i]| + rho |t| max|d_ref|

The first two terms are those three roundings and carry no margin.  rho covers the conditioning of the 11-coefficient
recursion, which has no closed form: it is MEASURED on the reference alone, as 8 x the largest relative difference (over the
iterations of the case) between d_ref and the same recursion in plain float64 with np.dot -- 8 because the device sums the
same terms in another order -- floored at 4 u_T in float32, where the coefficient error is far below the vector's own
rounding.  It never depends on what the device returned beyond the iterates that define the problem.

Scalars: the run's xnorm / gnorm against sqrt(fsum(x^2)), sqrt(fsum(g^2)) within P 2^-53 relative, the worst case of a double
sum of P exact products; one dropped tail element moves a norm by about 1 / P, so this is the check that sees the dot-product
kernels."""
import math

import numpy as np

LD = np.longdouble
M = 5                                    # history length of the optimiser
VEC_BLOCKS, VEC_THREADS = 1024, 256      # kVecBlocks, kVecThreads of vec_kernels.h


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def vec_width(dtype):
    """Elements per 16-byte pack."""
    return 16 // np.dtype(dtype).itemsize


def num_params(L, q):
    return L * q + (L * (L - 1) // 2) * q * q


def strip_starts(L, q, world):
    """First element of every rank's vectors under the column-strip decomposition: rank r > 0 starts at L q + (pairs whose
    first site lies before its first site) q^2, rank 0 at 0."""
    def pairs_before(s):
        return L * (L - 1) // 2 - (L - s) * (L - s - 1) // 2
    return [0] + [L * q + pairs_before(L * r // world) * q * q for r in range(1, world)]


def region(i, P, dtype, starts=(0,)):
    """Which loop of the vector walk (DCA_VEC_LOOP) handles element i of a P-vector whose ranks start at `starts` (16-byte
    aligned allocations): 'head' (elements in front of the first 16-byte boundary), 'packs' (with the trip of the
    grid-stride loop) or 'tail'."""
    vec = vec_width(dtype)
    starts = list(starts)
    r = max(j for j, s in enumerate(starts) if s <= i)
    lo, hi = starts[r], (starts[r + 1] if r + 1 < len(starts) else P)
    n, li = hi - lo, i - lo
    head = min((-lo) % vec, n)
    nv = (n - head) // vec
    where = "head" if li < head else "tail" if li >= head + nv * vec else "packs, trip %d" % (1 + (li - head) // vec // (VEC_BLOCKS * VEC_THREADS))
    return where if len(starts) == 1 else "rank %d %s" % (r, where)


# ----------------------------------------------------------------------------- dot products
def fsum_dot(a, b):
    """sum a[i] b[i] as math.fsum of the products: float32 x float32 products are exact in double; anything else is
    multiplied in longdouble, the doubles the products round to go through fsum and their remainders (2^-53 of the
    products, so their own summation error is below 2^-110 of the sum) are added up in longdouble."""
    if a.dtype == np.float32 and b.dtype == np.float32:
        return LD(math.fsum((a.astype(np.float64) * b.astype(np.float64)).tolist()))
    p = a.astype(LD) * b.astype(LD)
    hi = p.astype(np.float64)
    return LD(math.fsum(hi.tolist())) + np.sum(p - hi)


def plain_dot(a, b):
    return np.dot(a.astype(np.float64), b.astype(np.float64))


def two_loop(g, S, Y, dot=fsum_dot, wide=LD, ys=None):
    """libLBFGS's two-loop recursion (lbfgs.c, m = len(S) stored pairs, oldest first): -H g with H_0 = (y.s / y.y) I of the
    newest pair.  `wide` is the type of the working vector, `dot` the dot product; ys: known y_j.s_j (or None)."""
    n = len(S)
    d = -g.astype(wide)
    if n == 0:
        return d
    ys = [dot(Y[j], S[j]) if ys is None or ys[j] is None else ys[j] for j in range(n)]
    alpha = [None] * n
    for j in reversed(range(n)):
        alpha[j] = dot(S[j], d) / ys[j]
        d = d - alpha[j] * Y[j].astype(wide)
    d = d * (ys[-1] / dot(Y[-1], Y[-1]))
    for j in range(n):
        beta = dot(Y[j], d) / ys[j]
        d = d + (alpha[j] - beta) * S[j].astype(wide)
    return d


def history(xs, gs, k):
    """The pairs the step from x_k uses, oldest first: (indices j, s_j, y_j), each one subtraction in the vectors' dtype."""
    js = list(range(max(0, k - M), k))
    return js, [xs[j + 1] - xs[j] for j in js], [gs[j + 1] - gs[j] for j in js]


def reference_direction(xs, gs, k, order=None, wide=LD, dot=fsum_dot):
    """d_ref of the step from x_k.  order: a permutation of the stored pairs (the negative controls use it)."""
    _, S, Y = history(xs, gs, k)
    if order is not None:
        S, Y = [S[i] for i in order], [Y[i] for i in order]
    return two_loop(gs[k], S, Y, dot=dot, wide=wide)


def apply_step(x, t, d, dtype):
    """The device's sequence: d = (T) v, p = (T)(t d), x' = (T)(x + p)."""
    dtype = np.dtype(dtype).type
    dT = np.asarray(d).astype(dtype)
    return (x + (dtype(t) * dT).astype(dtype)).astype(dtype)


def exact_norm(v):
    return float(np.sqrt(fsum_dot(v, v)))


# ----------------------------------------------------------------------------- the audit
class StepReport:
    """One step x_k -> x_{k+1}: the worst element, its ratio to the bound and the loop that handles it."""

    def __init__(self, k, bound_pairs, step, ratio, index, where, err, bound, rel_plain):
        self.k, self.bound_pairs, self.step, self.ratio, self.index, self.where = k, bound_pairs, step, ratio, index, where
        self.err, self.bound, self.rel_plain = err, bound, rel_plain

    def __repr__(self):
        return "step %d (%d pairs, t = %.6g): element %d [%s] off by %.3e, bound %.3e, ratio %.3f" % (
            self.k, self.bound_pairs, self.step, self.index, self.where, self.err, self.bound, self.ratio)


class Audit:
    def __init__(self, dtype, P, steps, rho_measured, rho, norm_bound, xnorm_dev, gnorm_dev):
        self.dtype, self.P, self.steps = np.dtype(dtype), P, steps
        self.rho_measured, self.rho = rho_measured, rho            # largest relative difference to the plain recursion; 8 x it, floored
        self.norm_bound, self.xnorm_dev, self.gnorm_dev = norm_bound, xnorm_dev, gnorm_dev     # relative deviations, None where not given

    @property
    def ratios(self):
        return [s.ratio for s in self.steps]

    @property
    def worst(self):
        return max(self.steps, key=lambda s: s.ratio)

    @property
    def norm_dev(self):
        devs = [d for d in self.xnorm_dev + self.gnorm_dev if d is not None]
        return max(devs) if devs else 0.0

    def failures(self):
        out = [repr(s) for s in self.steps if not s.ratio <= 1.0]
        for name, devs in (("xnorm", self.xnorm_dev), ("gnorm", self.gnorm_dev)):
            out += ["%s of iterate %d off by %.3e relative, bound %.3e" % (name, k, d, self.norm_bound)
                    for k, d in enumerate(devs) if d is not None and not d <= self.norm_bound]
        return out

    @property
    def ok(self):
        return not self.failures()

    def first_failing_step(self):
        bad = [s.k for s in self.steps if not s.ratio <= 1.0]
        return bad[0] if bad else None

    def summary(self):
        w = self.worst
        return "%s P=%d: worst ratio %.3f at step %d, element %d [%s]; rho measured %.3e -> %.3e; norms off by %.3e of %.3e" % (
            self.dtype.name, self.P, w.ratio, w.k, w.index, w.where, self.rho_measured, self.rho, self.norm_dev, self.norm_bound)

    def as_dict(self):
        w = self.worst
        return dict(ratios=[float(r) for r in self.ratios], worst_ratio=float(w.ratio), worst_step=w.k, worst_index=w.index, worst_where=w.where,
                    rho_measured=self.rho_measured, rho=self.rho, norm_dev=self.norm_dev, norm_bound=self.norm_bound, failures=self.failures())


def audit(xs, gs, steps, dtype, xnorms=None, gnorms=None, starts=(0,)):
    """xs, gs: K + 1 vectors of `dtype` (x_0 .. x_K and their gradients), steps: the K accepted step lengths.  xnorms, gnorms:
    optional K + 1 norms as the run reported them (None where it reported none).  starts: first element of every rank's
    share of the vectors (names the loop of the walk a bad element belongs to).  -> Audit."""
    dtype = np.dtype(dtype)
    K, P = len(steps), len(xs[0])
    assert len(xs) == K + 1 and len(gs) == K + 1
    assert all(v.dtype == dtype and v.shape == (P,) for v in list(xs) + list(gs)), "iterates and gradients in the engine's own dtype"
    u = unit_roundoff(dtype)
    ys = {}                                   # y_j . s_j, kept from step to step like the optimiser's own
    kept, rel_plain = [], []
    for k in range(K):
        js, S, Y = history(xs, gs, k)
        d_ref = two_loop(gs[k], S, Y, ys=[ys.get(j) for j in js])
        if js:
            ys.setdefault(js[-1], fsum_dot(Y[-1], S[-1]))
            d_plain = two_loop(gs[k], S, Y, dot=plain_dot, wide=np.float64)
            rel_plain.append(float(np.max(np.abs(d_ref - d_plain)) / np.max(np.abs(d_ref))))
        else:
            rel_plain.append(0.0)
        t = LD(dtype.type(steps[k]))
        td = np.abs(t * d_ref)
        err = np.abs(xs[k + 1].astype(LD) - (xs[k].astype(LD) + t * d_ref)).astype(np.float64)
        base = (0.5 * np.spacing(np.abs(xs[k + 1])).astype(LD) + 2 * u * td).astype(np.float64)
        kept.append((err, base, float(np.max(td))))
    rho_measured = max(rel_plain) if rel_plain else 0.0
    rho = 8.0 * rho_measured
    if dtype == np.float32:
        rho = max(rho, 4 * u)
    reports = []
    for k, (err, base, tdmax) in enumerate(kept):
        bound = base + rho * tdmax
        ratio = err / bound
        i = int(np.argmax(ratio))
        reports.append(StepReport(k, min(k, M), float(steps[k]), float(ratio[i]), i, region(i, P, dtype, starts), float(err[i]), float(bound[i]), rel_plain[k]))

    def devs(norms, vs):
        if norms is None:
            return [None] * (K + 1)
        out = []
        for nv, v in zip(norms, vs):
            ref = exact_norm(v) if nv is not None else None
            out.append(None if nv is None else abs(float(nv) - ref) / ref)
        return out
    return Audit(dtype, P, reports, rho_measured, rho, P * 2.0 ** -53, devs(xnorms, xs), devs(gnorms, gs))


# ----------------------------------------------------------------------------- the cases of the GPU test
class Case:
    """A random alignment of N draws (duplicates removed) at a shape where the vector walk changes path."""

    def __init__(self, q, L, N, lam, why):
        self.q, self.L, self.N, self.lam, self.why = q, L, N, lam, why
        self.P = num_params(L, q)
        self.name = "q%d_L%d" % (q, L)

    def __repr__(self):
        return self.name


K_STEPS = 8           # history slots 0 .. 4, the wrap back to slot 0 and bound = 5
CASES = [
    Case(5, 2, 40, 0.05, "P % 4 = 3, fewer packs than one wave"),
    Case(5, 3, 40, 0.01, "P % 4 = 2"),
    Case(5, 6, 48, 0.01, "P % 4 = 1, odd: float64 tail of 1"),
    Case(5, 7, 48, 0.01, "P % 4 = 0, no tail"),
    Case(21, 2, 60, 0.001, "P % 4 = 3, odd"),
    Case(21, 72, 64, 0.01, "second trip of the stride loop, P % 4 = 0"),
    Case(21, 73, 64, 0.01, "second trip of the stride loop, P % 4 = 1"),
]
BY_NAME = {c.name: c for c in CASES}
P_MOD4 = {"q5_L2": 3, "q5_L3": 2, "q5_L6": 1, "q5_L7": 0, "q21_L2": 3, "q21_L72": 0, "q21_L73": 1}
SECOND_TRIP = ("q21_L72", "q21_L73")


def alignment(case):
    """uint8 [N', L], states 0 .. q-1: N uniform draws, first occurrences kept."""
    rng = np.random.default_rng(1000 * case.q + case.L)
    X = rng.integers(0, case.q, size=(case.N, case.L), dtype=np.uint8)
    _, first = np.unique(X, axis=0, return_index=True)
    return np.ascontiguousarray(X[np.sort(first)])
