"""TEST INFRASTRUCTURE ONLY -- host reference for ONE arDCA evaluation (fx, g and the optimiser's |g|^2) of
pydca_amd/csrc/ardca.hip, with no GPU dependency: tests/test_ardca_eval_audit.py feeds it what the device returned,
tests/test_ardca_eval_audit_host.py pins it on the CPU.

reference(case, plan) evaluates the objective of include/dca_hip.h in np.longdouble with exact sums over the sequences:

    W_n = w_n / sum w;  u_nl(b) = h_l(b) + sum_{k<l} J_kl(s_nk, b);  c_nl(b) = (u - max u) - log sum_b exp(u - max u);
    R_nl(b) = W_n (exp c_nl(b) - [s_nl = b]);
    g[h_l(b)] = 2 lambda_h h_l(b) + sum_n R_nl(b);   g[J_kl(a, b)] = 2 lambda_J J_kl(a, b) + sum_{n: s_nk = a} R_nl(b);
    fx = - sum_n W_n sum_l c_nl(s_nl) + lambda_h sum h^2 + lambda_J sum J^2.

The sums over n are plm_eval_reference's exact limb sums (what they cut off, below 2^-131 per addend, enters the bound), fx is
its fsum_ld.  Per element e the reference also returns m_e, the number of addends (the sequences with s_nk = a; all N for a
field), and A[e] = sum |R| over them.

ELEMENT BOUND, from the device's rounding sequence as ardca.hip and site_conditionals.h write it (u = 2^-53,
gamma(k) = k u / (1 - k u), eta the smallest normal double).  Nothing the device returns enters it.

  * u^_l(b): h_l(b), then l addends in ascending k, one accumulator: |u^ - u| <= gamma(l) Uabs, Uabs = |h| + sum_k |J|.
  * m^ = max_b u^ is exact, and c is the same for any shift m, so the reference is read with the device's m^:
    d^ = fl(u^ - m^) is off by delta = gamma(l) Uabs + u |d|.
  * Z^ = sum_b exp^(d^_b), ascending b: every term carries delta_b + eps_exp relative, the sum gamma(q - 1):
    rho_Z = sum_b p_b delta_b + eps_exp + gamma(q - 1) (+ q eta for terms that underflow; Z >= 1).
    eps_exp = 4 x (the largest error in ulps of numpy's exp against the longdouble exp over the case's arguments, not below the
    1/2 ulp of a correctly rounded function) x 2 u: the device library is another implementation of the same function, both
    documented to about an ulp -- plm_eval_reference's treatment and its factor.  eps_log likewise.
  * lz^ = log^(Z^): |lz^ - lz| <= rho_Z / (1 - rho_Z) + eps_log |lz|.
  * the residual's argument fl(d^_b - lz^) is off by delta_b + (the error of lz^) + u |c_b|; exp^ of it adds eps_exp:
    p^_b = p_b (1 + theta_b'), |theta_b'| <= theta_b / (1 - theta_b), theta_b = delta_b + dlz + u |c_b| + eps_exp.
  * W^_n = fl(w_n / meff), meff the ascending sum of the weights: gamma(N) relative; fl(p^ - [s = b]) and the product by W^
    one rounding each:  |R^ - R| <= W p theta / (1 - theta) (1 + gamma(N + 2)) + gamma(N + 2) |R| + 2 eta =: E_R,
    the 2 eta for a p^ or a product that underflows (an argument below -745 gives 0 for a p of 10^-330).
  * the m_e addends of an element are added in ascending n from an accumulator of zero (m_e - 1 roundings, adding to zero is
    exact), a further pass adds its own sum to the stored one (one rounding per further pass), then fl(2 lambda x) (one
    rounding, 2 lambda is exact) and its add: no path from an addend to the result sees more than m_e + passes + 2 roundings.

    bound[e] = gamma(m_e + passes + 2) (A[e] + |2 lambda x_e|) + sum_{addends} E_R + m_e (2^-131 + 2 eta) + 2^-58 (A[e] + |2 lambda x_e|)

  the last term for the reference's own longdouble roundings.  One missing addend of typical size A / m stands out while
  m (m + passes + 2) u < 1: at N <= 200 always.

fx: the site value fl(fl(u^_s - m^) - lz^) is off by delta_s + dlz + u |c_s| =: eps_site.  Then log P(s_n) adds L values
(L - 1 roundings), W^_n carries gamma(N), the product one rounding, ar_wsum_kernel adds ceil(pass / 256) products per thread
and 8 tree levels, the host adds the passes (one rounding each) and the penalty: depth_F = (L - 1) + (N + 2) + ceil(pass / 256)
+ 8 + passes + 2.  The penalty dots are dot_depth() deep (below), times lambda and added: two more each.

    fx_bound = sum_n W_n sum_l eps_site + gamma(depth_F) sum W |c_s| + gamma(dot_depth + 4) penalty + 2^-58 (sum W |c_s| + penalty)

|g|^2 (ar_dot_kernel, ar_dot_final_kernel): a product (one rounding), thread i of 65 536 adds the elements i, i + 65 536, ...
in ascending order (ceil(n / 65 536) - 1 roundings from zero), a fixed tree over the 256 threads of a block (8 levels) and one
over the 256 block results (8 levels): dot_depth(n) = ceil(n / 65 536) + 16.  The optimiser reports sqrt(|g|^2) (correctly
rounded, and squared again by the test in longdouble): dot_bound = gamma(dot_depth + 2) sum g^2.

audit() checks ALL P elements (it asserts the count) and names what fails: the site (field) or the pair, the states, and the
workgroup and thread of ar_field_kernel / ar_grad_kernel that write the element."""
import os
import subprocess

import numpy as np

from plm_eval_reference import CUT_OFF, EXP_FACTOR, LD, exact_group_sums, fsum_ld, gamma, num_params, ulps_off

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAMBDA_H, LAMBDA_J = 0.01, 0.02
SCALE = 0.4                               # standard deviation of the model's parameters
U = 2.0 ** -53
ETA = float(np.finfo(np.float64).tiny)
FIELD_THREADS = 256                       # ar_field_kernel, ar_wsum_kernel
DOT_STRIDE = 256 * 256                    # ar_dot_kernel: kDotBlocks blocks of 256 threads
OWN = 2.0 ** -58                          # the reference's own roundings, relative to an element's sum of |addends|


def pair_index(L, k, l):
    return L * (L - 1) // 2 - (L - k) * (L - k - 1) // 2 + (l - k - 1)


# ----------------------------------------------------------------------------- the case table
class Case:
    """One row of the table: shape, pass size (0: one pass), the field entry that saturates a site, what the case reaches
    and the geometry facts (plan_of) that say so."""

    def __init__(self, q, L, N, reaches, facts, pass_size=0, saturate=None):
        self.q, self.L, self.N, self.reaches, self.facts, self.pass_size, self.saturate = q, L, N, reaches, facts, pass_size, saturate
        self.P = num_params(L, q)
        self.name = "q%d_L%d_N%d%s%s" % (q, L, N, "_pass%d" % pass_size if pass_size else "", "_saturated" if saturate else "")

    def __repr__(self):
        return self.name


# facts: KC, threads (ar_plan.h); chunks: the earlier sites of the last site by workgroup; own / idle: threads of a full chunk
# with / without a column; fieldBlocks: workgroups of ar_field_kernel; dotRows: terms per thread of the dot over all P
# parameters; tiles: the sequences of each pass by staged tile
CASES = [
    Case(21, 35, 130, "chunks 16 + 16 + 2; 336 of 384 threads own a column; P = 263 130 > 65 536: the dot kernels' stride loop",
         dict(KC=16, chunks=[16, 16, 2], threads=384, own=336, idle=48, fieldBlocks=3, dotRows=5, tiles=[[64, 64, 2]])),
    Case(21, 35, 150, "two passes, 100 (tiles 64 + 36) and 50: both gradient kernels accumulate",
         dict(KC=16, chunks=[16, 16, 2], tiles=[[64, 36], [50]]), pass_size=100),
    Case(32, 16, 130, "KC = 7: 7 + 7 + 1; q = QM = 32", dict(KC=7, chunks=[7, 7, 1], threads=256, own=224, idle=32, QM=32)),
    Case(25, 24, 130, "KC = 11: 11 + 11 + 1; the first q of QM = 32", dict(KC=11, chunks=[11, 11, 1], threads=320, own=275, idle=45, QM=32)),
    Case(24, 14, 130, "KC = 12: 12 + 1; q = QM = 24", dict(KC=12, chunks=[12, 1], threads=320, own=288, idle=32, QM=24)),
    Case(9, 58, 130, "KC = 56: 56 + 1; 504 of 512 threads; odd P", dict(KC=56, chunks=[56, 1], threads=512, own=504, idle=8, QM=24, oddP=1)),
    Case(8, 66, 130, "KC = 64: 64 + 1; exactly 512 threads, none idle; q = QM = 8", dict(KC=64, chunks=[64, 1], threads=512, own=512, idle=0, QM=8)),
    Case(5, 67, 130, "KC = 64: 64 + 2; L q = 335 puts ar_field_kernel in a second block",
         dict(KC=64, chunks=[64, 2], threads=320, own=320, idle=0, fieldBlocks=2)),
    Case(21, 2, 130, "one pair; site 0 has no chunk", dict(KC=16, chunks=[1], fieldBlocks=1, dotRows=1)),
    Case(2, 3, 130, "smallest alphabet", dict(KC=64, chunks=[2], threads=128, own=128, QM=8)),
    Case(21, 2, 1, "a single sequence", dict(tiles=[[1]])),
    Case(24, 14, 64, "exactly one full tile; two chunks", dict(chunks=[12, 1], tiles=[[64]])),
    Case(5, 67, 130, "site 40 saturates: a field of +800 makes exp underflow to 0 for the other states",
         dict(KC=64, chunks=[64, 2]), saturate=(40, 2, 800.0)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------- the gradient geometry behind a program
def compile_plan_driver(directory):
    """tests/ar_plan_driver.cpp compiled with the host compiler -> driver(q) = dict(KC, threads, lds, tile, budget, maxThreads)"""
    exe = os.path.join(str(directory), "ar_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-fast-math", "-ffp-contract=off", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "ar_plan_driver.cpp")])
    cache = {}

    def driver(q):
        if q not in cache:
            v = [int(t) for t in subprocess.check_output([exe, str(q)]).split()]
            assert len(v) == 7 and v[0] == q
            cache[q] = dict(zip(["KC", "threads", "lds", "tile", "budget", "maxThreads"], v[1:]))
        return dict(cache[q])

    return driver


def plan_of(case, driver):
    """ar_plan.h's numbers for the case's q and what they make of its shape"""
    p = driver(case.q)
    N, L, q, KC, tile = case.N, case.L, case.q, p["KC"], p["tile"]
    p["chunks"] = [min(KC, L - 1 - k0) for k0 in range(0, L - 1, KC)]
    p["own"] = KC * q
    p["idle"] = p["threads"] - KC * q
    p["fieldBlocks"] = -(-L * q // FIELD_THREADS)
    p["dotRows"] = -(-case.P // DOT_STRIDE)
    p["pass"] = min(case.pass_size, N) if case.pass_size else N
    p["passes"] = -(-N // p["pass"])
    p["tiles"] = [[min(tile, nq - n0) for n0 in range(0, nq, tile)] for nq in (min(p["pass"], N - f) for f in range(0, N, p["pass"]))]
    p["QM"] = 8 if q <= 8 else 24 if q <= 24 else 32
    p["oddP"] = case.P % 2
    return p


# ----------------------------------------------------------------------------- inputs
def alignment(case):
    """uint8 [N, L] with skewed state frequencies (per site its own): the buckets of a pair differ in size, some are empty"""
    rng = np.random.default_rng(7100 + 100 * case.q + case.L + case.N)
    pr = rng.random((case.L, case.q)) ** 3 + 0.02
    cdf = np.cumsum(pr / pr.sum(axis=1, keepdims=True), axis=1)
    r = rng.random((case.N, case.L))
    return np.ascontiguousarray((r[:, :, None] > cdf[None, :, :-1]).sum(axis=2).astype(np.uint8))


def weights(case):
    """float64 weights over four decades; from 8 sequences on, three of them exactly 0"""
    rng = np.random.default_rng(9100 + case.N + case.q)
    w = 10.0 ** rng.uniform(-4.0, 0.0, case.N)
    if case.N >= 8:
        w[rng.choice(case.N, 3, replace=False)] = 0.0
    return w


def parameters(case):
    """packed x: normal, standard deviation SCALE; the saturating field entry on top"""
    rng = np.random.default_rng(11100 + 10 * case.L + case.q)
    x = rng.normal(0.0, SCALE, case.P)
    if case.saturate:
        l, b, v = case.saturate
        x[l * case.q + b] = v
    return x


# ----------------------------------------------------------------------------- the reference
class Reference:
    pass


def dot_depth(n):
    return -(-n // DOT_STRIDE) + 16


def dot_bound(n, sum_abs):
    """bound of sqrt(dot)^2 against the exact sum of the n products (module docstring)"""
    return gamma(dot_depth(n) + 2, U) * float(sum_abs)


def reference(case, plan):
    """-> Reference: fx, fx_bound, g (longdouble [P]), bound, A, pen (float64 [P]), m (int64 [P]), R64 ([N, L, q]) and the inputs"""
    N, L, q, P = case.N, case.L, case.q, case.P
    Lq, qq = L * q, q * q
    X, w, x = alignment(case), weights(case), parameters(case)
    Xi = X.astype(np.int64)
    passes, pass_size = plan["passes"], plan["pass"]
    wL = w.astype(LD)
    W = wL / fsum_ld(wL)
    h = x[:Lq].reshape(L, q)
    Jb = x[Lq:].reshape(L * (L - 1) // 2, q, q)

    # u and its sum of |terms|
    Ux = np.zeros((N, L, q), dtype=LD)
    Uabs = np.zeros((N, L, q))
    for l in range(L):
        Ux[:, l] = h[l].astype(LD)
        Uabs[:, l] = np.abs(h[l])
        if l:
            T = Jb[[pair_index(L, k, l) for k in range(l)]][np.arange(l)[None, :], Xi[:, :l]]      # [N, l, q]
            Ux[:, l] += T.astype(LD).sum(axis=1)
            Uabs[:, l] += np.abs(T).sum(axis=1)
    d = Ux - Ux.max(axis=2, keepdims=True)
    Z = np.exp(d).sum(axis=2)
    lz = np.log(Z)
    c = d - lz[:, :, None]
    p = np.exp(c)
    onehot = np.zeros((N, L, q))
    np.put_along_axis(onehot, Xi[:, :, None], 1.0, axis=2)
    pm = np.where(onehot > 0, np.expm1(c), p)                  # p - [s = b] without the cancellation at p near 1
    R = W[:, None, None] * pm

    # the library functions over the case's arguments (results that do not underflow; those are the floor's)
    with np.errstate(under="ignore"):
        exp_ulps = 0.0
        for a in (d.astype(np.float64).ravel(), c.astype(np.float64).ravel()):
            a = a[a > -700.0]
            exp_ulps = max(exp_ulps, ulps_off(np.exp(a), np.exp(a.astype(LD))))
        Z64 = Z.astype(np.float64).ravel()
        log_ulps = ulps_off(np.log(Z64), np.log(Z64.astype(LD)))
    eps_exp = EXP_FACTOR * max(exp_ulps, 0.5) * 2 * U
    eps_log = EXP_FACTOR * max(log_ulps, 0.5) * 2 * U

    up = 1 + 2.0 ** -10                                        # longdouble roundings of the reference, float64 ones of the bound
    d64, c64, P64 = np.abs(d).astype(np.float64), np.abs(c).astype(np.float64), p.astype(np.float64)
    du = gamma(np.arange(L), U)[None, :, None] * Uabs * up
    delta = du + U * (d64 + 2 * du.max(axis=2, keepdims=True)) * up
    rho_z = (P64 * delta).sum(axis=2) * up + eps_exp + gamma(q - 1, U) + q * ETA
    dlz = rho_z / (1 - rho_z) + eps_log * np.abs(lz).astype(np.float64) * up
    theta = delta + dlz[:, :, None] + U * c64 * up + eps_exp
    assert theta.max() < 0.25
    rel = theta / (1 - theta)
    W64 = W.astype(np.float64) * up
    R64 = R.astype(np.float64)
    absR = np.abs(R64) * up
    g2 = gamma(N + 2, U)
    ER = (W64[:, None, None] * P64 * rel * (1 + g2) + g2 * absR + 2 * ETA) * up

    # element sums
    oh = onehot.reshape(N, Lq)
    V = R.reshape(N, Lq)
    G = exact_group_sums(oh, V)
    col = exact_group_sums(np.ones((N, 1)), V)[0]
    AG, EG = oh.T @ absR.reshape(N, Lq), oh.T @ ER.reshape(N, Lq)
    mG = oh.sum(axis=0).astype(np.int64).reshape(L, q)
    iu, ju = np.triu_indices(L, 1)
    assert all(pair_index(L, int(k), int(l)) == i for i, (k, l) in enumerate(zip(iu[:L], ju[:L])))

    def blocks(M):          # [L q, L q] -> [pairs, a, b] = M[(k, a)][(l, b)], k < l
        return M.reshape(L, q, L, q).transpose(0, 2, 1, 3)[iu, ju]

    xL = x.astype(LD)
    g = np.zeros(P, dtype=LD)
    A, E, pen = np.zeros(P), np.zeros(P), np.zeros(P)
    m = np.zeros(P, dtype=np.int64)
    g[:Lq] = 2 * LD(LAMBDA_H) * xL[:Lq] + col
    g[Lq:] = 2 * LD(LAMBDA_J) * xL[Lq:] + blocks(G).ravel()
    A[:Lq], A[Lq:] = absR.reshape(N, Lq).sum(axis=0), blocks(AG).ravel()
    E[:Lq], E[Lq:] = ER.reshape(N, Lq).sum(axis=0), blocks(EG).ravel()
    pen[:Lq], pen[Lq:] = np.abs(2 * LAMBDA_H * x[:Lq]), np.abs(2 * LAMBDA_J * x[Lq:])
    m[:Lq] = N
    m[Lq:] = np.broadcast_to(mG[iu][:, :, None], (len(iu), q, q)).ravel()

    ref = Reference()
    ref.case, ref.plan, ref.X, ref.w, ref.x, ref.R64 = case, plan, X, w, x, R64
    ref.exp_ulps, ref.log_ulps, ref.eps_exp, ref.eps_log = exp_ulps, log_ulps, eps_exp, eps_log
    ref.iu, ref.ju = iu, ju
    ref.g, ref.A, ref.pen, ref.m = g, A, pen, m
    ref.bound = gamma(m + passes + 2, U) * (A + pen) + E * up + m * (CUT_OFF + 2 * ETA) + OWN * (A + pen)

    site = np.take_along_axis(c, Xi[:, :, None], axis=2)[:, :, 0]
    terms = -W[:, None] * site
    reg = LD(LAMBDA_H) * fsum_ld(xL[:Lq] * xL[:Lq]) + LD(LAMBDA_J) * fsum_ld(xL[Lq:] * xL[Lq:])
    ref.fx = fsum_ld(terms) + reg
    eps_site = np.take_along_axis(delta, Xi[:, :, None], axis=2)[:, :, 0] + dlz + U * np.abs(site).astype(np.float64) * up
    FA = float(np.sum(np.abs(terms))) * up
    depth_f = (L - 1) + (N + 2) + -(-pass_size // FIELD_THREADS) + 8 + passes + 2
    ref.fx_A = FA + float(reg)
    ref.fx_bound = float(np.sum(W64[:, None] * eps_site)) * up + gamma(depth_f, U) * FA + gamma(dot_depth(max(Lq, P - Lq)) + 4, U) * float(reg) * up + OWN * ref.fx_A
    return ref


# ----------------------------------------------------------------------------- naming
def element_of(case, e):
    """packed index -> ("field", l, None, b, None) or ("coupling", k, l, a, b): a at the earlier site k"""
    L, q = case.L, case.q
    if e < L * q:
        return ("field", e // q, None, e % q, None)
    p, t = divmod(e - L * q, q * q)
    iu, ju = np.triu_indices(L, 1)
    return ("coupling", int(iu[p]), int(ju[p]), t // q, t % q)


def index_of(case, k, l, a, b):
    return case.L * case.q + pair_index(case.L, k, l) * case.q * case.q + a * case.q + b


def writer_of(ref, e):
    """the kernel, workgroup and thread that write element e, and the chunk of earlier sites of a coupling"""
    case, KC = ref.case, ref.plan["KC"]
    kind, k, l, a, b = element_of(case, e)
    if kind == "field":
        return dict(kernel="ar_field_kernel", block=(int(e) // FIELD_THREADS,), thread=int(e) % FIELD_THREADS, chunk=None)
    chunk = k // KC
    return dict(kernel="ar_grad_kernel", block=(chunk, case.L - 1 - l), thread=(k - chunk * KC) * case.q + b, chunk=chunk)


class Failure:
    def __init__(self, ref, e, dev, ratio):
        self.index, self.ratio = int(e), float(ratio)
        self.kind, self.k, self.l, self.a, self.b = element_of(ref.case, e)
        self.dev, self.ref, self.bound, self.m = float(dev), float(ref.g[e]), float(ref.bound[e]), int(ref.m[e])
        self.writer = writer_of(ref, e)

    def __repr__(self):
        where = "field (site %d, b=%d)" % (self.k, self.a) if self.kind == "field" else "coupling (pair %d < %d; a=%d, b=%d)" % (self.k, self.l, self.a, self.b)
        w = self.writer
        return "%s element %d: device %.17g, reference %.17g, off by %.3e = %.3g x bound %.3e; %d addends; written by %s block %s thread %d%s" % (
            where, self.index, self.dev, self.ref, abs(self.dev - self.ref), self.ratio, self.bound, self.m, w["kernel"], w["block"], w["thread"],
            "" if w["chunk"] is None else ", chunk %d" % w["chunk"])


class Audit:
    """checked: elements compared (= P); worst: the largest |error| / bound; failing: the indices out of bound; failures: the
    worst of them by name; fx_ratio: |fx error| / its bound"""

    def __init__(self, case, checked, ratios, failing, failures, fx_err, fx_bound):
        self.case, self.checked, self.ratios, self.failing, self.failures = case, checked, ratios, failing, failures
        nan = np.isnan(ratios)
        self.worst, self.worst_index = (float("nan"), int(np.argmax(nan))) if nan.any() else (float(np.max(ratios)), int(np.argmax(ratios)))
        self.fx_err, self.fx_bound, self.fx_ratio = fx_err, fx_bound, fx_err / fx_bound

    @property
    def ok(self):
        return len(self.failing) == 0 and self.fx_ratio <= 1.0

    def summary(self):
        return "%s: %d of %d elements checked, worst |error| / bound %.4f at element %d, %d out of bound; fx off by %.3e of bound %.3e (%.4f)" % (
            self.case.name, self.checked, self.case.P, self.worst, self.worst_index, len(self.failing), self.fx_err, self.fx_bound, self.fx_ratio)

    def report(self):
        lines = [self.summary()] + [repr(f) for f in self.failures]
        if not self.fx_ratio <= 1.0:
            lines.append("fx out of bound")
        return "\n".join(lines)


def audit(ref, fx, g, named=12):
    """fx, g: what the evaluation returned.  Every one of the P elements is compared; nothing is exempt."""
    case = ref.case
    g = np.asarray(g)
    assert g.shape == (case.P,) and g.dtype == np.float64
    err = np.abs(g.astype(LD) - ref.g).astype(np.float64)
    assert np.all(ref.bound > 0)
    ratios = err / ref.bound
    checked = int(np.count_nonzero(ratios <= 1.0) + np.count_nonzero(~(ratios <= 1.0)))
    failing = np.flatnonzero(~(ratios <= 1.0))
    order = failing[np.argsort(-np.nan_to_num(ratios[failing], nan=np.inf))][:named]
    failures = [Failure(ref, e, g[e], ratios[e]) for e in order]
    fx_err = abs(float(LD(fx) - ref.fx))
    return Audit(case, checked, ratios, failing, failures, fx_err if fx_err == fx_err else np.inf, ref.fx_bound)


def assert_within_bounds(ref, fx, g):
    """what the GPU test asserts of a device evaluation -> the number of elements checked"""
    a = audit(ref, fx, g)
    print(a.summary())
    assert a.checked == ref.case.P
    assert a.ok, a.report()
    return a.checked


def gnorm_ratio(g, gnorm):
    """|gnorm^2 - sum g^2| / dot_bound, the sum in longdouble over the g given (the device's own)"""
    gL = np.asarray(g, dtype=np.float64).astype(LD)
    s = fsum_ld(gL * gL)
    err = abs(float(LD(gnorm) * LD(gnorm) - s))
    return (err if err == err else np.inf) / dot_bound(len(gL), s)


# ----------------------------------------------------------------------------- the dot kernels' order in float64
def dot_emulated(a, b, stride_loop=True):
    """ar_dot_kernel and ar_dot_final_kernel with NumPy: thread i of 65 536 adds a[j] b[j], j = i, i + 65 536, ... ascending;
    a tree over the 256 threads of a block; a tree over the 256 blocks.  stride_loop False: the first 65 536 elements only."""
    prod = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)
    rows = -(-len(prod) // DOT_STRIDE)
    prod = np.concatenate([prod, np.zeros(rows * DOT_STRIDE - len(prod))]).reshape(rows, DOT_STRIDE)
    part = np.zeros(DOT_STRIDE)
    for r in range(rows if stride_loop else 1):
        part = part + prod[r]
    sh = part.reshape(256, 256).copy()              # [block, thread]
    wd = 128
    while wd > 0:
        sh[:, :wd] = sh[:, :wd] + sh[:, wd:2 * wd]
        wd >>= 1
    fin = sh[:, 0].copy()
    wd = 128
    while wd > 0:
        fin[:wd] = fin[:wd] + fin[wd:2 * wd]
        wd >>= 1
    return float(fin[0])
