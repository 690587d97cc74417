"""TEST INFRASTRUCTURE ONLY -- host reference for ONE plmDCA evaluation (fx, g) of the stage chain in pydca_amd/csrc/plm_stages.h
(expand, logits, softmax scan, scatter, slab sums, fold), with no GPU dependency: tests/test_plm_eval_audit.py feeds it what the
device returned, tests/test_plm_eval_audit_host.py pins it on the CPU.

reference(case) evaluates the engine's semantics in np.longdouble with exact sums over the sequences:

    W from the packed x;  S[n] = sum_j W[j q + x_nj];  z = S + h (+ p_{n-1});  p = softmax(z);  R = w (p - delta);
    G[(j,b)][c] = sum_{n >= halo, x_nj = b} R[n][c];
    g[J_ij(a,b)] = (2 lambda_J x + G[(j,b)][(i,a)]) + G[(i,a)][(j,b)];   g[h_i(a)] = 2 lambda_h h + sum_{n >= halo} R[n][(i,a)];
    fx = - sum_{n >= halo, i} w_n log p_n(x_ni) + lambda_h sum h^2 + lambda_J sum J^2.

The carried chain always starts at row 0 from a zero carry (rows < halo warm it and are not summed); DCA_CARRY_EXACT has no
carry.  The device's chunked scan is held to this SERIAL chain, its start-up error is a term of the bound.  fx is a math.fsum of
the terms' leading doubles (two passes: fsum rounds to a double) plus the longdouble sum of their remainders.  The bucket sums of G are formed exactly as well, but
not through math.fsum (2 10^8 addends at 3000 x 60): every |R| <= 1 is cut into five 26-bit fixed-point limbs (the cut is exact
in longdouble), the limbs are integers below 2^27, so their sums over up to 2^15 sequences stay below 2^53 and a float64 matrix
product with the one-hot state matrix adds them EXACTLY in whatever order the BLAS takes; what is cut off is below 2^-131 per
addend and enters the bound as such.  exact_group_sums_fsum is the same sum through math.fsum; the host test holds the two equal.

Dyadic parameters (fields: multiples of 2^-6 in [-2, 2], couplings: multiples of 2^-8 in [-1/4, 1/4]): every partial sum of
S and of S + h is a multiple of 2^-8 below (L - 1) / 4 + 2, i.e. an integer below 2^24 in units of 2^-8 -- exact in float32 in
any order, the site-pair alphabet's re-associated one included (parameters() asserts the magnitudes).  A logits kernel that adds
the right rows reproduces S exactly, one that does not is off by at least 2^-8.  Weights are 1 / k, k in 1 .. 8, rounded once to
the engine's type T; lambda_h = 3/4, lambda_J = 3 are dyadic.

ELEMENT BOUND, from the device's rounding sequence (u = unit roundoff of T, gamma(k) = k u / (1 - k u)):

    bound[e] = gamma(m_e + 2) A[e] + sum_{addends} w_n E_p[n, site, state] + m_e (2^-131 + eta_T)

A[e] = |2 lambda x_e| + sum |R| over the m_e addends R of element e (both conditionals of a coupling).  First term: an addend is
formed with one rounding (r = fl(w p^) - w: the subtraction; the product's rounding is in E_p), the m_e addends are then added
in SOME tree -- per bucket in sequence order, per tile range into slabs, slabs in ascending order, the site-pair accumulators
marginalised, the canonical blocks of the float64 mode; adding a zero is exact -- which has m_e - 1 additions, and the fold adds
the regulariser term (one product rounding, 2 lambda exact) and the second conditional: two more.  No path from an addend to
the result sees more than m_e + 2 roundings (Higham, Accuracy and Stability, section 4.2).  Last term: the reference's cut-off
and the flush of results below the smallest normal eta_T.  The price of a worst case over all orders: A is about m_e typical
addends, so ONE missing addend stands out only while m_e (m_e + 2) u < 1 (4096 addends in float32); the alignments' skewed state
frequencies give every site a bucket far below that (tests/test_plm_eval_audit_host.py asserts it).

E_p, the error of one device probability p^_n[a] of site i against the exact chain:
  * z' = fl(z + p^_{n-1}) : u (|z|max + 1) absolute on the logit (z = S + h itself is exact, see above); absent without carry;
  * d = fl(z' - max z')  : u D, D = the spread of the site's logits;
  * t = exp(d)           : eps_exp relative; an absolute error delta of the argument is a relative error delta of t.
    eps_exp = 4 x (largest error in ulps of np.exp in T against the longdouble exp over the arguments of the case, not below the
    1/2 ulp of a correctly rounded function) x 2 u.  The device library is another implementation of the same function, both are
    documented to about an ulp: factor 4.  rho = eps_exp + u D + u (|z|max + 1);
  * sum of q terms, 1 / sum, t * (1 / sum) : gamma(q - 1) + 2 u relative; numerator and denominator both carry rho:
    phi = 2 rho + gamma(q - 1) + 2 u is the relative error made AT step n;
  * the error e_{n-1} of the carry perturbs the logits by e_{n-1}.  d softmax = diag(p) - p p^T maps a perturbation v to
    p_a (v_a - <v>_p): its 1-norm is at most half the spread of v, and spread(v) <= ||v||_1, so the 1-norm of the carried
    error halves per step: s_n = phi_n + s_{n-1} / 2 <= 2 max_n phi_n + 2^-(n - ws + 1) s_start.  A chunk of the
    chunked scan that starts at row ws > 0 from a ZERO carry drops a carry of spread <= 1: s_start = 1, i.e. 2^-warm at its
    first owned row -- the start-up term.  The serial chain and the exact mode have none.  Element a of step n then errs by
    p_a (phi_n + s_{n-1}): Theta = phi_n + 2 max phi + 2^-(n - ws) [ws > 0], taken as Theta / (1 - Theta) for the higher orders;
  * r = fl(w p^): u p (1 + Theta).
  E_p = p Theta / (1 - Theta) + u p (1 + Theta).

fx: -fl(w fl(log p^)) summed in double-double with the regulariser's double products: the bound is
sum w Theta / (1 - Theta) + (eps_log + u) sum |w log p| + 2^-50 (sum |w log p| + regulariser), eps_log measured like eps_exp.

audit() checks ALL P elements (it asserts the count) and names what fails: parameter kind, sites, states, and per conditional
the 512-byte column strip, the scatter kernel's site group and the (tile, split) of the first and last addend; where one missing
or extra addend, one missing slab or one halo row explains the difference within the bound, it names that too."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the reference needs the 64-bit significand of x87 long double"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 128                                  # kNC: sequences per scatter tile
LAMBDA_H, LAMBDA_J = 0.75, 3.0
CARRY = {"exact": 0, "chunked": 1, "serial": 2}          # DCA_CARRY_*
EXP_FACTOR = 4.0
LIMB_BITS, LIMBS = 26, 5
CUT_OFF = 2.0 ** -(LIMB_BITS * LIMBS + 1)

SHAPE = ["N", "L", "q", "elemBytes", "halo", "chunkArg", "warmArg", "carryMode", "stripWorld", "stripRank", "strips"]
KNOBS = ["scatterRem", "scatterSplit", "scatterCanon", "scatterWaves", "plmPairs", "scatterMerge", "foldMerge", "fuseFx"]
KNOB_ENV = {"DCA_SCATTER_REM": "scatterRem", "DCA_SCATTER_SPLIT": "scatterSplit", "DCA_SCATTER_CANON": "scatterCanon",
            "DCA_SCATTER_WAVES": "scatterWaves", "DCA_PLM_PAIRS": "plmPairs", "DCA_SCATTER_MERGE": "scatterMerge",
            "DCA_FOLD_MERGE": "foldMerge", "DCA_PLM_FUSE_FX": "fuseFx"}
SCALARS = ["cS0", "cS1", "Lloc", "oLo", "oHi", "pairBegin", "pairEnd", "chunk", "warm", "numScanChunks", "numScatChunks", "P", "Cs", "pairs",
           "gUnits", "pairJT", "Wrows", "Grows", "Npad", "NT", "scatJW", "scatWaves", "scatSplit", "scatChunksPerSplit", "scatBlockChunks",
           "scatPerBlock", "scatRemCT", "scatRemSplit", "scatRemChunksPerSplit", "nFxPart", "nRegPart", "grecvTotal", "xsendTotal", "xrecvTotal"]


def unit_roundoff(dtype):
    return 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53


def gamma(k, u):
    return k * u / (1.0 - k * u)


def num_params(L, q):
    return L * q + (L * (L - 1) // 2) * q * q


# ----------------------------------------------------------------------------- the case table
class Case:
    """One row of the table: shape, precision, configuration, what it reaches, and the plan facts that say so."""

    def __init__(self, bits, q, N, L, reaches, facts, env=None, halo=0, mode="chunked", chunk=0, head_of=None):
        self.bits, self.q, self.N, self.L, self.reaches, self.facts = bits, q, N, L, reaches, facts
        self.head_of = head_of            # a case whose first N sequences (and their weights) this one takes
        self.env, self.halo, self.mode, self.chunk = dict(env or {}), halo, mode, chunk
        self.dtype = np.dtype(np.float32 if bits == 32 else np.float64)
        self.P = num_params(L, q)
        extra = "".join("_%s%s" % (k.replace("DCA_", "").lower(), v) for k, v in sorted(self.env.items()))
        extra += ("_halo%d" % halo if halo else "") + ("_chunk%d" % chunk if chunk else "") + ("_" + mode if mode != "chunked" else "")
        self.name = "f%d_q%d_%dx%d%s" % (bits, q, N, L, extra)

    def __repr__(self):
        return self.name


# facts: plan columns (tests/plm_plan_driver.cpp) and the derived `strips` (512-byte column strips), `dealPairs` ((strip, split)
# pairs dealt to the XCDs), `seqBlocks` (sequence blocks of the logits kernel), `logitTiles`, `siteGroups` (scatter), `scanBlocks`
CASES = [
    Case(32, 21, 300, 7, "2 strips; (strip, split) pairs dealt to the XCDs; scan chunks of 32 shorter than the 40-step warm-up",
         dict(strips=2, dealPairs=1, chunk=32, warm=40)),
    Case(32, 21, 3000, 60, "10 strips: logits decode with 8 full + 2 left-over strips; 4 sequence blocks; split 2 in blockIdx.y; two slabs folded on the fly",
         dict(strips=10, seqBlocks=4, scatSplit=2, scatRemCT=0, dealPairs=0)),
    Case(32, 21, 3000, 60, "left-over strips behind the main ones in one launch; plm_sum_slabs_cols_kernel",
         dict(strips=10, scatRemCT=2, dealPairs=0), env={"DCA_SCATTER_REM": "1"}),
    Case(32, 21, 4500, 49, "9 strips, split 3: streaming plm_sum_slabs_kernel", dict(strips=9, scatSplit=3, scatRemCT=0)),
    Case(32, 5, 10000, 13, "site pairs, tile 10, odd L, one strip, split 6: the 4-slab unrolled loop plus a remainder slab",
         dict(pairs=1, pairJT=10, strips=1, scatSplit=6)),
    Case(32, 5, 641, 43, "pair tile 11, two tiles; odd L; 640 + 1 sequences", dict(pairs=1, pairJT=11, logitTiles=2, seqBlocks=2)),
    Case(32, 5, 641, 47, "pair tile 12, two tiles; odd L; 640 + 1 sequences", dict(pairs=1, pairJT=12, logitTiles=2, seqBlocks=2)),
    Case(32, 5, 641, 49, "pair tile 10, three tiles; odd L; 640 + 1 sequences", dict(pairs=1, pairJT=10, logitTiles=3, seqBlocks=2)),
    Case(32, 5, 300, 65, "scatter groups of 64 sites + 1; second site block of the scan with a ragged 16-byte tail",
         dict(pairs=1, siteGroups=2, scanBlocks=2)),
    Case(32, 5, 300, 129, "scatter groups of 64 sites + 1; third site block of the scan with a ragged 16-byte tail",
         dict(pairs=1, siteGroups=3, scanBlocks=3)),
    Case(32, 5, 769, 27, "per-site q = 5 blocks; 768 + 1 sequences", dict(pairs=0, seqBlocks=2), env={"DCA_PLM_PAIRS": "0"}),
    Case(32, 21, 200, 65, "scan tail block of one site (84 bytes rounded up to 96)", dict(scanBlocks=2)),
    Case(32, 21, 1000, 33, "halo rows warm the chain and are left out of every sum", dict(numScatChunks=8), halo=64),
    Case(32, 5, 1000, 33, "halo rows warm the chain and are left out of every sum (site pairs)", dict(pairs=1, numScatChunks=8), halo=64),
    Case(32, 21, 1300, 9, "chunk 256: last chunk partial, chunk count not a multiple of the 4 waves", dict(chunk=256, numScanChunks=6), chunk=256),
    Case(32, 21, 1300, 9, "chunk 128: last chunk partial, chunk count not a multiple of the 4 waves", dict(chunk=128, numScanChunks=11), chunk=128),
    Case(32, 21, 1300, 9, "the serial chain", dict(chunk=1300, numScanChunks=1), mode="serial"),
    Case(32, 21, 1300, 9, "no carry", dict(warm=0), mode="exact"),
    Case(64, 21, 300, 55, "one workgroup per (strip, site group), 8 waves; plm_colsum_parts_kernel", dict(scatWaves=8, scatPerBlock=0, scatSplit=1)),
    Case(64, 21, 300, 150, "the same with 16 waves", dict(scatWaves=16, scatPerBlock=0, scatSplit=1)),
    Case(64, 5, 300, 10, "4-wave gather block", dict(scatWaves=4, scatPerBlock=0), env={"DCA_SCATTER_WAVES": "4"}),
    Case(64, 5, 700, 65, "per-chunk column sums taken inside the scan kernel", dict(pairs=0, scatPerBlock=0)),
    Case(64, 21, 16385, 4, "two canonical blocks in one workgroup; the second holds one sequence and goes through scatter_add_site_f64",
         dict(scatBlockChunks=128, numScatChunks=129, scatPerBlock=0, scatSplit=1)),
    Case(64, 21, 33000, 4, "slab per block (3 slabs, ordered sum)", dict(scatPerBlock=1, scatSplit=3, scatChunksPerSplit=128)),
    Case(64, 21, 33000, 4, "the one-workgroup form of the same order", dict(scatPerBlock=0, scatSplit=1, scatBlockChunks=128), env={"DCA_SCATTER_CANON": "1"}),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------- the launch planner behind a C call
def compile_plan_driver(directory):
    """tests/plm_plan_driver.cpp compiled as tests/test_plm_plan_host.py compiles it -> the C function"""
    so = os.path.join(str(directory), "libplm_plan_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-fast-math", "-ffp-contract=off", "-shared", "-fPIC", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", so, os.path.join(ROOT, "tests", "plm_plan_driver.cpp")])
    fn = C.CDLL(so).plm_plan_driver
    fn.restype = None
    return fn


def plan_of(case, driver):
    """the planner's decisions for the case (SCALARS) and the derived facts"""
    ks = np.load(os.path.join(ROOT, "tests", "golden", "plm_plans.npz"))["kernel_shapes"].tolist()
    shape = dict(N=case.N, L=case.L, q=case.q, elemBytes=case.dtype.itemsize, halo=case.halo, chunkArg=case.chunk, warmArg=0,
                 carryMode=CARRY[case.mode], stripWorld=1, stripRank=0, strips=0)
    knobs = {k: -1 for k in KNOBS}
    for name, v in case.env.items():
        knobs[KNOB_ENV[name]] = int(v)
    buf = (C.c_longlong * (len(SCALARS) + 2 + 3))()
    driver((C.c_int * len(SHAPE))(*[shape[n] for n in SHAPE]), (C.c_int * len(KNOBS))(*[knobs[n] for n in KNOBS]), (C.c_int * 6)(*ks), 1, buf)
    p = {n: int(buf[i]) for i, n in enumerate(SCALARS)}
    cw = 512 // case.dtype.itemsize
    slot = 1 if case.q == 21 else 2 if p["pairs"] else 0
    p["strips"] = -(-p["Cs"] // cw)
    p["dealPairs"] = int(p["strips"] < 8 or p["scatPerBlock"])
    p["seqBlocks"] = p["Npad"] // ks[slot]
    p["logitTiles"] = -(-p["gUnits"] // (p["pairJT"] if p["pairs"] else ks[3 + slot]))
    p["siteGroups"] = -(-p["gUnits"] // (p["scatWaves"] * p["scatJW"]))
    p["scanBlocks"] = -(-case.L // 64)
    return p


# ----------------------------------------------------------------------------- inputs
def alignment(case):
    """uint8 [N, L] with skewed state frequencies (per site its own), so that the bucket sizes differ across states and sites"""
    if case.head_of is not None:
        return np.ascontiguousarray(alignment(case.head_of)[:case.N])
    rng = np.random.default_rng(7000 + 100 * case.q + case.L + case.N)
    pr = rng.random((case.L, case.q)) ** 3 + 0.02
    cdf = np.cumsum(pr / pr.sum(axis=1, keepdims=True), axis=1)
    r = rng.random((case.N, case.L))
    X = (r[:, :, None] > cdf[None, :, :-1]).sum(axis=2).astype(np.uint8)
    return np.ascontiguousarray(X)


def weights(case):
    """float64 1 / k, k in 1 .. 8 (set_weights takes doubles; the engine rounds them once to its type)"""
    if case.head_of is not None:
        return weights(case.head_of)[:case.N].copy()
    rng = np.random.default_rng(9000 + case.N)
    return 1.0 / rng.integers(1, 9, size=case.N).astype(np.float64)


def parameters(case):
    """packed x in the case's dtype: dyadic fields and couplings; asserts that every partial sum of S + h is exact in float32"""
    L, q = case.L, case.q
    rng = np.random.default_rng(11000 + 10 * L + q)
    h = rng.integers(-128, 129, size=L * q) / 64.0
    J = rng.integers(-64, 65, size=(L * (L - 1) // 2) * q * q) / 256.0
    assert np.abs(h).max() <= 2 and np.abs(J).max() <= 0.25
    # in units of 2^-8 every term is an integer; the largest partial sum of (L - 1) couplings and a field:
    assert (L - 1) * 64 + 2 * 256 < 2 ** 24, "partial sums of S + h leave float32's exact integers"
    return np.concatenate([h, J]).astype(case.dtype)


def expand(x, L, q):
    """W[(i,a)][(j,b)] = W[(j,b)][(i,a)] = J_ij(a,b) as float64 [L q, L q] (exact), and the fields [L, q]"""
    x = np.asarray(x, dtype=np.float64)
    iu, ju = np.triu_indices(L, 1)
    J = x[L * q:].reshape(len(iu), q, q)
    Wt = np.zeros((L, L, q, q))
    Wt[iu, ju] = J
    Wt[ju, iu] = J.transpose(0, 2, 1)
    return np.ascontiguousarray(Wt.transpose(0, 2, 1, 3)).reshape(L * q, L * q), x[:L * q].reshape(L, q)


def logit_sums(W, X, q):
    """S[n] = sum_j W[j q + x_nj] in float64: exact for the dyadic parameters"""
    N, L = X.shape
    S = np.zeros((N, W.shape[1]))
    for j in range(L):
        S += W[j * q + X[:, j].astype(np.int64)]
    return S


def one_hot(X, q, halo):
    """[N, L q] float64: 1 where x_nj = b, rows < halo zero"""
    N, L = X.shape
    oh = np.zeros((N, L * q))
    oh[np.arange(N)[:, None], np.arange(L)[None, :] * q + X] = 1.0
    oh[:halo] = 0.0
    return oh


def exact_group_sums(oh, V):
    """oh^T V with every sum exact up to CUT_OFF per addend: V longdouble, |V| <= 1 (module docstring)"""
    assert np.abs(V).max() <= 1 and oh.shape[0] < 2 ** 15 * 4
    acc = np.zeros((oh.shape[1], V.shape[1]), dtype=LD)
    r = V.astype(LD, copy=True)
    for k in range(1, LIMBS + 1):
        scale = LD(2.0) ** (LIMB_BITS * k)
        a = np.rint(r * scale)
        r -= a / scale
        acc += (oh.T @ a.astype(np.float64)).astype(LD) / scale
    assert np.abs(r).max() <= CUT_OFF
    return acc


def fsum_ld(values):
    """exact sum of longdoubles, rounded to longdouble: math.fsum of the leading doubles (it returns the exact sum rounded to a
    double; a second pass with that double taken off returns what it lost) + the longdouble sum of the remainders"""
    v = np.asarray(values, dtype=LD).ravel()
    hi = v.astype(np.float64)
    lst = hi.tolist()
    s1 = math.fsum(lst)
    return LD(s1) + LD(math.fsum(lst + [-s1])) + np.sum(v - hi.astype(LD))


def exact_group_sums_fsum(oh, V):
    """the same sums through math.fsum (small cases: the host test compares the two)"""
    out = np.zeros((oh.shape[1], V.shape[1]), dtype=LD)
    for k in range(oh.shape[1]):
        rows = np.flatnonzero(oh[:, k])
        for c in range(V.shape[1]):
            out[k, c] = fsum_ld(V[rows, c]) if len(rows) else 0
    return out


def chunk_starts(N, halo, chunk, warm, carry):
    """per scan chunk: first owned row s, end e, first walked row ws (plm_softmax_kernel)"""
    s = np.arange(halo, N, chunk)
    e = np.minimum(s + chunk, N)
    ws = np.maximum(0, s - warm) if carry else s.copy()
    return s, e, ws


def ulps_off(approx, exact):
    """|approx - exact| in units in the last place of approx's type"""
    return float(np.max(np.abs(approx.astype(LD) - exact) / np.spacing(np.abs(approx)).astype(LD))) if approx.size else 0.0


# ----------------------------------------------------------------------------- the reference
class Reference:
    pass


def reference(case, plan, sums="limbs"):
    """-> Reference: fx, fx_bound, g (longdouble [P]), bound, A (float64 [P]), m (int64 [P]) and what audit() needs to name things.
    plan: plan_of(case) (chunk and warm-up of the device's scan, the scatter geometry)."""
    N, L, q, halo, T = case.N, case.L, case.q, case.halo, case.dtype.type
    u = unit_roundoff(T)
    eta = float(np.finfo(T).tiny)
    X, x = alignment(case), parameters(case)
    wT = weights(case).astype(T)
    w = wT.astype(np.float64)
    W, h = expand(x, L, q)
    S = logit_sums(W, X, q)
    carry = case.mode != "exact"
    Lq = L * q

    # the chain, serial from row 0
    P = np.zeros((N, L, q), dtype=LD)
    spread = np.zeros((N, L))
    zmax = np.zeros((N, L))
    hL = h.astype(LD)
    p = np.zeros((L, q), dtype=LD)
    args = np.zeros((N, L, q), dtype=T)               # the arguments of exp, as the engine's type holds them
    for n in range(N):
        z = S[n].reshape(L, q).astype(LD) + hL
        if carry:
            z = z + p
        m = z.max(axis=1, keepdims=True)
        d = z - m
        t = np.exp(d)
        p = t / t.sum(axis=1, keepdims=True)
        P[n] = p
        args[n] = d
        spread[n] = (-d.min(axis=1)).astype(np.float64)
        zmax[n] = np.abs(z).max(axis=1).astype(np.float64)
    exp_ulps = ulps_off(np.exp(args), np.exp(args.astype(LD)))      # the accuracy of np.exp in T over the case's arguments
    del args
    px = np.take_along_axis(P, X[:, :, None].astype(np.int64), axis=2)[:, :, 0]
    logp = np.log(px)
    pxT = px.astype(T)
    log_ulps = ulps_off(np.log(pxT[pxT < 1]), np.log(pxT[pxT < 1].astype(LD)))
    eps_exp = EXP_FACTOR * max(exp_ulps, 0.5) * 2 * u
    eps_log = EXP_FACTOR * max(log_ulps, 0.5) * 2 * u

    # Theta[n, i]: relative error of the device's p^_n at site i (module docstring)
    rho = eps_exp + u * spread + (u * (zmax + 1) if carry else 0.0)
    phi = 2 * rho + gamma(q - 1, u) + 2 * u
    theta = phi.copy()
    if carry:
        theta += 2 * phi.max(axis=0, keepdims=True)
        s_, e_, ws_ = chunk_starts(N, halo, plan["chunk"], plan["warm"], True)
        for s0, e0, ws0 in zip(s_, e_, ws_):
            if ws0 > 0:
                theta[s0:e0] += (2.0 ** -(np.arange(s0, e0) - ws0).astype(np.float64))[:, None]
    assert theta.max() < 0.25
    rel = theta / (1 - theta)
    P64 = P.astype(np.float64)
    Ep = (P64 * (rel + u * (1 + theta))[:, :, None]).reshape(N, Lq)           # [N, L q]

    # R = w (p - delta)
    R = P * w.astype(LD)[:, None, None]
    np.put_along_axis(R, X[:, :, None].astype(np.int64), np.take_along_axis(R, X[:, :, None].astype(np.int64), axis=2) - w.astype(LD)[:, None, None], axis=2)
    R = R.reshape(N, Lq)
    oh = one_hot(X, q, halo)
    group = exact_group_sums if sums == "limbs" else exact_group_sums_fsum
    G = group(oh, R)
    own = np.zeros((N, 1))
    own[halo:] = 1.0
    col = group(own, R)[0]
    R64 = R.astype(np.float64)
    absR = np.abs(R64) * (1 + 2.0 ** -40)
    AG, EG = oh.T @ absR, oh.T @ (Ep * w[:, None])
    mG = oh.sum(axis=0).astype(np.int64)                                     # bucket sizes [L q]
    Acol, Ecol = absR[halo:].sum(axis=0), (Ep * w[:, None])[halo:].sum(axis=0)

    ref = Reference()
    ref.case, ref.plan, ref.X, ref.x, ref.w, ref.R64 = case, plan, X, x, w, R64
    ref.exp_ulps, ref.log_ulps, ref.eps_exp, ref.eps_log = exp_ulps, log_ulps, eps_exp, eps_log
    xL = x.astype(LD)
    iu, ju = np.triu_indices(L, 1)
    ref.iu, ref.ju = iu, ju

    def views(M):       # [L q, L q] -> ([pairs, a, b] = M[(j,b)][(i,a)], [pairs, a, b] = M[(i,a)][(j,b)])
        M4 = M.reshape(L, q, L, q)
        return M4.transpose(2, 0, 3, 1)[iu, ju], M4.transpose(0, 2, 1, 3)[iu, ju]

    g = np.zeros(case.P, dtype=LD)
    A = np.zeros(case.P)
    E = np.zeros(case.P)
    m_e = np.zeros(case.P, dtype=np.int64)
    g[:Lq] = 2 * LD(LAMBDA_H) * xL[:Lq] + col
    A[:Lq] = np.abs(2 * LAMBDA_H * x[:Lq].astype(np.float64)) + Acol
    E[:Lq] = Ecol
    m_e[:Lq] = N - halo
    v1, v2 = views(G)
    g[Lq:] = ((2 * LD(LAMBDA_J) * xL[Lq:].reshape(v1.shape) + v1) + v2).ravel()
    a1, a2 = views(AG)
    A[Lq:] = (np.abs(2 * LAMBDA_J * x[Lq:].astype(np.float64)).reshape(a1.shape) + a1 + a2).ravel()
    e1, e2 = views(EG)
    E[Lq:] = (e1 + e2).ravel()
    mrow = mG.reshape(L, q)
    m_e[Lq:] = (mrow[ju][:, None, :] + mrow[iu][:, :, None]).ravel()
    ref.g, ref.A, ref.m = g, A, m_e
    ref.bound = gamma(m_e + 2, u) * A + E + m_e * (CUT_OFF + eta)

    terms = (-(w.astype(LD))[:, None] * logp)[halo:]
    reg = LD(LAMBDA_H) * fsum_ld(xL[:Lq] * xL[:Lq]) + LD(LAMBDA_J) * fsum_ld(xL[Lq:] * xL[Lq:])
    ref.fx = fsum_ld(terms) + reg
    sum_abs = float(np.sum(np.abs(terms)))
    ref.fx_A = sum_abs + float(reg)
    ref.fx_bound = float(np.sum((w[:, None] * rel)[halo:])) + (eps_log + u) * (1 + 2 * u) * sum_abs + 2.0 ** -50 * ref.fx_A
    return ref


# ----------------------------------------------------------------------------- naming
def element_of(case, e):
    """packed index -> ("field", i, None, a, None) or ("coupling", i, j, a, b)"""
    L, q = case.L, case.q
    if e < L * q:
        return ("field", e // q, None, e % q, None)
    p, t = divmod(e - L * q, q * q)
    iu, ju = np.triu_indices(L, 1)
    return ("coupling", int(iu[p]), int(ju[p]), t // q, t % q)


def index_of(case, i, j, a, b):
    L, q = case.L, case.q
    return L * q + (i * (2 * L - i - 1) // 2 + (j - i - 1)) * q * q + a * q + b


def _where(ref, n, strip):
    """(n, tile, split) of owned sequence n for a column of `strip`"""
    p, t = ref.plan, (n - ref.case.halo) // NC
    rem = p["scatRemCT"] and strip >= p["strips"] - p["scatRemCT"]
    return (int(n), int(t), int(t // (p["scatRemChunksPerSplit"] if rem else p["scatChunksPerSplit"])))


def conditionals(ref, e):
    """the sums of G that element e reads: dicts with the row (site, state; state None = all of site 0's rows: the field sum), the
    column (site, state), its strip, the row's site group and the first and last addend as (n, tile, split)"""
    case, p = ref.case, ref.plan
    kind, i, j, a, b = element_of(case, e)
    cw = 512 // case.dtype.itemsize
    per_group = p["scatWaves"] * p["scatJW"] * (2 if p["pairs"] else 1)
    rows = [(0 if case.bits == 32 else None, None, i, a)] if kind == "field" else [(j, b, i, a), (i, a, j, b)]
    out = []
    for rs, rst, cs, cst in rows:
        ns = np.arange(case.halo, case.N) if rst is None else case.halo + np.flatnonzero(ref.X[case.halo:, rs] == rst)
        strip = (cs * case.q + cst) // cw
        out.append(dict(row_site=rs, row_state=rst, col_site=cs, col_state=cst, column=cs * case.q + cst, strip=strip,
                        site_group=None if rs is None else rs // per_group, addends=ns,
                        first=_where(ref, ns[0], strip) if len(ns) else None, last=_where(ref, ns[-1], strip) if len(ns) else None))
    return out


def explain(ref, e, diff):
    """one missing / extra addend, one missing slab or one summed halo row that accounts for diff = device - reference within
    the element's bound -> (what, view index, (n, tile, split)) or None"""
    tol, best = ref.bound[e], None
    conds = conditionals(ref, e)
    if len(conds) == 2:           # the same slab missing from both conditionals (their columns lie in one strip)
        split_of = [np.array([_where(ref, n, v["strip"])[2] for n in v["addends"]]) for v in conds]
        for s in np.intersect1d(*split_of):
            r = abs(diff + sum(ref.R64[v["addends"], v["column"]][sp == s].sum() for v, sp in zip(conds, split_of)))
            if r <= tol:
                best = (r, "missing slab", -1, (None, None, int(s)))
    for k, v in enumerate(conds):
        ns, c = v["addends"], v["column"]
        if len(ns):
            vals = ref.R64[ns, c]
            for what, target in (("missing addend", -vals), ("extra addend", vals)):
                r = np.abs(diff - target)
                t = int(np.argmin(r))
                if r[t] <= tol and (best is None or r[t] < best[0]):
                    best = (r[t], what, k, _where(ref, ns[t], v["strip"]))
            splits = np.array([_where(ref, n, v["strip"])[2] for n in ns])
            for s in np.unique(splits):
                r = abs(diff + vals[splits == s].sum())
                if np.count_nonzero(splits == s) > 1 and r <= tol and (best is None or r < best[0]):
                    best = (r, "missing slab", k, (None, None, int(s)))
        hs = np.arange(ref.case.halo) if v["row_state"] is None else np.flatnonzero(ref.X[:ref.case.halo, v["row_site"]] == v["row_state"])
        for n in hs:
            r = abs(diff - ref.R64[n, c])
            if r <= tol and (best is None or r < best[0]):
                best = (r, "halo row summed", k, (int(n), None, None))
    return None if best is None else best[1:]


class Failure:
    def __init__(self, ref, e, dev, ratio):
        self.index, self.ratio = int(e), float(ratio)
        self.kind, self.i, self.j, self.a, self.b = element_of(ref.case, e)
        self.dev, self.ref, self.bound = float(dev), float(ref.g[e]), float(ref.bound[e])
        self.views = conditionals(ref, e)
        self.explained = explain(ref, e, float(LD(dev) - ref.g[e]))

    def __repr__(self):
        s = "%s (i=%s, j=%s; a=%s, b=%s) element %d: device %.9g, reference %.9g, off by %.3e = %.3g x bound %.3e" % (
            self.kind, self.i, self.j, self.a, self.b, self.index, self.dev, self.ref, abs(self.dev - self.ref), self.ratio, self.bound)
        for v in self.views:
            s += "; sum of row (site %s, state %s) at column (site %d, state %d): strip %d, site group %s, %d addends, first (n, tile, split) %s, last %s" % (
                v["row_site"], "all" if v["row_state"] is None else v["row_state"], v["col_site"], v["col_state"], v["strip"], v["site_group"],
                len(v["addends"]), v["first"], v["last"])
        if self.explained:
            what, k, where = self.explained
            s += "; explained by: %s of %s at (n, tile, split) %s" % (what, "both sums" if k < 0 else "sum %d" % (k + 1), where)
        return s


class Audit:
    """checked: elements compared (= P); worst: largest |error| / bound; failing: indices out of bound; failures: the worst of
    them by name; fx_ratio: |fx error| / its bound"""

    def __init__(self, case, checked, ratios, failing, failures, fx_err, fx_bound):
        self.case, self.checked, self.failing, self.failures = case, checked, failing, failures
        self.worst, self.worst_index = (float(np.max(ratios)), int(np.argmax(ratios))) if not np.isnan(ratios).any() else (float("nan"), int(np.argmax(np.isnan(ratios))))
        self.fx_err, self.fx_bound = fx_err, fx_bound
        self.fx_ratio = fx_err / fx_bound

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
    """fx, g: what the evaluation returned (g in the engine's dtype).  Every one of the P elements is compared; nothing is exempt."""
    case = ref.case
    g = np.asarray(g)
    assert g.shape == (case.P,) and g.dtype == case.dtype, "the gradient in the engine's own dtype"
    err = np.abs(g.astype(LD) - ref.g).astype(np.float64)
    # a bound of zero: no addend and a zero parameter (a state that a site never takes) -- the element has to be exactly zero
    with np.errstate(divide="ignore", invalid="ignore"):
        ratios = np.where(ref.bound > 0, err / ref.bound, np.where(err == 0, 0.0, np.inf))
    checked = int(np.count_nonzero(ratios <= 1.0) + np.count_nonzero(~(ratios <= 1.0)))
    assert checked == case.P == len(ref.bound) and np.all(ref.bound >= 0)
    failing = np.flatnonzero(~(ratios <= 1.0))
    order = failing[np.argsort(-np.nan_to_num(ratios[failing], nan=np.inf))][:named]
    failures = [Failure(ref, e, g[e], ratios[e]) for e in order]
    return Audit(case, checked, ratios, failing, failures, abs(float(LD(fx) - ref.fx)), ref.fx_bound)


def assert_within_bounds(ref, fx, g):
    """what the GPU test asserts of a device evaluation -> Audit"""
    a = audit(ref, fx, g)
    print(a.summary())
    assert a.checked == ref.case.P
    assert a.ok, a.report()
    return a


# ----------------------------------------------------------------------------- emulation of the stages in the engine's type
def emulate(ref, order="sequential", fault=None):
    """The stage chain in the engine's type T with NumPy: logits (exact), the scan chunked as the plan says (lock step over the
    chunks), R, the bucket sums in `order` ("sequential": per bucket in sequence order; "blas": one matrix product in T), fold.
    fault: (name, ...) -- one of the negative controls, see FAULTS.  -> (fx, g)"""
    case, plan = ref.case, ref.plan
    N, L, q, halo, T = case.N, case.L, case.q, case.halo, case.dtype.type
    Lq = L * q
    X, x = ref.X, ref.x
    fname = fault[0] if fault else None
    W, h = expand(x, L, q)
    S64 = logit_sums(W, X, q)
    S = S64.astype(T)
    assert np.array_equal(S.astype(np.float64), S64)
    hT = h.astype(T)
    assert np.array_equal((S.reshape(N, L, q) + hT).astype(np.float64), S64.reshape(N, L, q) + h)
    wT = ref.w.astype(T)
    carry = case.mode != "exact"
    warm = 4 if fname == "warm_up_4" else plan["warm"]
    s_, e_, ws_ = chunk_starts(N, halo, plan["chunk"], warm, carry)
    Pm = np.zeros((N, L, q), dtype=T)
    p = np.zeros((len(s_), L, q), dtype=T)
    for t in range(int((e_ - ws_).max())):
        n = ws_ + t
        active = n < e_
        rows = np.minimum(n, N - 1)
        z = S[rows].reshape(-1, L, q) + hT
        if carry:
            z = z + p
        tt = np.exp(z - z.max(axis=2, keepdims=True))
        sm = np.zeros(tt.shape[:2], dtype=T)
        for a in range(q):
            sm = sm + tt[:, :, a]
        pn = tt * (T(1) / sm)[:, :, None]
        p = np.where(active[:, None, None], pn, p)
        keep = active & ((n >= s_) | (n < halo))
        Pm[rows[keep]] = pn[keep]
    assert Pm.dtype == T
    xi = X[:, :, None].astype(np.int64)
    px = np.take_along_axis(Pm, xi, axis=2)[:, :, 0]
    fterms = -(wT[halo:, None] * np.log(px[halo:])).astype(np.float64)
    R = wT[:, None, None] * Pm
    np.put_along_axis(R, xi, np.take_along_axis(R, xi, axis=2) - wT[:, None, None], axis=2)
    R = R.reshape(N, Lq)
    assert R.dtype == T
    oh = one_hot(X, q, halo)
    if order == "blas":
        G = oh.astype(T).T @ R
    else:
        G = np.zeros((Lq, Lq), dtype=T)
        for k in range(Lq):
            rows = np.flatnonzero(oh[:, k])
            if len(rows):
                G[k] = np.add.reduce(R[rows], axis=0)
    assert G.dtype == T

    # ---- negative controls on the sums
    if fname == "drop_tile_last_row":             # (site j, tile t): row 127 of the tile missing from the sum of its (site, state)
        _, j, t = fault
        n = halo + NC * t + NC - 1
        G[j * q + X[n, j]] -= R[n]
    elif fname == "drop_slab":                    # (strip, split): one slab of one strip not added
        _, strip, split = fault
        cw = 512 // case.dtype.itemsize
        cps = plan["scatChunksPerSplit"]
        lo, hi = halo + split * cps * NC, min(N, halo + (split + 1) * cps * NC)
        ohs = np.zeros_like(oh)
        ohs[lo:hi] = oh[lo:hi]
        G[:, strip * cw:(strip + 1) * cw] -= (ohs.astype(T).T @ R)[:, strip * cw:(strip + 1) * cw]
    elif fname == "padding_site":                 # odd L: the padding site's sums (state 0: every owned row) land on its partner's state 0
        assert L % 2 == 1
        G[(L - 1) * q + 0] += np.add.reduce(R[halo:], axis=0)
    elif fname == "swap_states":                  # (site j, b1, b2)
        _, j, b1, b2 = fault
        G[[j * q + b1, j * q + b2]] = G[[j * q + b2, j * q + b1]]
    elif fname == "halo_row":                     # row halo - 1 summed
        assert halo > 0
        n = halo - 1
        G[np.arange(L) * q + X[n]] += R[n]

    g = np.zeros(case.P, dtype=T)
    if order == "blas" or case.bits == 64:
        colsum = np.add.reduce(R[halo:], axis=0) if case.bits == 32 else np.sum(R[halo:].astype(LD), axis=0).astype(T)
    else:
        colsum = np.zeros(Lq, dtype=T)
        for b in range(q):                         # float32: the column sums of R are read off site 0's rows of G
            colsum = colsum + G[b]
    hg = (T(2) * T(LAMBDA_H) * x[:Lq] + colsum).reshape(L, q)
    if fname == "shift_field":                     # (site i): the field column of one site shifted by one state
        hg[fault[1]] = np.roll(hg[fault[1]], 1)
    g[:Lq] = hg.ravel()
    G4 = G.reshape(L, q, L, q)
    iu, ju = ref.iu, ref.ju
    v1 = G4.transpose(2, 0, 3, 1)[iu, ju]
    v2 = G4.transpose(0, 2, 1, 3)[iu, ju].copy()
    if fname == "transposed_block":                # (i, j): site j's conditional read from the transposed block
        pidx = (index_of(case, fault[1], fault[2], 0, 0) - Lq) // (q * q)
        v2[pidx] = v2[pidx].T
    gJ = (T(2) * T(LAMBDA_J) * x[Lq:].reshape(v1.shape) + v1) + v2
    assert gJ.dtype == T
    g[Lq:] = gJ.ravel()
    x64 = x.astype(np.float64)
    fx = math.fsum(fterms.ravel().tolist()) + LAMBDA_H * math.fsum((x64[:Lq] ** 2).tolist()) + LAMBDA_J * math.fsum((x64[Lq:] ** 2).tolist())
    return fx, g


FAULTS = ["drop_tile_last_row", "drop_slab", "padding_site", "swap_states", "transposed_block", "halo_row", "shift_field", "warm_up_4"]
