"""TEST INFRASTRUCTURE ONLY -- host reference for the arDCA epistasis entries (pydca_amd/csrc/ar_epistasis.hip and the scores
of scoring.hip on its output), with no GPU dependency: tests/test_ar_epistasis_audit.py feeds it what the device returned,
tests/test_ar_epistasis_audit_host.py pins it on the CPU.

reference(case, plan) evaluates, in np.longdouble and straight from the definition (no products, no table V), for the wild
type w with logits u_m(c) = h_m(c) + sum_{k<m} J_km(w_k, c) and dJ_km(a, .) = J_km(a, .) - J_km(w_k, .):

    eps_kl(a, b) = T - sum_{m>l} [ lse_c(u_m + dJ_km(a,.) + dJ_lm(b,.)) - lse_c(u_m + dJ_km(a,.)) - lse_c(u_m + dJ_lm(b,.)) + lse_c(u_m) ]
    T            = (J_kl(a, b) - J_kl(w_k, b)) - (J_kl(a, w_l) - J_kl(w_k, w_l))
    d_k(a)       = (u_k(a) - u_k(w_k)) + sum_{m>k} [ dJ_km(a, w_m) - (lse_c(u_m + dJ_km(a,.)) - lse_c(u_m)) ]

(u_m enters shifted by lse(u_m), so every lse is the logarithm of a number near 1 and the longdouble roundings stay small).
The rows a = w_k and the columns b = w_l are exact zeros.  The bracket is ln r_m of the kernel's header.

ELEMENT BOUNDS, from the device's rounding sequence as ar_epistasis.hip writes it (u = 2^-53, gamma(k) = k u / (1 - k u)).
Nothing the device returns enters them.  Every call of the device's exp or log is allowed 2 ulp: LIB = 4 u relative.

  * cond_m(c), the wild type's conditionals (ardca.hip's logits kernel, n = 1): the log-softmax of m + 1 terms, bounded as in
    tests/ardca_eval_reference.py: du = gamma(m) (|h| + sum |J|), delta = du + u (|u - max| + 2 max du),
    rho_Z = sum_c p delta + LIB + gamma(q - 1), dlz = rho_Z / (1 - rho_Z) + LIB |log Z|, econd(c) = delta(c) + dlz + u |cond(c)|.
    p_m(c) = exp(cond) is off by econd + LIB relative, sqrt p = exp(cond / 2) by econd / 2 + LIB.  With E_m = max_c econd_m(c):
    a relative perturbation of p_m moves ln r_m by at most 3 times it (the numerator and both normalisers).
  * U^k_m(a, c) = exp(fl(J - J_w)): the rounded difference moves the argument by u |arg|, the exponential adds LIB:
    eU_km(a) = u max_c |arg| + LIB, relative.
  * S_m(k, a): q fused multiply-adds of positive terms from 0, relative gamma(q); gamma(q + 1) here, which also covers the
    separate rounding of each product in the float64 restatement (NumPy has no fused multiply-add).
    eS_km(a) = E_m + LIB + eU_km(a) + gamma(q + 1).
  * V = fl(fl(U / S) sqrt p): two more roundings; r_m = sum_c V^k V^l, again gamma(q + 1).  Together
    rho_m(k, a; l, b) = 3 E_m + 4 LIB + 2 eU_km(a) + 2 eU_lm(b) + 3 gamma(q + 1) + 4 u     (relative error of r_m = error of ln r_m).
  * the running product: one rounding per joined step, gamma(L - 1 - l).  The split of the exponent is exact.
  * one logarithm of the mantissa product: LIB |log prod|, |log prod| <= ln 2 + sum of |ln r_m| over the steps after the tile's
    last split (the plan's mstart and steps say which); fl(esum ln 2) with the rounded constant: 2 u |esum ln 2|,
    |esum ln 2| <= |sum ln r| + |log prod|; their sum: u |sum ln r|.  A column that never joins (l = L - 1) has log(1.0) = 0:
    none of these.
  * T: three subtractions, u (|J(a,b) - J(w_k,b)| + |J(a,w_l) - J(w_k,w_l)| + |T|); the last subtraction u |eps|.

    eps_bound = sum_{m>l} rho_m + gamma(L - 1 - l) + [log terms] + [T terms] + u |eps| + 2^-58 sum of |lse terms| (the reference's own)

  d_k(a): (cond_k(a) - cond_k(w_k)) carries econd(a) + econd(w_k) + u |difference|; site m's term fl(fl(dJ) - log S) carries
  u |dJ| + eS_km(a) + LIB |log S| + u |term|; the L - 1 - k terms are added in ascending m, gamma(L - 1 - k) sum |term|; u |d|.

  log P(s) of a sequence (logp_reference, for the single mutants through dca_ar_log_probabilities): every site value carries
  delta(s_l) + dlz + u |cond|, the L values are added in one accumulator: gamma(L - 1) sum |site|.

  scores (fn_kernel of scoring.hip on the plm-layout float64 source, qm = q - 1): a centred element carries
  beta_e = gamma(qm^2 + 3) (|v| + row mean + column mean + mean, all of |v|); |FN - FN_ref| <= ||beta||_2 + gamma(ceil(qm^2 / 64) + 8) FN,
  plus 2 ||eps bounds of the block||_2 when the reference's eps is the source.  APC, absolute (it crosses zero): the site means are
  tree sums, gamma(ceil(L / 256) + 9) of their size plus the mean FN bound; the overall mean likewise; one quotient, one
  product, one difference.  At q = 2 the centred 1 x 1 block is exactly 0, every FN is 0 and the APC is 0 / 0: NaN by
  definition, and the device has to say so too.

The derivation is not the authority: tests/test_ar_epistasis_audit_host.py holds the bounds to the float64 restatement of the
kernel's order (restate(); it must stay inside on every element) and to planted faults (each must leave by 100 bounds).

audit() checks ALL elements of eps and d and names what fails by (k, l, a, b), the tile that writes it, the tile's step count
and the steps the element's column joins."""
import os
import subprocess

import numpy as np

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
ETA = float(np.finfo(np.float64).tiny)
LIB = 4 * U                               # 2 ulp of a device exp / log
UP = 1 + 2.0 ** -10                       # second-order terms and the float64 roundings of the bound itself
OWN = 2.0 ** -58                          # the reference's own longdouble roundings, relative to its sum of |terms|
LN2 = 0.69314718055994530942
SCALES = (0.5, 2.0)
PLANT = 140.0                             # exp(-140) = 2^-202


def gamma(k):
    return k * U / (1.0 - k * U)


def pair_index(L, k, l):
    return L * (L - 1) // 2 - (L - k) * (L - k - 1) // 2 + (l - k - 1)


# ----------------------------------------------------------------------------- the case table
class Case:
    """One row of the table at one coupling scale.  facts: what ar_epistasis_plan.h makes of the shape (plan_of).  planted:
    {m: D} -- J_0m(1, 0) = J_0m(0, 0) + D and J_1m(1, 1) = J_1m(0, 1) + D, wild type all 0: r_m of (k, l, a, b) = (0, 1, 1, 1)
    is about exp(-D)."""

    def __init__(self, q, L, scale, reaches, facts, planted=None, tag=""):
        self.q, self.L, self.scale, self.reaches, self.facts, self.planted = q, L, scale, reaches, facts, planted
        self.pairs = L * (L - 1) // 2
        self.P = L * q + self.pairs * q * q
        self.name = "q%d_L%d_s%g%s" % (q, L, scale, tag)

    def __repr__(self):
        return self.name


# facts: QM, NPRE, lds (bytes); grid: (row tiles, column tiles) of L q; launched; steps: of every launched tile in launch order;
# mid: launched tiles whose first column is not state 0 of its site; rows / cols: the distinct numbers of live rows / columns
SHAPES = [
    (5, 13, "L q = 65: the second column tile holds one live column and starts mid-site (C0 = 64: site 12, state 4); one ragged row tile",
     dict(QM=8, NPRE=3, lds=15360, grid=(1, 2), launched=2, steps=[12, 0], mid=1, rows=[65], cols=[1, 64])),
    (5, 26, "L q = 130: three column tiles, two start mid-site; the second row tile (2 rows of the last site) is never launched: "
            "3 of 6 tiles skipped; steps 25, 13, 0",
     dict(QM=8, grid=(2, 3), launched=3, skipped=3, steps=[25, 13, 0], mid=2, rows=[128], cols=[2, 64])),
    (5, 27, "one more site: the second row tile is launched with 7 live rows; step counts 1 and 2 mod 4",
     dict(grid=(2, 3), launched=4, steps=[26, 14, 1, 1], mid=3, rows=[7, 128], cols=[7, 64], residues=[1, 2])),
    (2, 65, "smallest alphabet, q q = 4; 64 steps: 16 splits", dict(QM=8, lds=6144, grid=(2, 3), launched=3, steps=[64, 32, 0], mid=0, splits=16)),
    (8, 16, "q = QM = 8; L q = 128: no ragged row or column anywhere",
     dict(QM=8, NPRE=3, grid=(1, 2), launched=2, steps=[15, 7], mid=0, rows=[128], cols=[64])),
    (8, 17, "one site more: ragged by 8", dict(QM=8, grid=(2, 3), launched=3, steps=[16, 8, 0], rows=[128], cols=[8, 64])),
    (9, 15, "the first q of QM = 24, NPRE = 9; mid-site starts", dict(QM=24, NPRE=9, lds=27648, launched=3, steps=[14, 7, 0], mid=2, cols=[7, 64])),
    (21, 13, "L q = 273: 3 x 5 tiles, 8 launched; every residue of steps mod 4",
     dict(QM=24, NPRE=9, lds=64512, grid=(3, 5), launched=8, steps=[12, 9, 6, 6, 3, 3, 0, 0], mid=7, residues=[0, 1, 2, 3])),
    (24, 11, "q = QM = 24; 3 x 5 tiles", dict(QM=24, NPRE=9, lds=73728, grid=(3, 5), launched=8, steps=[10, 8, 5, 5, 2, 2, 0, 0], mid=5)),
    (25, 6, "the first q of QM = 32, NPRE = 12", dict(QM=32, NPRE=12, lds=76800, grid=(2, 3), launched=3, steps=[5, 3, 0], mid=2)),
    (32, 9, "q = QM = 32; LDS 98 304 bytes > 64 KiB: hipFuncSetAttribute has to take effect; 3 x 5 tiles",
     dict(QM=32, NPRE=12, lds=98304, grid=(3, 5), launched=8, steps=[8, 6, 4, 4, 2, 2, 0, 0], mid=0, rows=[128], cols=[32, 64])),
    (32, 4, "L q = 128 at the largest alphabet; tiles of 3 and 1 steps: never a split",
     dict(QM=32, lds=98304, grid=(1, 2), launched=2, steps=[3, 1], splits=0, rows=[128], cols=[64])),
    (21, 2, "one pair: the tile streams site 1, which its column never joins (m > l fails): eps = T",
     dict(QM=24, grid=(1, 1), launched=1, steps=[1], joined=0, rows=[42], cols=[42])),
]
RANGE_FACTS = dict(QM=8, grid=(1, 1), launched=1, steps=[11], splits=2, joined=10)
CASES = [Case(q, L, s, reaches, facts) for (q, L, reaches, facts) in SHAPES for s in SCALES]
RANGE = Case(2, 12, 0.5, "range: r_m of (0, 1, 1, 1) is about 2^-200 at each of 10 later sites; a float64 product without the split underflows",
             RANGE_FACTS, planted={m: PLANT for m in range(2, 12)}, tag="_planted")
# beyond the header's contract (the run of sites 2 .. 5 spans 2^-1190) and therefore no device case: the splits counted from
# mstart = 1 see sites {2, 3, 4}, {5 .. 8}, {9, 10, 11} and stay in range, counted from l + 1 = 2 they see {2 .. 5} and underflow
OFF_CONTRACT = Case(2, 12, 0.5, "split alignment made observable", RANGE_FACTS,
                    planted={m: (229.0 if m <= 4 else PLANT) for m in range(2, 12)}, tag="_offcontract")
CASES.append(RANGE)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ----------------------------------------------------------------------------- the product kernel's geometry
def compile_plan_driver(directory):
    """tests/ar_epistasis_plan_driver.cpp compiled with the host compiler -> driver(L, q) = dict(QM, NPRE, lds, the constants,
    tiles = [dict(rt, ct, mstart, steps, mid, rows, cols)] in launch order)"""
    exe = os.path.join(str(directory), "ar_epistasis_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "ar_epistasis_plan_driver.cpp")])
    cache = {}

    def driver(L, q):
        if (L, q) not in cache:
            lines = [[int(t) for t in ln.split()] for ln in subprocess.check_output([exe, str(L), str(q)]).decode().splitlines()]
            head = lines[0]
            assert len(head) == 12 and head[:2] == [L, q] and head[11] == len(lines) - 1
            p = dict(zip(["QM", "NPRE", "lds", "threads", "rowsPerThread", "colsPerThread", "tileR", "tileC", "rescale"], head[2:11]))
            p["tiles"] = [dict(zip(["rt", "ct", "mstart", "steps", "mid", "rows", "cols"], t)) for t in lines[1:]]
            cache[(L, q)] = p
        p = cache[(L, q)]
        return dict(p, tiles=[dict(t) for t in p["tiles"]])

    return driver


def plan_of(case, driver):
    """ar_epistasis_plan.h's numbers for the case's shape and what the case table says of them"""
    p = driver(case.L, case.q)
    L, q, Lq = case.L, case.q, case.L * case.q
    p["grid"] = (-(-Lq // p["tileR"]), -(-Lq // p["tileC"]))
    p["launched"] = len(p["tiles"])
    p["skipped"] = p["grid"][0] * p["grid"][1] - p["launched"]
    p["steps"] = [t["steps"] for t in p["tiles"]]
    p["residues"] = sorted({s % p["rescale"] for s in p["steps"]})
    p["splits"] = max(p["steps"]) // p["rescale"]
    p["mid"] = sum(t["mid"] for t in p["tiles"])
    p["rows"] = sorted({t["rows"] for t in p["tiles"]})
    p["cols"] = sorted({t["cols"] for t in p["tiles"]})
    # the most steps any written element's column joins: L - 1 - (the first site of a tile that holds a pair)
    p["joined"] = max(L - 1 - max(t["ct"] * p["tileC"] // q, 1) for t in p["tiles"])
    return p


def tile_of(plan, R, C):
    """the launched tile that writes element (R, C) of the flattened table"""
    for t in plan["tiles"]:
        if t["rt"] == R // plan["tileR"] and t["ct"] == C // plan["tileC"]:
            return t
    return None


# ----------------------------------------------------------------------------- inputs
def wildtype(case):
    """uint8 [L]: random, state 0 at site 0 and state q - 1 at site L - 1 (and the other way round next to them)"""
    if case.planted:
        return np.zeros(case.L, dtype=np.uint8)
    w = np.random.default_rng(5200 + 100 * case.q + case.L).integers(0, case.q, size=case.L).astype(np.uint8)
    w[0], w[-1] = 0, case.q - 1
    if case.L >= 4:
        w[1], w[-2] = case.q - 1, 0
    return w


def model(case):
    """packed x (fields, then the pair blocks in pair order): normal, standard deviation case.scale; the planted entries on top"""
    L, q = case.L, case.q
    x = np.random.default_rng(6200 + 100 * q + L + int(10 * case.scale)).normal(0.0, case.scale, case.P)
    if case.planted:
        Jb = x[L * q:].reshape(case.pairs, q, q)
        for m, D in case.planted.items():
            Jb[pair_index(L, 0, m), 1, 0] = Jb[pair_index(L, 0, m), 0, 0] + D
            Jb[pair_index(L, 1, m), 1, 1] = Jb[pair_index(L, 1, m), 0, 1] + D
    return x


def unpack(x, L, q):
    """-> h [L, q], J [L, L, q, q] (the block of k < l at [k, l], zero elsewhere), float64"""
    h = x[:L * q].reshape(L, q)
    J = np.zeros((L, L, q, q))
    iu, ju = np.triu_indices(L, 1)
    J[iu, ju] = x[L * q:].reshape(len(iu), q, q)
    return h, J


def blocks(M, L, q):
    """[L q, L q] -> [pairs, a, b] = M[(k, a)][(l, b)], k < l in pair order"""
    iu, ju = np.triu_indices(L, 1)
    return np.ascontiguousarray(M.reshape(L, q, L, q).transpose(0, 2, 1, 3)[iu, ju])


def lse(A):
    """log sum exp over the last axis, in A's type"""
    mx = A.max(axis=-1)
    return mx + np.log(np.exp(A - mx[..., None]).sum(axis=-1))


# ----------------------------------------------------------------------------- conditionals and log P in longdouble
def conditionals(x, L, q, X):
    """X: codes [n, L] -> cond (longdouble [n, L, q]), econd (float64 [n, L, q]: the bound of the device's conditional
    fl(fl(u - max) - log Z))"""
    h, J = unpack(x, L, q)
    X = np.asarray(X, dtype=np.int64)
    n = X.shape[0]
    Ux = np.zeros((n, L, q), dtype=LD)
    Uabs = np.zeros((n, L, q))
    for l in range(L):
        Ux[:, l] = h[l].astype(LD)
        Uabs[:, l] = np.abs(h[l])
        if l:
            T = J[np.arange(l)[None, :], l, X[:, :l]]                                            # [n, l, q]
            Ux[:, l] += T.astype(LD).sum(axis=1)
            Uabs[:, l] += np.abs(T).sum(axis=1)
    d = Ux - Ux.max(axis=2, keepdims=True)
    lz = np.log(np.exp(d).sum(axis=2))
    c = d - lz[:, :, None]
    du = gamma(np.arange(L))[None, :, None] * Uabs * UP
    delta = du + U * (np.abs(d).astype(np.float64) + 2 * du.max(axis=2, keepdims=True)) * UP
    rho_z = (np.exp(c).astype(np.float64) * delta).sum(axis=2) * UP + LIB + gamma(q - 1) + q * ETA
    dlz = rho_z / (1 - rho_z) + LIB * np.abs(lz).astype(np.float64) * UP
    econd = delta + dlz[:, :, None] + U * np.abs(c).astype(np.float64) * UP
    return c, econd


def logp_reference(x, L, q, X):
    """log P of the codes X [n, L] -> (longdouble [n], bound float64 [n]) of dca_ar_log_probabilities"""
    X = np.asarray(X, dtype=np.int64)
    c, econd = conditionals(x, L, q, X)
    site = np.take_along_axis(c, X[:, :, None], axis=2)[:, :, 0]
    esite = np.take_along_axis(econd, X[:, :, None], axis=2)[:, :, 0]
    A = np.abs(site).astype(np.float64).sum(axis=1) * UP
    return site.sum(axis=1), (esite.sum(axis=1) + gamma(L - 1) * A + OWN * A) * UP


def single_mutants(w, L, q):
    """uint8 [L q + 1, L]: row k q + a is w with site k set to a; the last row is w"""
    rows = np.repeat(np.asarray(w, dtype=np.uint8)[None, :], L * q + 1, axis=0)
    idx = np.arange(L * q)
    rows[idx, idx // q] = idx % q
    return rows


# ----------------------------------------------------------------------------- the reference
class Reference:
    pass


def reference(case, plan):
    """-> Reference: eps (longdouble [pairs, q, q]), eps_bound (float64, 0 on the wild-type rows and columns), d (longdouble
    [L, q]), d_bound, ln_r_abs / ln_r_sum (per element: sum of |ln r_m| and of ln r_m), window (the largest |sum of ln r_m| over
    4 consecutive joined sites, per element) and the inputs"""
    L, q, Lq = case.L, case.q, case.L * case.q
    x, w = model(case), wildtype(case)
    wi = w.astype(np.int64)
    h, J = unpack(x, L, q)
    c, econd = conditionals(x, L, q, wi[None, :])
    c, econd = c[0], econd[0]                                                                    # [L, q]
    E = econd.max(axis=1)
    g1 = gamma(q + 1)

    dJ = J.astype(LD) - J[np.arange(L), :, wi][:, :, None, :].astype(LD)                          # [k, m, a, c]
    eU = U * np.abs(dJ).astype(np.float64).max(axis=3) * UP + LIB                                # [k, m, a]
    lnS = np.zeros((L, L, q), dtype=LD)                                                          # [k, m, a], k < m
    for m in range(1, L):
        lnS[:m, m] = lse(c[m][None, None, :] + dJ[:m, m])

    # which steps lie after a column tile's last split
    col_tile = np.arange(Lq) // plan["tileC"]
    tail_from = np.full(Lq, L, dtype=np.int64)
    for t in plan["tiles"]:
        tail_from[col_tile == t["ct"]] = t["mstart"] + t["steps"] // plan["rescale"] * plan["rescale"]
    site_of = np.arange(Lq) // q

    lsum = np.zeros((Lq, Lq), dtype=LD)
    labs, ltail, rho, own = (np.zeros((Lq, Lq)) for _ in range(4))
    series = []                                                                                  # (m, ln r_m [m q, m q]) for the windows
    for m in range(2, L):
        M = m * q
        A = c[m][None, :] + dJ[:m, m].reshape(M, q)
        ls = lnS[:m, m].reshape(M)
        lr = lse(A[:, None, :] + dJ[:m, m].reshape(M, q)[None, :, :]) - ls[:, None] - ls[None, :]
        joins = (site_of[:M] < m)[None, :] & (site_of[:M][:, None] < site_of[:M][None, :])       # k < l < m
        lr = np.where(joins, lr, LD(0))
        lr64 = np.abs(lr).astype(np.float64)
        lsum[:M, :M] += lr
        labs[:M, :M] += lr64
        ltail[:M, :M] += np.where((m >= tail_from[:M])[None, :], lr64, 0.0)
        e = eU[:m, m].reshape(M)
        rho[:M, :M] += np.where(joins, 3 * E[m] + 4 * LIB + 3 * g1 + 4 * U + 2 * e[:, None] + 2 * e[None, :], 0.0)
        own[:M, :M] += np.where(joins, lr64 + np.abs(ls).astype(np.float64)[:, None] + np.abs(ls).astype(np.float64)[None, :], 0.0)
        series.append(lr)

    JJ = J.transpose(0, 2, 1, 3).reshape(Lq, Lq).astype(LD)
    rowW, colW = site_of * q + wi[site_of], site_of * q + wi[site_of]
    d1, d2 = JJ - JJ[rowW, :], JJ[:, colW] - JJ[rowW][:, colW]
    T = d1 - d2
    eps = T - lsum
    nj = (L - 1 - site_of)[None, :].astype(np.float64)
    ls64 = np.abs(lsum).astype(np.float64)
    logs = np.where(nj > 0, LIB * (LN2 + ltail) + 2 * U * (ls64 + LN2 + ltail) + U * ls64, 0.0)
    tabs = np.abs(d1).astype(np.float64) + np.abs(d2).astype(np.float64) + np.abs(T).astype(np.float64)
    bound = ((rho + gamma(nj)) * UP + logs + U * tabs + U * np.abs(eps).astype(np.float64) + OWN * (own + tabs)) * UP
    wt = (np.arange(Lq) == rowW)
    zero = wt[:, None] | wt[None, :]
    eps = np.where(zero, LD(0), eps)
    bound = np.where(zero, 0.0, bound)

    # d_k(a)
    wm = wi[None, :, None, None]
    dJw = np.take_along_axis(dJ, np.broadcast_to(wm, (L, L, q, 1)), axis=3)[:, :, :, 0]         # dJ_km(a, w_m)
    later = (np.arange(L)[:, None] < np.arange(L)[None, :])[:, :, None]
    term = np.where(later, dJw - lnS, LD(0))
    cdiff = c - c[np.arange(L), wi][:, None]
    d = cdiff + term.sum(axis=1)
    eS = E[None, :, None] + LIB + eU + g1
    lnS64, term64 = np.abs(lnS).astype(np.float64), np.abs(term).astype(np.float64)
    eterm = np.where(later, U * np.abs(dJw).astype(np.float64) + eS * UP + LIB * lnS64 + U * term64, 0.0).sum(axis=1)
    A = term64.sum(axis=1)
    nd = (L - 1 - np.arange(L))[:, None].astype(np.float64)
    d_bound = (econd + econd[np.arange(L), wi][:, None] + U * np.abs(cdiff).astype(np.float64) + eterm * UP + gamma(nd) * A
               + U * np.abs(d).astype(np.float64) + OWN * (A + lnS64.sum(axis=1) + np.abs(c).astype(np.float64))) * UP
    wt2 = np.arange(q)[None, :] == wi[:, None]
    d = np.where(wt2, LD(0), d)
    d_bound = np.where(wt2, 0.0, d_bound)

    # the kernel's contract: the largest |sum of ln r_m| over 4 consecutive sites, per element
    window = np.zeros((Lq, Lq))
    for i in range(len(series)):
        acc = np.zeros((Lq, Lq), dtype=LD)
        for lr in series[i:i + 4]:
            acc[:lr.shape[0], :lr.shape[1]] += lr
        window = np.maximum(window, np.abs(acc).astype(np.float64))

    ref = Reference()
    ref.case, ref.plan, ref.x, ref.w = case, plan, x, w
    ref.eps, ref.eps_bound = blocks(eps, L, q), blocks(bound, L, q)
    ref.d, ref.d_bound = d, d_bound
    ref.zero, ref.d_zero, ref.term = blocks(zero, L, q), wt2, term          # the exact zeros; site m's term of d_k(a) at [k, m, a]
    ref.ln_r_abs, ref.ln_r_sum, ref.window = blocks(labs, L, q), blocks(lsum.astype(np.float64), L, q), blocks(window, L, q)
    ref.iu, ref.ju = np.triu_indices(L, 1)
    return ref


# ----------------------------------------------------------------------------- the kernel's order in float64
def restate(x, L, q, w, plan, fault=None):
    """ar_epistasis.hip with NumPy in float64 -> (eps [pairs, q, q], d [L, q]): p = exp(cond) and sqrt p = exp(cond / 2); U;
    S over ascending c; V = (U / S) sqrt p; r over ascending c; per launched tile the product over ascending m with the
    exponent split at the steps t = 3 (mod 4) counted from the tile's mstart; one logarithm.  (The fused multiply-adds of S and
    r round their products here: the bound allows for it.)
    fault: None or a tuple naming a planted fault of the order --
      ("drop", C, m)          site m left out of column C's product
      ("join_ge", C)          column C joins at m >= l
      ("esum", R, C, n)       the n-th split of element (R, C) adds one to the exponent
      ("count_from_l",)       the splits counted from l + 1, per column, instead of from mstart
      ("skip_tile", rt, ct)   tile (rt, ct) not written
      ("b_offset", ct)        column tile ct reads its second run from row offset C0 instead of C0 q
      ("keep_wt_rows",)       the rows a = w_k not zeroed"""
    Lq, qq = L * q, q * q
    kind = fault[0] if fault else None
    h, J = unpack(np.asarray(x, dtype=np.float64), L, q)
    wi = np.asarray(w, dtype=np.int64)
    cond = np.zeros((L, q))
    for l in range(L):
        u = h[l].copy()
        for k in range(l):
            u = u + J[k, l, wi[k]]
        mx = u.max()
        z = 0.0
        for b in range(q):
            z = z + np.exp(u[b] - mx)
        cond[l] = (u - mx) - np.log(z)
    p, sp = np.exp(cond), np.exp(0.5 * cond)
    V = [None] * L                                        # V[m]: [m q, q] flattened like the device table of site m
    term = np.zeros((L, L, q))                            # [k, m, a]
    for m in range(1, L):
        Um = np.exp(J[:m, m] - J[np.arange(m), m, wi[:m]][:, None, :])                           # [k, a, c]
        S = np.zeros((m, q))
        for cc in range(q):
            S = S + p[m, cc] * Um[:, :, cc]
        term[:m, m] = (J[:m, m, :, wi[m]] - J[np.arange(m), m, wi[:m], wi[m]][:, None]) - np.log(S)
        V[m] = ((Um / S[:, :, None]) * sp[m][None, None, :]).reshape(m * qq)
    d = np.zeros((L, q))
    for k in range(L):
        s = np.zeros(q)
        for m in range(k + 1, L):
            s = s + term[k, m]
        d[k] = (cond[k] - cond[k, wi[k]]) + s
        d[k, wi[k]] = 0.0

    site_of = np.arange(Lq) // q
    wcode = site_of * q + wi[site_of]
    JJ = J.transpose(0, 2, 1, 3).reshape(Lq, Lq)
    T = (JJ - JJ[wcode, :]) - (JJ[:, wcode] - JJ[wcode][:, wcode])
    out = np.zeros((Lq, Lq))
    TR, TC, RS = plan["tileR"], plan["tileC"], plan["rescale"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for t in plan["tiles"]:
            if kind == "skip_tile" and (t["rt"], t["ct"]) == fault[1:]:
                continue
            R0, C0 = t["rt"] * TR, t["ct"] * TC
            rows, cols = np.arange(R0, min(R0 + TR, Lq)), np.arange(C0, min(C0 + TC, Lq))
            lcol = site_of[cols]
            prod = np.ones((len(rows), len(cols)))
            esum = np.zeros(prod.shape, dtype=np.int64)
            nsplit = 0
            b0 = C0 if (kind == "b_offset" and t["ct"] == fault[1]) else C0 * q
            for step in range(t["steps"]):
                m = t["mstart"] + step
                flat, lim = V[m], m * qq
                ga = (rows * q)[:, None] + np.arange(q)[None, :]
                gb = b0 + (np.arange(len(cols)) * q)[:, None] + np.arange(q)[None, :]
                A = np.where(ga < lim, flat[np.minimum(ga, lim - 1)], 0.0)
                B = np.where(gb < lim, flat[np.minimum(gb, lim - 1)], 0.0)
                r = np.zeros(prod.shape)
                for cc in range(q):
                    r = r + A[:, cc][:, None] * B[:, cc][None, :]
                join = m > lcol
                if kind == "join_ge":
                    join = join | ((cols == fault[1]) & (m >= lcol))
                if kind == "drop" and m == fault[2]:
                    join = join & (cols != fault[1])
                prod[:, join] = prod[:, join] * r[:, join]
                if kind == "count_from_l":
                    split = (m - (lcol + 1) >= 0) & ((m - (lcol + 1)) % RS == RS - 1)
                else:
                    split = np.full(len(cols), step % RS == RS - 1)
                if split.any():
                    mant, ex = np.frexp(prod[:, split])
                    esum[:, split] += ex - 1
                    prod[:, split] = mant * 2.0
                    if kind == "esum" and nsplit == fault[3] and R0 <= fault[1] < R0 + len(rows) and C0 <= fault[2] < C0 + len(cols):
                        esum[fault[1] - R0, fault[2] - C0] += 1
                    nsplit += 1
            v = T[np.ix_(rows, cols)] - (np.log(prod) + esum.astype(np.float64) * LN2)
            zero = (cols == wcode[cols])[None, :] | np.zeros((len(rows), 1), dtype=bool)
            if kind != "keep_wt_rows":
                zero = zero | (rows == wcode[rows])[:, None]
            v = np.where(zero, 0.0, v)
            pairmask = site_of[rows][:, None] < lcol[None, :]
            out[np.ix_(rows, cols)] = np.where(pairmask, v, 0.0)
    return blocks(out, L, q), d


# ----------------------------------------------------------------------------- the audit
class Failure:
    def __init__(self, ref, what, index, dev, ratio):
        case, plan = ref.case, ref.plan
        self.what, self.index, self.ratio, self.dev = what, tuple(int(i) for i in index), float(ratio), float(dev)
        if what == "eps":
            pr, self.a, self.b = self.index
            self.k, self.l = int(ref.iu[pr]), int(ref.ju[pr])
            self.ref, self.bound = float(ref.eps[self.index]), float(ref.eps_bound[self.index])
            t = tile_of(plan, self.k * case.q + self.a, self.l * case.q + self.b)
            self.tile, self.steps, self.mstart = (t["rt"], t["ct"]), t["steps"], t["mstart"]
            self.joined = case.L - 1 - self.l
        else:
            self.k, self.a = self.index
            self.l = self.b = self.tile = None
            self.ref, self.bound = float(ref.d[self.index]), float(ref.d_bound[self.index])
            self.joined = case.L - 1 - self.k

    def __repr__(self):
        head = "%s: device %.17g, reference %.17g, off by %.3e = %.3g x bound %.3e" % (
            self.what, self.dev, self.ref, abs(self.dev - self.ref), self.ratio, self.bound)
        if self.what == "eps":
            return "%s; (k, l, a, b) = (%d, %d, %d, %d), tile (row %d, column %d) of %d steps from site %d, %d joined" % (
                head, self.k, self.l, self.a, self.b, self.tile[0], self.tile[1], self.steps, self.mstart, self.joined)
        return "%s; (k, a) = (%d, %d), %d later sites" % (head, self.k, self.a, self.joined)


def ratios_of(dev, ref, bound):
    """|dev - ref| / bound per element; where the bound is 0 (an exact zero): 0 for the same value, inf otherwise"""
    dev = np.asarray(dev)
    assert dev.dtype == np.float64 and dev.shape == ref.shape
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


class Audit:
    """checked: elements compared (all of eps and of d); worst / worst_d: the largest |error| / bound; failures: the worst
    elements out of bound, by name"""

    def __init__(self, ref, r_eps, r_d, named):
        self.case, self.r_eps, self.r_d = ref.case, r_eps, r_d
        self.checked = int(r_eps.size + r_d.size)
        self.worst = float(r_eps.max()) if r_eps.size else 0.0
        self.worst_d = float(r_d.max())
        self.failing = np.argwhere(~(r_eps <= 1.0))
        self.failing_d = np.argwhere(~(r_d <= 1.0))
        self.failures = []
        self._ref, self._named = ref, named

    def name(self, eps, d):
        order = np.argsort(-self.r_eps[tuple(self.failing.T)], kind="stable")[:self._named]
        self.failures = [Failure(self._ref, "eps", self.failing[i], eps[tuple(self.failing[i])], self.r_eps[tuple(self.failing[i])]) for i in order]
        order = np.argsort(-self.r_d[tuple(self.failing_d.T)], kind="stable")[:self._named]
        self.failures += [Failure(self._ref, "d", self.failing_d[i], d[tuple(self.failing_d[i])], self.r_d[tuple(self.failing_d[i])]) for i in order]
        return self

    @property
    def ok(self):
        return len(self.failing) == 0 and len(self.failing_d) == 0

    def summary(self):
        return "%s: %d elements checked, worst |error| / bound: eps %.4f, d %.4f; out of bound: eps %d, d %d" % (
            self.case.name, self.checked, self.worst, self.worst_d, len(self.failing), len(self.failing_d))

    def report(self):
        return "\n".join([self.summary()] + [repr(f) for f in self.failures])


def audit(ref, eps, d, named=12):
    """eps [pairs, q, q], d [L, q]: what the entry returned.  Every element is compared; nothing is exempt."""
    return Audit(ref, ratios_of(eps, ref.eps, ref.eps_bound), ratios_of(d, ref.d, ref.d_bound), named).name(np.asarray(eps), np.asarray(d))


def assert_within_bounds(ref, eps, d):
    """what the GPU test asserts of a device result -> the audit"""
    a = audit(ref, eps, d)
    print(a.summary())
    assert a.checked == ref.case.pairs * ref.case.q ** 2 + ref.case.L * ref.case.q
    assert a.ok, a.report()
    return a


# ----------------------------------------------------------------------------- the scores
def fn_reference(eps, q, eps_bound=None):
    """FN of pair blocks (the last state's row and column dropped, double-centred, Frobenius norm) in longdouble ->
    (fn [pairs], bound float64 [pairs]) of fn_kernel on this source; eps_bound: the source is a reference the device's own
    table may differ from by this much per element"""
    qm = q - 1
    blk = np.asarray(eps)[:, :qm, :qm].astype(LD)
    cen = blk - blk.mean(axis=1, keepdims=True) - blk.mean(axis=2, keepdims=True) + blk.mean(axis=(1, 2), keepdims=True)
    fn = np.sqrt((cen * cen).sum(axis=(1, 2)))
    ab = np.abs(blk).astype(np.float64)
    beta = gamma(qm * qm + 3) * (ab + ab.mean(axis=1, keepdims=True) + ab.mean(axis=2, keepdims=True) + ab.mean(axis=(1, 2), keepdims=True))
    bound = np.sqrt((beta * beta).sum(axis=(1, 2))) + gamma(-(-qm * qm // 64) + 8) * fn.astype(np.float64)
    if eps_bound is not None:
        bound = bound + 2 * np.sqrt((eps_bound[:, :qm, :qm] ** 2).sum(axis=(1, 2)))
    return fn, bound * UP


def apc_reference(fn, fn_bound, L):
    """the average-product correction of FN (longdouble) and its absolute bound; NaN where the mean FN is 0"""
    iu, ju = np.triu_indices(L, 1)
    M, B = np.zeros((L, L), dtype=LD), np.zeros((L, L))
    M[iu, ju], B[iu, ju] = fn, fn_bound
    M, B = M + M.T, B + B.T
    with np.errstate(divide="ignore", invalid="ignore"):
        av = M.sum(axis=1) / (L - 1)
        allm = av.mean()
        corr = av[iu] * (av[ju] / allm)
        g = gamma(-(-L // 256) + 9)
        av64 = av.astype(np.float64)
        eav = B.sum(axis=1) / (L - 1) + g * av64
        eall = eav.mean() + g * float(allm)
        rel = eav[iu] / av64[iu] + eav[ju] / av64[ju] + eall / float(allm) + 2 * U
        c64 = corr.astype(np.float64)
        bound = (fn_bound + c64 * rel * UP + U * (fn.astype(np.float64) + c64)) * UP
    return fn - corr, bound


def score_ratios(dev, ref, bound):
    """|dev - ref| / bound per pair; a NaN of the reference (0 / 0) has to be a NaN of the device"""
    dev = np.asarray(dev, dtype=np.float64)
    nan = np.isnan(ref.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(dev.astype(LD) - ref).astype(np.float64)
        r = np.where(err == 0, 0.0, err / bound)                  # a block of exact zeros has FN = 0 and a bound of 0
    r = np.where(nan, np.where(np.isnan(dev), 0.0, np.inf), r)
    return np.where(np.isnan(r), np.inf, r)
