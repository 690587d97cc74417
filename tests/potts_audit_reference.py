"""TEST INFRASTRUCTURE ONLY -- the element audit of the fitted Potts model as a sequence model (energy.hip, pll.hip, sample.hip,
ais.hip, boltzmann.hip) at every alphabet size and launch geometry, with no GPU dependency: tests/test_potts_audit.py feeds it
what the device returned, tests/test_potts_audit_host.py pins it on the CPU.

CASES is the table: each case names what it reaches, and `facts` are those claims as numbers of pydca_amd/csrc/potts_plan.h, read
through tests/potts_plan_driver.cpp (compile_plan_driver / plan_of); the host test asserts them and their union.

MODELS.  plm cases: x = N(0, sigma) rounded to the case's element type (sigma 0.5 for the sampler, AIS and bmDCA, 0.7 for
energies and PLL), set with plm_set_x and read back, so that the reference sees the stored values.  mf cases: the device's
mf_couplings() / mf_fields() on an alignment of tests/mf_shape_cases.py (on the CPU: the oracle's float64 model of the same
alignment); the inverse is audited elsewhere, here the model is an input.

REFERENCES are formed in np.longdouble from the stored values (widening is exact); energies with fsum_ld; the site sums u(a) by
longdouble adds in ascending j, whose own error, below L 2^-64 sum|terms|, enters the bound as OWN = 2^-58 sum|terms|.  The chains
come from the float64 restatements the suite already has (imported below, not restated).  Nothing the device returns enters a
reference or a bound.

BOUNDS (u = 2^-53, gamma(k) = k u / (1 - k u)):
  * energies: every term is widened exactly and added in double in some order: k = L + L (L - 1) / 2 terms and G slabs,
        |E - E_ref| <= gamma(k + G) sum|terms|.
  * mutation scan: dE(i, w_i) == 0.0 exactly; otherwise two sums of L - 1 terms, two differences and one add,
        gamma(L + 3) (|h_i(a)| + |h_i(w_i)| + sum_j |J(a, w_j)| + sum_j |J(w_i, w_j)|).
  * site conditionals, as ardca_eval_reference.py bounds the same body: u^(a) is off by du(a) = gamma(L) Uabs(a),
    Uabs = |h| + sum_j |J|.  cond is the same for any shift m, so it is read with the device's m^: d^(a) = fl(u^(a) - m^) is off by
    delta(a) = du(a) + u (|u(a) - max u| + max_b du(b)).  Z^ = sum_b exp^(d^(b)) ascending: rho_Z = sum_b p_b delta(b) + eps_exp
    + gamma(q - 1);  lz^ = log^(Z^): dlz = rho_Z / (1 - rho_Z) + eps_log (|lz| + max_b du(b));  cond^(a) = fl(d^(a) - lz^):
        |cond^(a) - cond(a)| <= delta(a) + dlz + u |cond(a)| + OWN (Uabs(a) + 1 + |cond(a)|).
    eps_exp = EXP_FACTOR x (numpy's largest exp error in ulps against longdouble over the case's own arguments, at least 1/2)
    x 2 u; eps_log likewise.  site == cond[s_i] and PLL == the ascending-i sum of site are asserted as bit equalities.
  * sampler, AIS chains, bmDCA chains: exact equality of the codes, under the margin condition
        |cum - r| / T >= 10 eps_draw  for every draw,   eps_draw = (q + 2) (beta gamma(L + 3) Sabs + eps_exp),
    Sabs = max_i (max_a |h_i(a)| + sum_j max_ab |J_ij(a, b)|) (an upper bound of every draw's sum|terms|; for AIS the base fields
    join it and beta is 1).  A property of inputs and restatement alone; a seed that violates it is changed, never the factor.  (q25_L513_mf has its model on the device only: the
    GPU test asserts the condition there, on the model it read back, as it does for every mf case.)
  * AIS log weights: per step fl(dbeta fl(E^ - E0^)) added to the running sum:
        sum_k |dbeta_k| (bound_E + gamma(L) sum|h0| + 2 u |E - E0|) + gamma(K) sum_k |dbeta_k (E - E0)|.
  * bmDCA: counts are integers and g = count / n one rounding: equality with the restatement's g; x and the record keep the
    tolerances of tests/test_boltzmann.py (x and eps bitwise, Pearson 1e-12)."""
import functools
import os
import subprocess

import numpy as np

import mf_shape_cases as MF
from plm_eval_reference import EXP_FACTOR, LD, fsum_ld, gamma, ulps_off
from test_ais import ais_ref, draw, start_ref, sweeps_ref                                       # noqa: F401
from test_boltzmann import bm_ref, data_stats, model_stats, record, update                      # noqa: F401
from test_potts_energies import _terms, mutation_ref                                           # noqa: F401
from test_potts_sampling import gibbs_ref, random_start, uniforms                              # noqa: F401
from test_pseudo_likelihood_host import conditionals_ref                                       # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
OWN = 2.0 ** -58
MARGIN_FACTOR = 10.0
SIGMA_SAMPLE, SIGMA_PLL = 0.5, 0.7
N_QUERIES, N_CHAINS = 600, 130            # one full block of 512 and a ragged one; two full workgroups and two chains
BETAS = (1.0, 0.5, 2.0)
SWEEPS = 3
ALL = ("energy", "pll", "sample", "ais", "bm")
MF_N = 200                                # sequences of a generated mf alignment


# ----------------------------------------------------------------------------- the case table
class Case:
    def __init__(self, q, L, src, reaches, facts, families=("energy", "pll", "sample", "ais"), chains=N_CHAINS, sweeps=SWEEPS,
                 mf=None, device_model_only=False):
        self.q, self.L, self.src, self.reaches, self.facts, self.families = q, L, src, reaches, facts, tuple(families)
        self.chains, self.sweeps, self.mf = chains, sweeps, mf
        self.device_model_only = device_model_only       # the CPU side forms no model of the case (an mf inverse of order > 10^4)
        self.elem = 4 if src == "f32" else 8
        self.dtype = np.dtype(np.float32 if src == "f32" else np.float64)
        self.P = L * q + L * (L - 1) // 2 * q * q
        self.name = "q%d_L%d_%s" % (q, L, src)

    def __repr__(self):
        return self.name


# A plm vector exists for q = 5 and q = 21 only (dca_plm_configure refuses every other alphabet), so kind 0 -- and with it every
# float32 instantiation and the bmDCA statistics -- is reachable at these two alphabets; the mf model (kind 1, float64) takes any q
# from 2 to 32 and carries the sweep over the alphabets.
MF_ENTRIES = ("energy", "pll", "sample", "ais")
CASES = [
    # kind 0
    Case(5, 131, "f32", "TS 24 in float32, nb 6; site CJ 16 with CPT 2, 8 x 16 + 3; sampler CJ 256, one chunk per row; TB 16, nb 9 ragged",
         dict(TS=24, nb=6, QM=8, CJ=16, CPT=2, KPB=1, siteChunks=9, siteLast=3, sCJ=256, nch=1, res=1, TB=16, bmNb=9), ALL),
    Case(5, 33, "f64", "TS 16 in float64, nb 3; site 2 x 16 + 1; sampler CJ 128; TB 16 in float64",
         dict(TS=16, nb=3, QM=8, CJ=16, siteChunks=3, siteLast=1, sCJ=128, nch=1, TB=16), ALL),
    Case(21, 20, "f32", "TS 6 in float32, four site blocks with a last one of 2; QM 24, site CJ 7 -> 2 x 7 + 6, KPB 3; sampler CJ 16 -> 16 + 4; "
         "TB 4, nb 5 exact", dict(TS=6, nb=4, QM=24, CJ=7, KPB=3, CPT=1, siteChunks=3, siteLast=6, sCJ=16, nch=2, sLast=4, TB=4, bmNb=5), ALL),
    Case(21, 19, "f64", "TS 4; site 6 x 3 + 1; sampler CJ 8 -> 8 + 8 + 3; TB 4 ragged in float64",
         dict(TS=4, CJ=3, siteChunks=7, siteLast=1, sCJ=8, nch=3, sLast=3, TB=4, bmNb=5), ALL),
    Case(5, 643, "f32", "state not resident at QM 8 in float32, three chunks (256 + 256 + 131)",
         dict(sQM=8, res=0, sCJ=256, nch=3, sLast=131), ("energy", "sample", "ais"), chains=64, sweeps=2),
    Case(21, 513, "f32", "state not resident at QM 24 in float32", dict(sQM=24, res=0), ("sample",), chains=64, sweeps=1),
    # kind 1: every float64 geometry, both sides of each q switch, gap row and column
    Case(2, 2, "mf", "kind 1 at q - 1 = 1; TS 24", dict(QM=8, TS=24), MF_ENTRIES, mf="N1_L2_q2"),
    Case(2, 70, "mf", "TS 24 with three site blocks; site CJ 16 with CPT 2, five chunks, last of 6; sampler CJ 320, one chunk per row",
         dict(TS=24, nb=3, QM=8, CJ=16, CPT=2, siteChunks=5, siteLast=6, sCJ=320, nch=1), MF_ENTRIES),
    Case(4, 49, "mf", "TS 24 at its largest q, three site blocks", dict(TS=24, nb=3), ("energy",)),
    Case(6, 33, "mf", "TS 16 at its largest q, three site blocks", dict(TS=16, nb=3), ("energy",)),
    Case(8, 20, "mf", "the top of QM 8; TS 12; sampler CJ 64", dict(QM=8, TS=12, sCJ=64, nch=1), MF_ENTRIES, mf="N700_L20_q8"),
    Case(8, 131, "mf", "site chunks 8 x 16 + 3; sampler CJ 64 -> 64 + 64 + 3; TS 12, nb 11",
         dict(TS=12, nb=11, QM=8, CJ=16, siteChunks=9, siteLast=3, sCJ=64, nch=3, sLast=3), MF_ENTRIES),
    Case(9, 20, "mf", "the bottom of QM 24; TS 8; sampler CJ 20, an exact fit", dict(QM=24, TS=8, sCJ=20, nch=1, sLast=20), MF_ENTRIES, mf="N700_L20_q9"),
    Case(9, 47, "mf", "TS 8; site CJ 3 -> 15 x 3 + 2; sampler CJ 20 -> 20 + 20 + 7",
         dict(TS=8, QM=24, CJ=3, KPB=3, siteChunks=16, siteLast=2, sCJ=20, nch=3, sLast=7), MF_ENTRIES),
    Case(16, 130, "mf", "TS 6, nb 22, 253 tiles -> tpg 2, G 127, last group of one tile, groups that cross a tile row",
         dict(TS=6, nb=22, ntiles=253, tpg=2, G=127, lastGroup=1), ("energy",)),
    Case(16, 27, "mf", "TS 6; site chunks exactly 9 x 3; sampler CJ 12 -> 12 + 12 + 3",
         dict(TS=6, QM=24, CJ=3, siteChunks=9, siteLast=3, sCJ=12, nch=3, sLast=3), MF_ENTRIES),
    Case(24, 9, "mf", "the top of QM 24; sampler CJ 4 -> 4 + 4 + 1; TS 4", dict(QM=24, sQM=24, TS=4, sCJ=4, nch=3, sLast=1), MF_ENTRIES),
    Case(25, 11, "mf", "the bottom of QM 32, KPB 4; TS 3; site CJ 2 -> 5 x 2 + 1; sampler CJ 4 -> 4 + 4 + 3",
         dict(TS=3, QM=32, KPB=4, CJ=2, siteChunks=6, siteLast=1, sCJ=4, nch=3, sLast=3), MF_ENTRIES),
    Case(25, 46, "mf", "TS 3 with nb 16, 136 tiles, tpg 2", dict(TS=3, nb=16, ntiles=136, tpg=2), ("energy",)),
    Case(32, 11, "mf", "tile = budget exactly; sampler chunk = 256 R exactly; largest LDS of each kernel",
         dict(TS=3, eLds=73728, eBudget=73728, chunkVals=4096, regVals=4096, QM=32, sQM=32), MF_ENTRIES),
    Case(32, 20, "mf", "q = 32 on the stage-shape alignment: sampler 5 x 4", dict(QM=32, TS=3, eLds=73728, nch=5), MF_ENTRIES, mf="N700_L20_q32"),
    Case(21, 8, "mf", "kind 1 on the toy protein golden", dict(QM=24), MF_ENTRIES, mf="mf_toy_protein"),
    Case(2, 643, "mf", "state not resident at QM 8 in float64, three chunks (320 + 320 + 3)",
         dict(sQM=8, res=0, sCJ=320, nch=3, sLast=3), ("energy", "sample", "ais"), chains=64, sweeps=2),
    Case(9, 513, "mf", "state not resident at QM 24 in float64", dict(sQM=24, res=0), ("sample", "pll"), chains=64, sweeps=1),
    # its inverse has order 12 312: the model exists on the device only, and the GPU test asserts the margin condition on it
    Case(25, 513, "mf", "state not resident at QM 32, 128 chunks of 4 and one of 1", dict(sQM=32, res=0, sCJ=4, nch=129, sLast=1),
         ("sample",), chains=64, sweeps=1, device_model_only=True),
]
# the shape of the block boundary (tests/test_potts_audit.py): not part of the table
BOUNDARY = [Case(5, 9, "f32", "n = 4097: a second block of 4096 sequences", {}, ())]
BY_NAME = {c.name: c for c in CASES + BOUNDARY}
assert len(BY_NAME) == len(CASES) + len(BOUNDARY)


def cases_of(family):
    return [c for c in CASES if family in c.families]


# ----------------------------------------------------------------------------- the launch geometry behind a program
def compile_plan_driver(directory):
    """tests/potts_plan_driver.cpp compiled with the host compiler -> driver(q, elem, L) = dict of every planned fact"""
    exe = os.path.join(str(directory), "potts_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fno-fast-math", "-ffp-contract=off", "-Wall",
                           "-I", os.path.join(ROOT, "pydca_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "potts_plan_driver.cpp")])
    cache = {}

    def driver(q, elem, L):
        key = (q, elem, L)
        if key not in cache:
            t = subprocess.check_output([exe, str(q), str(elem), str(L)]).split()
            cache[key] = {t[k].decode(): int(t[k + 1]) for k in range(0, len(t), 2)}
            assert (cache[key]["q"], cache[key]["elem"], cache[key]["L"]) == key
        return dict(cache[key])

    return driver


def plan_of(case, driver):
    """potts_plan.h's numbers for the case and what they make of its shape"""
    p = driver(case.q, case.elem, case.L)
    p["siteChunks"] = -(-case.L // p["CJ"])
    p["siteLast"] = case.L - (p["siteChunks"] - 1) * p["CJ"]
    p["sLast"] = case.L - (p["nch"] - 1) * p["sCJ"]
    p["lastGroup"] = p["ntiles"] - (p["G"] - 1) * p["tpg"]
    p["bmTiles"] = p["bmNb"] * (p["bmNb"] + 1) // 2
    p["bmRagged"] = int(case.L % p["TB"] != 0)
    return p


# ----------------------------------------------------------------------------- inputs
def plm_model(x, L, q):
    x = np.asarray(x, dtype=np.float64)
    return x[:L * q].reshape(L, q), x[L * q:].reshape(-1, q, q)


class LazyPairs:
    """the pair blocks of a stored vector, widened to float64 where they are read (the dense float64 table of q 25, L 513 would
    be 0.66 GB)"""
    def __init__(self, x, L, q):
        self.J = x[L * q:].reshape(-1, q, q)

    def __getitem__(self, idx):
        return self.J[idx].astype(np.float64)


@functools.lru_cache(maxsize=2)
def mf_model_cached(name):
    return mf_model_cpu(BY_NAME[name])


@functools.lru_cache(maxsize=2)
def plm_x(name, sigma):
    """the case's parameter vector in its element type"""
    case = BY_NAME[name]
    rng = np.random.default_rng([case.q, case.L, case.elem, int(round(10 * sigma))])
    x = rng.standard_normal(case.P, dtype=np.float32 if case.P > 10 ** 7 else np.float64) * case.dtype.type(sigma)
    x = x.astype(case.dtype)
    x.setflags(write=False)
    return x


def training_alignment(case, N=40):
    return np.random.default_rng([7, case.q, case.L]).integers(0, case.q, size=(N, case.L), dtype=np.uint8)


def mf_alignment(case):
    """-> (X uint8[N, L] 0-based codes with the gap at q - 1, weights float64[N] or None for compute_weights(0.8))"""
    if case.mf is None:                         # random columns, each with its own state frequencies, and dyadic weights
        rng = np.random.default_rng([3, case.q, case.L])
        X = np.stack([rng.choice(case.q, size=MF_N, p=rng.dirichlet(np.ones(case.q))).astype(np.uint8) for _ in range(case.L)], axis=1)
        return X, rng.integers(1, 9, MF_N) / 8.0
    if case.mf in MF.BY_NAME:
        X, k = MF.alignment(case.mf)
        return np.array(X), k / 8.0
    G = np.load(os.path.join(ROOT, "tests", "golden", case.mf + ".npz"))
    return (G["X"] - 1).astype(np.uint8), None


class LazyMfPairs:
    """the pair blocks of a dense mf coupling matrix with their zero gap row and column, built where they are read (the pair
    table of q 25, L 513 would be 0.66 GB beside the matrix)"""
    def __init__(self, J, L, q):
        self.J4, self.q = np.asarray(J).reshape(L, q - 1, L, q - 1), q
        self.iu, self.ju = np.triu_indices(L, 1)

    def __getitem__(self, idx):
        idx = np.asarray(idx)
        out = np.zeros(idx.shape + (self.q, self.q))
        out[..., :self.q - 1, :self.q - 1] = self.J4[self.iu[idx], :, self.ju[idx], :]
        return out


def mf_model_lazy(J, fields, L, q):
    h = np.zeros((L, q))
    h[:, :q - 1] = fields
    return h, LazyMfPairs(J, L, q)


def mf_model(J, fields, L, q):
    """Dense -inv(C) (L(q-1) square) and fields (L x (q-1)) -> h, Jp with zero gap rows / columns."""
    qm = q - 1
    h = np.zeros((L, q))
    h[:, :qm] = fields
    J4 = np.asarray(J).reshape(L, qm, L, qm)
    iu, ju = np.triu_indices(L, 1)
    Jp = np.zeros((iu.size, q, q))
    Jp[:, :qm, :qm] = J4[iu, :, ju, :]
    return h, Jp


def mf_model_cpu(case):
    """the oracle's float64 mf model of the case's alignment (the CPU stand-in for mf_couplings() / mf_fields())"""
    from oracle import mf as omf
    X, w = mf_alignment(case)
    L, q = case.L, case.q
    X1 = X.astype(np.int64) + 1
    if w is None:
        w = omf.compute_sequences_weight(X1, 0.8)
    fi = omf.get_reg_single_site_freqs(omf.compute_single_site_freqs(X1, q, w), L, q, MF.THETA)
    fij = omf.get_reg_pair_site_freqs(omf.compute_pair_site_freqs(X1, q, w), L, q, MF.THETA)
    J = omf.compute_couplings(omf.construct_corr_mat(fi, fij, L, q))
    return mf_model(J, omf.compute_fields(J, fi, L, q), L, q)


def model_of(case, sigma):
    """(h, Jp) float64 of a plm case's stored vector, or the CPU mf model"""
    if case.src == "mf":
        return mf_model_cached(case.name)
    x = plm_x(case.name, sigma)
    if case.P > 10 ** 7:
        return x[:case.L * case.q].reshape(case.L, case.q).astype(np.float64), LazyPairs(x, case.L, case.q)
    return plm_model(x, case.L, case.q)


def queries(case, n=N_QUERIES, seed=0):
    return np.random.default_rng([11, case.q, case.L, seed]).integers(0, case.q, size=(n, case.L), dtype=np.uint8)


def base_fields(case):
    return np.random.default_rng([13, case.q, case.L]).normal(0, 1.0, (case.L, case.q))


def pair_table(L):
    iu, ju = np.triu_indices(L, 1)
    pidx = np.zeros((L, L), dtype=np.int64)
    pidx[iu, ju] = np.arange(iu.size)
    pidx[ju, iu] = np.arange(iu.size)
    return iu, ju, pidx


# ----------------------------------------------------------------------------- the audit's verdict
class Audit:
    """ratios = |device - reference| / bound per element; identities: named bit equalities that failed"""
    def __init__(self, what, ratios, identities=()):
        self.what = what
        self.ratios = np.asarray(ratios, dtype=np.float64)
        self.checked = self.ratios.size
        r = np.where(np.isfinite(self.ratios), self.ratios, np.inf)
        self.worst = float(r.max()) if r.size else 0.0
        self.failing = np.argwhere(~(r <= 1.0))
        self.identities = list(identities)

    @property
    def ok(self):
        return len(self.failing) == 0 and not self.identities

    def summary(self):
        return "%s: %d elements, worst error / bound %.3g" % (self.what, self.checked, self.worst)

    def report(self):
        lines = [self.summary(), "%d elements out of bound" % len(self.failing)]
        lines += ["    element %s: ratio %.3g" % (tuple(int(v) for v in e), self.ratios[tuple(e)]) for e in self.failing[:12]]
        return "\n".join(lines + ["    identity broken: " + s for s in self.identities])


def ratio(dev, ref, bound):
    """|dev - ref| / bound in longdouble; 0 where both the error and the bound are 0"""
    err = np.abs(np.asarray(dev).astype(LD) - ref)
    b = np.asarray(bound).astype(LD)
    out = np.where(err == 0, LD(0), err / np.where(b > 0, b, LD(1)))
    return np.where((b <= 0) & (err > 0), np.inf, out).astype(np.float64)


def assert_ok(*audits):
    for a in audits:
        assert a.ok, a.report()


# ----------------------------------------------------------------------------- energies and the scan
class EnergyRef:
    pass


def energy_reference(h, Jp, X, G):
    """E per sequence in longdouble (fsum_ld over the exact terms) and its bound"""
    L = h.shape[0]
    iu, ju, _ = pair_table(L)
    p = np.arange(iu.size)
    ref = EnergyRef()
    ref.E = np.zeros(X.shape[0], dtype=LD)
    ref.S = np.zeros(X.shape[0])
    for n in range(X.shape[0]):
        x = X[n].astype(np.int64)
        terms = np.concatenate([h[np.arange(L), x], np.asarray(Jp[p, x[iu], x[ju]], dtype=np.float64)])
        ref.E[n] = fsum_ld(terms)
        ref.S[n] = float(fsum_ld(np.abs(terms)))
    ref.k = L + iu.size
    ref.bound = gamma(ref.k + G, U) * ref.S * (1 + 2 * U)
    return ref


def audit_energies(ref, E):
    assert E.shape == ref.E.shape and E.dtype == np.float64
    return Audit("energies", ratio(E, ref.E, ref.bound))


def site_sums(h, Jp, w, dtype, fault=None, plan=None):
    """S[i, a] = sum_{j != i, ascending} J_ij(a, w_j) and A[i, a] = the same over |J|, accumulated in `dtype`.  fault: a faulty
    variant (negative controls): 'untransposed' reads the stored block as it lies for j < i; 'self' adds the neighbour j = i (the
    block that follows the site's last in memory); 'ragged' drops the last neighbour of a ragged last chunk."""
    L, q = h.shape
    _, _, pidx = pair_table(L)
    S = np.zeros((L, q), dtype=dtype)
    A = np.zeros((L, q), dtype=dtype)
    for i in range(L):
        Jrow = np.asarray(Jp[pidx[i]], dtype=np.float64)            # L x q x q, the block (min, max)
        if fault != "untransposed":
            Jrow[:i] = Jrow[:i].transpose(0, 2, 1)                  # j < i: J_ij(a, b) = block(j, i)[b, a]
        T = Jrow[np.arange(L), :, w.astype(np.int64)].astype(dtype)  # L x q: J_ij(., w_j)
        for j in range(L):
            if j == i and fault != "self":
                continue
            if fault == "ragged" and j == L - 1 and L % plan["CJ"] and i != j:
                continue
            S[i] = S[i] + T[j]
            A[i] = A[i] + np.abs(T[j])
    return S, A


class ScanRef:
    pass


def scan_reference(h, Jp, w):
    L, q = h.shape
    S, A = site_sums(h, Jp, w, LD)
    wi = w.astype(np.int64)
    rows = np.arange(L)
    hl = h.astype(LD)
    ref = ScanRef()
    ref.w = wi
    ref.dE = (hl - hl[rows, wi][:, None]) + (S - S[rows, wi][:, None])
    ref.dE[rows, wi] = 0
    scale = (np.abs(h) + np.abs(h[rows, wi])[:, None] + (A + A[rows, wi][:, None]).astype(np.float64))
    ref.bound = (gamma(L + 3, U) + OWN) * scale
    ref.bound[rows, wi] = 0.0
    return ref


def audit_scan(ref, dE):
    assert dE.shape == ref.dE.shape
    a = Audit("mutation scan", ratio(dE, ref.dE, ref.bound))
    L = dE.shape[0]
    if not np.all(dE[np.arange(L), ref.w].view(np.uint64) == 0):
        a.identities.append("dE(i, w_i) is not +0.0 everywhere")
    return a


# ----------------------------------------------------------------------------- site conditionals
class CondRef:
    pass


def site_table(h, Jp, X, dtype, fault=None, plan=None):
    """u[n, i, a] = h_i(a) + sum_{j != i, ascending} J_ij(a, s_nj) and Uabs likewise, accumulated in `dtype` (longdouble: the
    reference; float64 with a fault: a negative control).  Faults as site_sums, and 'next_fields': the fields of site i + 1."""
    n = X.shape[0]
    L, q = h.shape
    u = np.zeros((n, L, q), dtype=dtype)
    A = np.zeros((n, L, q), dtype=dtype)
    _, _, pidx = pair_table(L)
    Xi = X.astype(np.int64)
    for i in range(L):
        hi = h[(i + 1) % L] if fault == "next_fields" else h[i]
        acc = np.repeat(hi.astype(dtype)[None, :], n, axis=0)
        ab = np.abs(acc)
        Jrow = np.asarray(Jp[pidx[i]], dtype=np.float64)
        if fault != "untransposed":
            Jrow[:i] = Jrow[:i].transpose(0, 2, 1)
        for j in range(L):
            if j == i and fault != "self":
                continue
            if fault == "ragged" and j == L - 1 and L % plan["CJ"]:
                continue
            t = Jrow[j].T[Xi[:, j]].astype(dtype)                    # n x q: J_ij(., s_nj)
            acc = acc + t
            ab = ab + np.abs(t)
        u[:, i], A[:, i] = acc, ab
    return u, A


def conditionals_of(u, X, fault=None):
    """cond, site, pll from u in u's type, in the kernel's order (ascending states, ascending sites).  Faults: 'no_last_state'
    leaves state q - 1 out of the softmax, 'padding_lane' reads the padding lane q (u = 0) as a state."""
    n, L, q = u.shape
    m = u.max(axis=2, keepdims=True)
    if fault == "padding_lane":
        m = np.maximum(m, 0)
    e = np.exp(u - m)
    Z = np.zeros((n, L), dtype=u.dtype)
    for a in range(q - 1 if fault == "no_last_state" else q):
        Z = Z + e[:, :, a]
    if fault == "padding_lane":
        Z = Z + np.exp(0 - m[:, :, 0])
    lz = np.log(Z)
    cond = (u - m) - lz[:, :, None]
    site = cond[np.arange(n)[:, None], np.arange(L)[None, :], X.astype(np.int64)]
    pll = np.zeros(n, dtype=u.dtype)
    for i in range(L):
        pll = pll + site[:, i]
    return cond, site, pll, lz


def cond_reference(h, Jp, X):
    L, q = h.shape
    ref = CondRef()
    ref.X = X
    u, A = site_table(h, Jp, X, LD)
    ref.cond, ref.site, ref.pll, lz = conditionals_of(u, X)
    Uabs = A.astype(np.float64) * (1 + 2 * U)
    u64 = u.astype(np.float64)
    d64 = u64 - u64.max(axis=2, keepdims=True)
    ref.exp_ulps = ulps_off(np.exp(d64), np.exp(d64.astype(LD)))
    Z64 = np.exp(d64).sum(axis=2)
    ref.log_ulps = ulps_off(np.log(Z64), np.log(Z64.astype(LD)))
    ref.eps_exp = EXP_FACTOR * max(ref.exp_ulps, 0.5) * 2 * U
    ref.eps_log = EXP_FACTOR * max(ref.log_ulps, 0.5) * 2 * U
    du = gamma(L, U) * Uabs
    dumax = du.max(axis=2, keepdims=True)
    delta = du + U * (np.abs(d64) + dumax) * (1 + 2 * U)
    P64 = np.exp(ref.cond).astype(np.float64)
    rho = (P64 * delta).sum(axis=2) * (1 + 2 * U) + ref.eps_exp + gamma(q - 1, U)
    dlz = rho / (1 - rho) + ref.eps_log * (np.abs(lz).astype(np.float64) + dumax[:, :, 0])
    c64 = np.abs(ref.cond).astype(np.float64)
    ref.cond_bound = delta + dlz[:, :, None] + U * c64 * (1 + 2 * U) + OWN * (Uabs + 1 + c64)
    ref.site_bound = ref.cond_bound[np.arange(X.shape[0])[:, None], np.arange(L)[None, :], X.astype(np.int64)]
    ref.pll_bound = ref.site_bound.sum(axis=1) * (1 + 2 * U) + gamma(L, U) * np.abs(ref.site).sum(axis=1).astype(np.float64)
    return ref


def audit_conditionals(ref, pll, site, cond):
    """the three outputs against the reference, and the two bit identities between them"""
    n, L = ref.X.shape
    assert pll.shape == (n,) and site.shape == (n, L) and cond.shape == ref.cond.shape
    ids = []
    picked = cond[np.arange(n)[:, None], np.arange(L)[None, :], ref.X.astype(np.int64)]
    if picked.tobytes() != site.tobytes():
        ids.append("site != cond[s_i] in %d places" % int(np.count_nonzero(picked.view(np.uint64) != site.view(np.uint64))))
    total = np.zeros(n)
    for i in range(L):
        total = total + site[:, i]
    if total.tobytes() != np.ascontiguousarray(pll).tobytes():
        ids.append("PLL != the ascending-i sum of site in %d sequences" % int(np.count_nonzero(total != pll)))
    return (Audit("cond", ratio(cond, ref.cond, ref.cond_bound), ids), Audit("site", ratio(site, ref.site, ref.site_bound)),
            Audit("PLL", ratio(pll, ref.pll, ref.pll_bound)))


# ----------------------------------------------------------------------------- chains: exact codes under the margin condition
def model_sabs(h, Jp, h0=None):
    """an upper bound of sum|terms| of any site sum of the model"""
    L = h.shape[0]
    iu, ju, _ = pair_table(L)
    step = 4096
    jm = np.concatenate([np.abs(np.asarray(Jp[np.arange(s, min(s + step, iu.size))])).max(axis=(1, 2)) for s in range(0, iu.size, step)]) \
        if iu.size else np.zeros(0)
    per_site = np.abs(h).max(axis=1)
    np.add.at(per_site, iu, jm)
    np.add.at(per_site, ju, jm)
    if h0 is not None:
        per_site = per_site + np.abs(h0).max(axis=1)
    return float(per_site.max())


def eps_draw(q, L, beta, sabs):
    """(q + 2) (beta gamma(L + 3) Sabs + eps_exp): eps_exp from numpy's exp against longdouble over the arguments a draw can
    meet, [-2 beta Sabs, 0]"""
    args = -np.linspace(0.0, 2.0 * beta * sabs, 20001)
    eps_exp = EXP_FACTOR * max(ulps_off(np.exp(args), np.exp(args.astype(LD))), 0.5) * 2 * U
    return (q + 2) * (beta * gamma(L + 3, U) * sabs + eps_exp)


def assert_margin(case, margin, beta, sabs):
    need = MARGIN_FACTOR * eps_draw(case.q, case.L, beta, sabs)
    assert margin >= need, "%s: the smallest draw margin %.3g is below %.3g: change the seed" % (case.name, margin, need)
    return need


def seed_of(case, k=0):
    return 1000 * case.q + case.L + 17 * k + (case.elem == 8)


def sample_runs(case):
    """(beta, given start or None, first chain, first sweep) of the case's plain-sweep runs"""
    runs = [(BETAS[0], False, 0, 0), (BETAS[1], True, 3, 2), (BETAS[2], False, 0, 0)]
    return runs if case.L <= 512 else runs[:2] if case.q <= 5 else runs[:1]


def sample_reference(case, h, Jp, fault=None):
    """per run (beta, X0 or None, first_chain, first_sweep, seed, expected codes); asserts the margin condition"""
    sabs = model_sabs(h, Jp)
    out = []
    for k, (beta, given, c0, s0) in enumerate(sample_runs(case)):
        seed = seed_of(case, k)
        chains = np.arange(c0, c0 + case.chains)
        X0 = queries(case, case.chains, seed=5 + k) if given else None
        start = X0 if given else random_start(seed, chains, case.L, case.q)
        codes, margin = gibbs_ref(h, Jp, beta, seed, chains, s0, case.sweeps, start)
        if fault is None:
            assert_margin(case, margin, beta, sabs)
        out.append((beta, X0, c0, s0, seed, codes, margin))
    return out


def audit_codes(what, expected, got):
    assert got.shape == expected.shape and got.dtype == np.uint8
    return Audit(what, (got != expected).astype(np.float64) * 2.0)


# ----------------------------------------------------------------------------- AIS
class AisRef:
    pass


def ais_runs(case):
    """(K, sweeps per temperature, base fields or None, betas or None, first chain) of the case's runs"""
    if case.L > 131:
        return [(2, 1, base_fields(case), None, 5)]
    return [(3, 2, base_fields(case), None, 5), (3, 1, None, [0.0, 0.1, 0.7, 1.0], 0)]


def ais_reference(case, h, Jp, G, run, k=0):
    """chains and log weights of one run: the chains from ais_ref (each step's state is the final state of the run cut after that
    step), the log weights in longdouble from them"""
    K, s, h0, betas, c0 = run
    base = h if h0 is None else h0
    b = np.arange(K + 1) / K if betas is None else np.asarray(betas, dtype=np.float64)
    seed = seed_of(case, 50 + k)
    chains = np.arange(c0, c0 + case.chains)
    L = case.L
    ref = AisRef()
    ref.args = dict(K=K, s=s, seed=seed, first_chain=c0, betas=betas, base_fields=h0)
    ref.logw = np.zeros(case.chains, dtype=LD)
    ref.bound = np.zeros(case.chains)
    running = np.zeros(case.chains)
    margin = np.inf
    for step in range(1, K + 1):
        X, _w, lz0, m = ais_ref(h, Jp, base, step, s, seed, chains, b[:step + 1] if step > 1 else [b[0], b[1]])
        margin = min(margin, m)
        er = energy_reference(h, Jp, X, G)
        e0t = base[np.arange(L)[None, :], X.astype(np.int64)]
        e0 = np.array([fsum_ld(r) for r in e0t], dtype=LD)
        db = b[step] - b[step - 1]
        diff = er.E - e0
        ref.logw = ref.logw + LD(db) * diff
        ad = np.abs(diff).astype(np.float64)
        ref.bound += abs(db) * (er.bound + gamma(L, U) * np.abs(e0t).sum(axis=1) + 2 * U * ad) * (1 + 4 * U)
        running += abs(db) * ad
    ref.bound += gamma(K, U) * running + OWN * running
    ref.codes, ref.margin = X, margin
    ref.lz0 = sum(float(m_) + float(np.log(np.exp(base[i] - m_).sum())) for i, m_ in enumerate(base.max(axis=1)))
    assert_margin(case, margin, 1.0, model_sabs(h, Jp, base))
    return ref


def audit_ais(ref, logw, codes):
    return audit_codes("AIS chains", ref.codes, codes), Audit("AIS log weights", ratio(logw, ref.logw, ref.bound))


# ----------------------------------------------------------------------------- bmDCA
BM_RATES = (0.3, 0.2, 0.01, 0.02)
BM_LAMBDA = 0.02
BM_K, BM_E, BM_T = 1, 1, 2


def bm_reference(case, x, X, extra_chain=False):
    """bm_ref on the case: per iteration (chains, x, g_i, g_ij, record).  extra_chain: the counts of n + 1 chains (negative
    control)."""
    fi, fij = data_stats(X, np.ones(X.shape[0]), case.q, BM_LAMBDA)
    n = case.chains + (1 if extra_chain else 0)
    return fi, fij, bm_ref(x.copy(), fi, fij, n, BM_K, BM_E, BM_T, seed_of(case, 90), BM_RATES)


def audit_bm(what, want, got):
    """(chains, x, g_i, g_ij, record) of one iteration: codes, counts and x bitwise, the record as tests/test_boltzmann.py"""
    S, x, gi, gij, rec = want
    S_, x_, gi_, gij_, rec_ = got
    bad = []
    if S_.shape != S.shape or not np.array_equal(S_, S):
        bad.append("chains differ")
    if gi_.tobytes() != gi.tobytes() or gij_.tobytes() != gij.tobytes():
        bad.append("g differs in %d + %d values" % (int(np.count_nonzero(gi_ != gi)), int(np.count_nonzero(gij_ != gij))))
    if x_ is not None and x_.tobytes() != x.tobytes():
        bad.append("x differs in %d values" % int(np.count_nonzero(x_ != x)))
    if rec_ is not None:
        if rec_[:2].tobytes() != rec[:2].tobytes():
            bad.append("eps differ: %r against %r" % (rec_[:2], rec[:2]))
        if not abs(rec_[2] - rec[2]) <= 1e-12:
            bad.append("Pearson %r against %r" % (rec_[2], rec[2]))
    return Audit(what, np.zeros(S.size), bad)


# ----------------------------------------------------------------------------- the energies in the kernel's tile order
def energy_by_tiles(h, Jp, X, plan, fault=None):
    """float64 energies in energy_pairs_kernel's order: per group the tiles ascending, per tile the pairs in (i, j) order, then the
    fields and the slabs ascending.  fault 'last_tile': the last tile of every group of more than one is dropped; 'diagonal': the
    pairs of the diagonal tiles are counted twice."""
    L = h.shape[0]
    TS, nb, tpg, ntiles = plan["TS"], plan["nb"], plan["tpg"], plan["ntiles"]
    _, _, pidx = pair_table(L)
    Xi = X.astype(np.int64)
    tiles = [(bi, bj) for bi in range(nb) for bj in range(bi, nb)]
    assert len(tiles) == ntiles
    slabs = []
    for g in range(plan["G"]):
        acc = np.zeros(X.shape[0])
        mine = tiles[g * tpg:min(ntiles, (g + 1) * tpg)]
        for t, (bi, bj) in enumerate(mine):
            if fault == "last_tile" and len(mine) > 1 and t == len(mine) - 1:
                continue
            for _rep in range(2 if fault == "diagonal" and bi == bj else 1):
                for i in range(bi * TS, min(L, bi * TS + TS)):
                    for j in range(bj * TS, min(L, bj * TS + TS)):
                        if j > i:
                            acc = acc + np.asarray(Jp[pidx[i, j]], dtype=np.float64)[Xi[:, i], Xi[:, j]]
        slabs.append(acc)
    E = np.zeros(X.shape[0])
    for i in range(L):
        E = E + h[i, Xi[:, i]]
    for s in slabs:
        E = E + s
    return E
