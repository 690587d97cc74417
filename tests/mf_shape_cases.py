"""TEST INFRASTRUCTURE ONLY -- constructed alignments and exact references for the mfDCA stage kernels at the shapes where
pydca_amd/csrc/mf_engine.hip changes path (tests/test_mf_stage_shapes.py on the GPU, tests/test_mf_stage_shapes_host.py
pins this module on the CPU).

Alignments use the device coding: states 0 .. q-1, gap = q-1.

Exact counts.  With weights w_n = k_n / 8, k_n in 1..8, every weighted count is (an integer) / 8 and Meff is (an integer) / 8:
the counts are formed here as int64 sums of the k_n and divided ONCE by the integer Meff.  A float64 sum of such weights in
any order is exact as well (every partial sum is a multiple of 1/8 below 2^53), so a kernel that adds the right sequences into
the right slot and divides once reproduces these frequencies bit for bit, and one that drops, doubles or misplaces a sequence
does not.  General weights (1 / count) are summed per bucket with math.fsum (correctly rounded)."""
import functools
import math

import numpy as np

from oracle import mf as omf

THETA = 0.5                     # pseudocount of every case
U = 2.0 ** -53                  # unit roundoff of float64
# Non-dominant bucket lengths that the counts kernel's 32-entry batch loop, its tail loop and the prefetch guard
# (k + 2 * 32 <= k1) tell apart: nothing, tail only, one batch short by one / exact / plus one, the same for two batches, and
# three batches exact / plus one.
BUCKET_EDGES = (0, 1, 31, 32, 33, 63, 64, 65, 96, 97)


class Case:
    def __init__(self, N, L, q, planted=False, weights="dyadic", seed=0):
        self.N, self.L, self.q, self.planted, self.weights, self.seed = N, L, q, planted, weights, seed
        self.n = L * (q - 1)
        self.name = "N%d_L%d_q%d%s" % (N, L, q, "" if weights == "dyadic" else "_" + weights)
        self.inverse = self.n <= 1100           # the reference inverse is LAPACK: seconds beyond that

    def __repr__(self):
        return self.name


# each the smallest shape that reaches the branch named beside it
CASES = [
    Case(1, 2, 2),                       # smallest legal problem; q-1 = 1; every non-dominant bucket empty
    Case(63, 5, 4),                      # N < 64; n = 15: no multiple of 4 (rows per thread of the corr kernel) or 64; generic corr
    Case(257, 9, 5, planted=True),       # sort segments of 2 with empty trailing segments; planted buckets; prefetch instance
    Case(513, 9, 21, planted=True),      # segments of 3, ragged last one; planted buckets; non-prefetch instance
    Case(700, 20, 32),                   # q at its limit: full LDS tables in sort and counts
    Case(700, 20, 8),                    # both sides of the q <= 8 dispatch, generic corr
    Case(700, 20, 9),
    Case(300, 258, 5),                   # second site block of row i = 0 holds one site; n = 1032 wraps the fields loop four times
    Case(300, 257, 5),                   # exactly one full site block for i = 0
    Case(64, 258, 21),                   # the same wrap on the q = 21 instance (n = 5160: no inverse)
    Case(600, 70, 5, weights="general"),  # n = 280 > 256 with 1 / count weights
]
BY_NAME = {c.name: c for c in CASES}
DYADIC = [c for c in CASES if c.weights == "dyadic"]
GENERAL = [c for c in CASES if c.weights == "general"]


# ----------------------------------------------------------------------------- alignments
def _planted_counts(N, q):
    """State counts of the planted columns (each sums to N)."""
    gap = q - 1
    cols = []
    c = np.zeros(q, dtype=np.int64)             # dominant state = gap; buckets 0, 1, 31, 32
    c[0], c[1], c[2] = 1, 31, 32
    c[gap] = N - 64
    cols.append(c)
    c = np.zeros(q, dtype=np.int64)             # buckets 33, 63, 64
    c[1], c[2], c[3] = 33, 63, 64
    c[0] = N - 160
    cols.append(c)
    c = np.zeros(q, dtype=np.int64)             # states 1 and 3 tied for dominant at 96 (one of them is walked); bucket 65
    c[1], c[3], c[0] = 96, 96, 65
    rest = N - 257
    for a in range(4, q):                       # what is left goes to further states, 64 at a time (below the tie)
        c[a] = min(64, rest)
        rest -= c[a]
    assert rest == 0
    cols.append(c)
    c = np.zeros(q, dtype=np.int64)             # bucket 97
    c[2] = 97
    c[3] = N - 97
    cols.append(c)
    c = np.zeros(q, dtype=np.int64)             # constant column
    c[2] = N
    cols.append(c)
    return cols


def nondominant_bucket_lengths(X, q):
    """Lengths of the buckets the counts kernel walks: per site except the last one (its rows have no j > i), every state but the
    dominant one -- the FIRST state with the largest count, whose row is filled by complement."""
    out = set()
    for i in range(X.shape[1] - 1):
        c = np.bincount(X[:, i], minlength=q)
        out |= {int(v) for a, v in enumerate(c) if a != int(np.argmax(c))}
    return out


def check_planted(X, q):
    """The edges a planted alignment exists for; asserted on the builder's own output."""
    N = X.shape[0]
    counts = [np.bincount(X[:, i], minlength=q) for i in range(X.shape[1] - 1)]
    missing = set(BUCKET_EDGES) - nondominant_bucket_lengths(X, q)
    assert not missing, "bucket lengths %s are not planted" % sorted(missing)
    assert any(c.max() == N for c in counts), "no constant column"
    assert any(int(np.argmax(c)) == q - 1 and np.sum(c == c.max()) == 1 for c in counts), "no column dominated by the gap"
    assert any(np.sum(c == c.max()) == 2 for c in counts), "no column with two states tied for dominant"


def _random_column(rng, N, q):
    return rng.choice(q, size=N, p=rng.dirichlet(np.ones(q))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def alignment(name):
    """-> (X uint8[N, L] read-only, k int64[N] read-only or None): the alignment and the numerators of its weights k / 8."""
    case = BY_NAME[name]
    N, L, q = case.N, case.L, case.q
    rng = np.random.default_rng([case.seed, N, L, q])
    if case.weights == "general":               # near-duplicates, so that 1 / count weights differ from 1
        base = np.stack([_random_column(rng, 150, q) for _ in range(L)], axis=1)
        X = base[rng.integers(0, 150, N)].copy()
        hit = rng.random(X.shape) < 0.05
        X[hit] = rng.integers(0, q, int(hit.sum()), dtype=np.uint8)
        k = None
    else:
        X = np.stack([_random_column(rng, N, q) for _ in range(L)], axis=1)
        if case.planted:
            sites = [0, 1, 3, 4, 6]             # all before the last site, random columns between and after them
            for site, c in zip(sites, _planted_counts(N, q)):
                assert c.sum() == N and c.min() >= 0
                X[:, site] = rng.permutation(np.repeat(np.arange(q), c)).astype(np.uint8)
            check_planted(X, q)
        if N == 1:
            X[0, 0], X[0, 1] = 0, q - 1
        k = rng.integers(1, 9, N).astype(np.int64)
        k.setflags(write=False)
    assert X.shape == (N, L) and X.max() < q
    X.setflags(write=False)
    return X, k


# ----------------------------------------------------------------------------- counts
def exact_counts(X, q, k):
    """int64 weighted counts of weights k / 8, times 8: single[L, q], pair[pairs, q, q] (pair order (0,1),(0,2),..., gap state
    included) and Meff * 8."""
    X = np.asarray(X).astype(np.int64)
    k = np.asarray(k, dtype=np.int64)
    N, L = X.shape
    Xr = np.repeat(X, k, axis=0)                # sequence n stands k_n times: plain integer histograms from here on
    single = np.stack([np.bincount(Xr[:, i], minlength=q) for i in range(L)])
    pair = np.zeros((L * (L - 1) // 2, q, q), dtype=np.int64)
    cols = np.arange(L, dtype=np.int64) * q
    p = 0
    for i in range(L - 1):
        code = (Xr[:, i, None] * (L * q) + cols[None, i + 1:] + Xr[:, i + 1:]).ravel()
        h = np.bincount(code, minlength=q * L * q).reshape(q, L, q)
        pair[p:p + L - 1 - i] = h[:, i + 1:, :].transpose(1, 0, 2)
        p += L - 1 - i
    return single, pair, int(k.sum())


def exact_freqs(X, q, k):
    """(fi[L, q], fij[pairs, q, q]) with the gap state: each an integer count divided once by the integer Meff."""
    single, pair, meff = exact_counts(X, q, k)
    return single / meff, pair / meff


def fsum_freqs(X, q, w):
    """The same frequencies for arbitrary float64 weights: math.fsum per bucket, divided by math.fsum(w)."""
    X = np.asarray(X).astype(np.int64)
    w = np.asarray(w, dtype=np.float64)
    N, L = X.shape
    meff = math.fsum(w.tolist())

    def buckets(code, size):
        order = np.argsort(code, kind="stable")
        edges = np.searchsorted(code[order], np.arange(size + 1))
        ws = w[order].tolist()
        return [math.fsum(ws[edges[c]:edges[c + 1]]) for c in range(size)]

    fi = np.array([buckets(X[:, i], q) for i in range(L)]) / meff
    fij = np.zeros((L * (L - 1) // 2, q, q))
    p = 0
    for i in range(L - 1):
        for j in range(i + 1, L):
            fij[p] = np.array(buckets(X[:, i] * q + X[:, j], q * q)).reshape(q, q)
            p += 1
    return fi, fij / meff


# ----------------------------------------------------------------------------- everything downstream: oracle/mf.py
class Reference:
    """Reference side of one case from its frequencies (gap state included); nothing here ever sees a device result."""

    def __init__(self, X, q, fi, fij_gap, theta=THETA):
        self.X, self.q, self.theta = X, q, theta
        self.N, self.L = X.shape
        self.fi, self.fij_gap = fi, fij_gap
        self.fij = np.ascontiguousarray(fij_gap[:, :q - 1, :q - 1])

    @functools.cached_property
    def reg_fi(self):
        return omf.get_reg_single_site_freqs(self.fi, self.L, self.q, self.theta)

    @functools.cached_property
    def reg_fij(self):
        return omf.get_reg_pair_site_freqs(self.fij, self.L, self.q, self.theta)

    @functools.cached_property
    def corr(self):
        return omf.construct_corr_mat(self.reg_fi, self.reg_fij, self.L, self.q)

    @functools.cached_property
    def couplings(self):
        return omf.compute_couplings(self.corr)

    @functools.cached_property
    def fields(self):
        return omf.compute_fields(self.couplings, self.reg_fi, self.L, self.q)

    @functools.cached_property
    def fn(self):
        return omf.frobenius_from_blocks(omf.mf_blocks(self.couplings, self.L, self.q))

    def scores(self, apc):
        if not apc:
            return self.fn
        with np.errstate(invalid="ignore"):     # q = 2: every block is 1 x 1, every FN is 0 and the correction is 0 / 0
            return omf.apc(self.fn, self.L)

    def bm_freqs(self, lam):
        """Data statistics of a Boltzmann-learning run in the kernel's order of operations:
        (1 - lam) * f + lam / q, (1 - lam) * f + lam / q^2."""
        om = 1.0 - lam
        return om * self.fi + lam / float(self.q), om * self.fij_gap + lam / float(self.q * self.q)

    def energies(self, Q):
        """Potts energies sum_i h_i(x_i) + sum_{i<j} J_ij(x_i, x_j) of the rows of Q under the reference fields and couplings
        (zero on the gap state) -> (E, sum of |terms|)."""
        L, q, qm = self.L, self.q, self.q - 1
        h = np.zeros((L, q))
        h[:, :qm] = self.fields
        J = np.zeros((L, q, L, q))
        J[:, :qm, :, :qm] = self.couplings.reshape(L, qm, L, qm)
        iu, ju = np.triu_indices(L, 1)
        Q = np.asarray(Q).astype(np.int64)
        hf = h[np.arange(L)[None, :], Q]
        jt = J[iu[None, :], Q[:, iu], ju[None, :], Q[:, ju]]
        return hf.sum(1) + jt.sum(1), np.abs(hf).sum(1) + np.abs(jt).sum(1)


@functools.lru_cache(maxsize=None)
def dyadic_reference(name):
    X, k = alignment(name)
    return Reference(X, BY_NAME[name].q, *exact_freqs(X, BY_NAME[name].q, k))


def ulps(a, b):
    """|a - b| in units of the spacing of b."""
    return np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(b))
