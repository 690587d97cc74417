"""Restatement of the greedy ascent (dca_plm_ascend, dca_mf_ascend) in numpy float64, literally in the order
of the specification, the np.longdouble path that forms the table afresh at every step, the margin of a path and the models
shared by tests/test_ascent_host.py (CPU) and tests/test_ascent.py (GPU).

A model is (h, Jp): h float64[L, q], Jp float64[pairs, q, q] with Jp[p][a, b] = J_ij(a, b) for the p-th pair i < j in pair order.

    1. table   U_i(a) = h_i(a) + sum over j != i, ascending j, of J_ij(a, s_j): one sequential double sum, h first
    2. step t  g(i, a) = U_i(a) - U_i(s_i), free i, a != s_i; the largest g, ties to the smallest i, then the smallest a;
               applied if g > min_gain and t < max_steps
    3. apply   s_i* <- a*; U_j(b) += (J_{j i*}(b, a*) - J_{j i*}(b, old)) for every free j != i* (difference first); U_i* unchanged
    4. outputs codes, steps, converged, gain (the sequential sum of the applied g), path and path gains

MARGIN RULE.  The float64 path equals the exact greedy path when no decision is closer than the error of the table: the margin of
a path (the smallest of best g - second-best g and best g - min_gain at the applied steps, and of |min_gain - best g| at the stop,
all in longdouble on fresh tables) must be at least MARGIN_FACTOR = 1e3 times the largest |U_incremental - U_fresh| met along the
path.  A property of the inputs alone; a seed that violates it is changed, never the factor."""
import os

import numpy as np

LD = np.longdouble
MARGIN_FACTOR = 1e3
FAULTS = ("untransposed", "tie_reversed", "update_self", "stale_current", "clamped_moves", "ge_min_gain")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def full_table(Jp, L, q, fault=None):
    """J[i, j, a, b] = J_ij(a, b) for every ordered pair (zero for i == j): the stored block for i < j, its transpose for i > j.
    fault 'untransposed': the stored block as it lies for i > j too."""
    J = np.zeros((L, L, q, q))
    iu, ju = np.triu_indices(L, 1)
    blocks = np.asarray(Jp[np.arange(iu.size)], dtype=np.float64) if iu.size else np.zeros((0, q, q))
    J[iu, ju] = blocks
    J[ju, iu] = blocks if fault == "untransposed" else blocks.transpose(0, 2, 1)
    return J


def fresh_table(h, J, s, dtype=np.float64):
    """step 1 for every site (the free ones are read from it): a sequential sum in `dtype`, h first, then j ascending"""
    L, q = h.shape
    U = h.astype(dtype).copy()
    rows = np.arange(L)
    for j in range(L):
        keep = rows != j
        U[keep] += J[keep, j, :, int(s[j])].astype(dtype)
    return U


def fresh_table_ld(hl, J_ld, s):
    """the table in longdouble, every site at once (J[i, i] is zero; the order of a longdouble sum is not part of any claim)"""
    L = hl.shape[0]
    return hl + J_ld[np.arange(L)[:, None], np.arange(L)[None, :], :, np.asarray(s)[None, :]].sum(axis=1)


def best_move(U, s, free, tie_reversed=False):
    """step 2 -> (g, i, a, second-best g) over the free sites; (-inf, -1, -1, -inf) without a candidate"""
    if free.size == 0:
        return -np.inf, -1, -1, -np.inf
    q = U.shape[1]
    g = U[free] - U[free, s[free]][:, None]
    g[np.arange(free.size), s[free]] = -np.inf
    flat = g.reshape(-1)
    if tie_reversed:
        k = flat.size - 1 - int(np.argmax(flat[::-1]))
    else:
        k = int(np.argmax(flat))                      # the first occurrence: the smallest site, then the smallest state
    best = flat[k]
    rest = np.delete(flat, k)
    second = rest.max() if rest.size else -np.inf
    return best, int(free[k // q]), k % q, second


class Ascent:
    """codes, steps, converged, gain, path [(site, state)], gains [g] of one chain"""


def ascend_one(h, J, x, free, max_steps, min_gain, fault=None, drift_against=None):
    """Steps 1-4 for one chain in float64.  fault: one of FAULTS (negative controls).  drift_against: the longdouble J table;
    then .drift is the largest |U_incremental - U_fresh| over the free rows at every decision."""
    L, q = h.shape
    s = np.array(x, dtype=np.int64)
    free = np.asarray(free, dtype=np.int64)
    movable = np.arange(L) if fault == "clamped_moves" else free
    U = fresh_table(h, J, s)
    r = Ascent()
    r.path, r.gains, r.gain, r.drift = [], [], 0.0, 0.0
    t = 0
    while True:
        if drift_against is not None and free.size:
            r.drift = max(r.drift, float(np.abs(U[free].astype(LD) - fresh_table_ld(h.astype(LD), drift_against, s)[free]).max()))
        g, i, a, _ = best_move(U, s, movable, tie_reversed=fault == "tie_reversed")
        ok = g >= min_gain if fault == "ge_min_gain" else g > min_gain
        if not ok:
            r.converged = 1
            break
        if t >= max_steps:
            r.converged = 0
            break
        old = int(s[i])
        s[i] = a
        delta = J[:, i, :, a] - J[:, i, :, old]                      # the difference first
        rows = np.arange(L) != i
        if fault == "update_self":
            rows[:] = True
            delta = delta.copy()
            delta[i] = J[(i + 1) % L, i, :, a] - J[(i + 1) % L, i, :, old]
        if fault == "stale_current":                                 # U_j(s_j) of before the update joins the updated U_j(a)
            stale = U[np.arange(L), s].copy()
            U[rows] += delta[rows]
            keep = np.arange(L) != i
            U[np.arange(L)[keep], s[keep]] = stale[keep]
        else:
            U[rows] += delta[rows]
        r.path.append((i, a))
        r.gains.append(float(g))
        r.gain += float(g)
        t += 1
    r.codes = s.astype(np.uint8)
    r.steps = t
    return r


def fresh_path(h, J_ld, x, free, max_steps, min_gain):
    """The greedy path on tables formed afresh from the model at every step, in longdouble -> (path, converged, margin)"""
    s = np.array(x, dtype=np.int64)
    free = np.asarray(free, dtype=np.int64)
    hl = h.astype(LD)
    path, margin = [], np.inf
    t = 0
    while True:
        g, i, a, second = best_move(fresh_table_ld(hl, J_ld, s), s, free)
        if not g > min_gain:
            return path, 1, min(margin, float(LD(min_gain) - g))
        if t >= max_steps:
            return path, 0, min(margin, float(g - LD(min_gain)))
        margin = min(margin, float(g - second), float(g - LD(min_gain)))
        s[i] = a
        path.append((i, a))
        t += 1


def margin(h, Jp, x, free, max_steps, min_gain=0.0):
    """the margin of one chain's path: the smallest of (best g - second-best g) and (best g - min_gain) at the applied steps and
    of |min_gain - best g| at the stop, in longdouble on fresh tables"""
    L, q = h.shape
    return fresh_path(h, full_table(Jp, L, q).astype(LD), x, free, max_steps, min_gain)[2]


def ascend(h, Jp, X, free, max_steps, min_gain=0.0, fault=None):
    """The restatement for every row of X -> dict of arrays in the entry's layout (path -1 / -1 / 0.0 past steps)"""
    L, q = h.shape
    X = np.asarray(X, dtype=np.uint8).reshape(-1, L)
    n = X.shape[0]
    J = full_table(Jp, L, q, fault)
    out = {"codes": np.zeros((n, L), np.uint8), "steps": np.zeros(n, np.int32), "converged": np.zeros(n, bool),
           "gains": np.zeros(n), "path": np.full((n, max_steps, 2), -1, np.int32), "path_gains": np.zeros((n, max_steps))}
    for k in range(n):
        r = ascend_one(h, J, X[k], free, max_steps, min_gain, fault)
        out["codes"][k], out["steps"][k], out["converged"][k], out["gains"][k] = r.codes, r.steps, r.converged, r.gain
        if r.steps:
            out["path"][k, :r.steps] = r.path
            out["path_gains"][k, :r.steps] = r.gains
    return out


def check_margins(h, Jp, X, free, max_steps, min_gain=0.0):
    """The float64 restatement against the fresh longdouble path for every row of X -> (smallest margin, largest drift); asserts
    the same path and the margin rule."""
    L, q = h.shape
    J = full_table(Jp, L, q)
    J_ld = J.astype(LD)
    margin, drift = np.inf, 0.0
    for x in np.asarray(X).reshape(-1, L):
        r = ascend_one(h, J, x, free, max_steps, min_gain, drift_against=J_ld)
        path, conv, m = fresh_path(h, J_ld, x, free, max_steps, min_gain)
        assert r.path == path and r.converged == conv, "the float64 path leaves the fresh longdouble path"
        margin, drift = min(margin, m), max(drift, r.drift)
    assert margin >= MARGIN_FACTOR * drift, "margin %.3g is below %g x drift %.3g: change the seed" % (margin, MARGIN_FACTOR, drift)
    return margin, drift


# ----------------------------------------------------------------------------- the models of both test files
PLM_SHAPES = [(5, 23), (21, 37)]                                    # (q, L), each in float32 and float64
MF_SHAPES = [(2, 2), (2, 9), (8, 6), (9, 6), (24, 6), (25, 6), (32, 6)]
MF_GOLDENS = ("mf_toy_protein", "mf_toy_rna")
MF_N = 200


def plm_model(x, L, q):
    x = np.asarray(x, dtype=np.float64)
    return x[:L * q].reshape(L, q), x[L * q:].reshape(-1, q, q)


def plm_x(q, L, bits, sigma=0.5):
    """the stored parameter vector of a plm case in its element type"""
    dt = np.float32 if bits == 32 else np.float64
    P = L * q + L * (L - 1) // 2 * q * q
    return (np.random.default_rng([24, q, L, bits]).standard_normal(P) * sigma).astype(dt)


def plm_alignment(q, L, N=40):
    return np.random.default_rng([25, q, L]).integers(0, q, size=(N, L), dtype=np.uint8)


def mf_alignment(q, L):
    """Random columns, each with its own state frequencies, and dyadic weights (reweighting by identity would flatten L = 2 to a
    model of zeros).  The first q rows of a column are a permutation of the states: a state that a column never shows has the
    pseudocount's frequency alone, and two such states tie to the last bit.  -> (X uint8[N, L], w float64[N])"""
    rng = np.random.default_rng([26, q, L])
    X = np.stack([np.concatenate([rng.permutation(q), rng.choice(q, size=MF_N - q, p=rng.dirichlet(np.ones(q)))]).astype(np.uint8)
                  for _ in range(L)], axis=1)
    return X, rng.integers(1, 9, MF_N) / 8.0


def golden_alignment(tag):
    G = np.load(os.path.join(ROOT, "tests", "golden", tag + ".npz"))
    return (G["X"] - 1).astype(np.uint8), int(G["q"])


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


def mf_model_cpu(X, q, w=None, theta=0.5, seqid=0.8):
    """the oracle's float64 mf model of an alignment with the weights w (None: reweighted at seqid), the CPU stand-in for
    mf_couplings() / mf_fields()"""
    from oracle import mf as omf
    L = X.shape[1]
    X1 = X.astype(np.int64) + 1
    if w is None:
        w = omf.compute_sequences_weight(X1, seqid)
    fi = omf.get_reg_single_site_freqs(omf.compute_single_site_freqs(X1, q, w), L, q, theta)
    fij = omf.get_reg_pair_site_freqs(omf.compute_pair_site_freqs(X1, q, w), L, q, theta)
    J = omf.compute_couplings(omf.construct_corr_mat(fi, fij, L, q))
    return mf_model(J, omf.compute_fields(J, fi, L, q), L, q)


def starts(n, L, q, seed):
    """a different row per chain"""
    return np.random.default_rng([27, seed, n, L, q]).integers(0, q, size=(n, L), dtype=np.uint8)


def golden_starts(X, n):
    """rows of the alignment itself: states a column never shows have the pseudocount's frequency alone, so their fields tie to
    the last bit and a random start would let rounding pick among them"""
    return X[(3 * np.arange(n)) % X.shape[0]]


def site_lists(L):
    """F = L, 1, 2 and 0; free sites at 0 and L - 1; one clamped site"""
    lists = [np.arange(L), np.array([0]), np.array([L - 1]), np.array([0, L - 1]), np.array([], dtype=np.int64)]
    if L > 2:
        lists.append(np.setdiff1d(np.arange(L), [L // 2]))
    return [np.asarray(v, dtype=np.int64) for v in lists]


# every model of the two test files: ("plm", q, L, bits) | ("mf", q, L) | ("golden", tag)
MODELS = [("plm", q, L, bits) for q, L in PLM_SHAPES for bits in (32, 64)] + [("mf", q, L) for q, L in MF_SHAPES] + \
    [("golden", tag) for tag in MF_GOLDENS]
N_CHAINS = 65


def model_id(m):
    return "_".join(str(v) for v in m)


def cpu_model(m):
    """(h, Jp, starts uint8[N_CHAINS, L]) of a model on the CPU: a plm model is its stored vector; an mf model is the oracle's
    (the GPU file reads the device's own and checks the margin rule on that)"""
    if m[0] == "plm":
        _, q, L, bits = m
        h, Jp = plm_model(plm_x(q, L, bits), L, q)
        return h, Jp, starts(N_CHAINS, L, q, 0)
    if m[0] == "mf":
        _, q, L = m
        X, w = mf_alignment(q, L)
        h, Jp = mf_model_cpu(X, q, w)
        return h, Jp, starts(N_CHAINS, L, q, 0)
    X, q = golden_alignment(m[1])
    h, Jp = mf_model_cpu(X, q)
    return h, Jp, golden_starts(X, N_CHAINS)
