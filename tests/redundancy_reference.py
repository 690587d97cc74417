"""TEST INFRASTRUCTURE ONLY: numpy reference of the redundancy filter and the identity clusters and the
seeded fixtures of tests/test_redundancy_host.py and tests/test_redundancy.py.  Everything is integer, so every comparison
with the device is array_equal.

ident(m, n) = #{i : X_mi = X_ni} (the gap state counts like any other); similar iff ident >= T."""
import numpy as np

MAX_ROWS = 3000


def identity_matrix(X):
    """int32[n, n] of identical-site counts, n <= MAX_ROWS"""
    X = np.asarray(X, dtype=np.uint8)
    n, L = X.shape
    assert n <= MAX_ROWS
    ident = np.zeros((n, n), dtype=np.int32)
    for i in range(L):
        c = X[:, i]
        ident += c[:, None] == c[None, :]
    return ident


def threshold(L, identity, strict=False):
    """The smallest k in 0..L with k / L >= identity (strict: > identity) in float64; L + 1 if none"""
    for k in range(L + 1):
        v = np.float64(k) / np.float64(L)
        if (v > identity) if strict else (v >= identity):
            return k
    return L + 1


def greedy_filter(ident, T, order=None):
    """The sequential definition -> (keep uint8[n], rep int32[n])"""
    n = ident.shape[0]
    order = np.arange(n) if order is None else np.asarray(order)
    keep = np.zeros(n, dtype=np.uint8)
    rep = np.zeros(n, dtype=np.int32)
    kept = []                                  # in the order they were kept = ascending rank
    for r in order:
        rep[r] = r
        for k in kept:
            if ident[r, k] >= T:
                rep[r] = k
                break
        else:
            keep[r] = 1
            kept.append(int(r))
    return keep, rep


def greedy_filter_rescan(ident, T, order=None):
    """Brute force, from the definition's words alone: for every row, scan ALL earlier rows of the order again"""
    n = ident.shape[0]
    order = list(range(n)) if order is None else [int(v) for v in order]
    keep = np.zeros(n, dtype=np.uint8)
    rep = np.zeros(n, dtype=np.int32)
    for p, r in enumerate(order):
        first = [m for m in order[:p] if keep[m] and ident[r, m] >= T]
        keep[r] = 0 if first else 1
        rep[r] = first[0] if first else r
    return keep, rep


def components(ident, T):
    """Union-find over the similar pairs -> int32[n] labels, the smallest row index of each component"""
    n = ident.shape[0]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    ii, jj = np.nonzero(np.triu(ident >= T, 1))
    for a, b in zip(ii.tolist(), jj.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int32)


def components_closure(ident, T):
    """The same by repeated boolean matrix closure (reachability), independent of union-find"""
    n = ident.shape[0]
    R = (ident >= T) | np.eye(n, dtype=bool)
    while True:
        R2 = (R.astype(np.int32) @ R.astype(np.int32)) > 0
        if np.array_equal(R2, R):
            break
        R = R2
    return np.argmax(R, axis=1).astype(np.int32)        # the first reachable index = the smallest


def degrees(ident, T):
    return (ident >= T).sum(axis=1).astype(np.int32)


def gap_order(X, q):
    """'fewest_gaps': gap count (state q - 1) ascending, then row index"""
    gaps = (np.asarray(X) == q - 1).sum(axis=1)
    return np.lexsort((np.arange(len(gaps)), gaps)).astype(np.int32)


# ---------------------------------------------------------------- fixtures (all seeded)
def mutate(rng, row, q, sites):
    out = row.copy()
    for s in sites:
        out[s] = (int(out[s]) + 1 + int(rng.integers(q - 1))) % q
    return out


def fixture_T(L):
    """The threshold the family fixture is built around: d = L // 8 mutations keep a descendant at exactly T = L - d"""
    return L - L // 8


FAMILY_MEMBERS = 7


def families(n, L, q, seed):
    """A = max(1, n // 7) ancestors a and, per family, in this file order (member-major: the members of a family lie A rows
    apart, so that they spread over the filter's blocks):
      b = a with d sites mutated (P1)                      ident(a, b) = T exactly
      c = b with d other sites mutated (P2)                ident(b, c) = T, ident(a, c) = L - 2 d < T: a chain a - b - c
      r = b with half of P2 set to c's states              similar to b and c, not to a (d >= 2): its first similar row in file
                                                           order, b, is removed; its representative is c
      e = a with d random sites mutated                    ident = T exactly
      f = a with d + 1 random sites mutated                ident = T - 1: not similar to a
      g = a                                                an exact duplicate
    rows past 7 A are uniform random.  -> (X uint8[n, L], T)"""
    rng = np.random.default_rng(seed)
    d = L // 8
    T = fixture_T(L)
    A = max(1, n // FAMILY_MEMBERS)
    X = rng.integers(0, q, size=(n, L), dtype=np.uint8)
    for fam in range(A):
        a = X[fam].copy() if fam < n else rng.integers(0, q, size=L, dtype=np.uint8)
        perm = rng.permutation(L)
        P1, P2 = perm[:d], perm[d:2 * d]
        b = mutate(rng, a, q, P1)
        c = mutate(rng, b, q, P2)
        r = b.copy()
        h = P2[:d // 2]
        r[h] = c[h]
        e = mutate(rng, a, q, rng.permutation(L)[:d])
        f = mutate(rng, a, q, rng.permutation(L)[:min(L, d + 1)])
        for m, row in enumerate((a, b, c, r, e, f, a)):
            k = m * A + fam
            if k < n:
                X[k] = row
    return X, T


def path(n, L, q, T, seed, shuffled=False):
    """s_0 .. s_{n-1}: consecutive rows share exactly T sites (L - T sites mutated per step, on a window that rotates over the
    sites), every other pair fewer than T -- one component of diameter n - 1.  shuffled: the row order permuted (the label is
    still the smallest index).  The builder checks the property itself."""
    rng = np.random.default_rng(seed)
    d = L - T
    assert 1 <= d and 2 * d <= L
    rows = [rng.integers(0, q, size=L, dtype=np.uint8)]
    for k in range(1, n):
        sites = [(k * d + t) % L for t in range(d)]
        rows.append(mutate(rng, rows[-1], q, sites))
    X = np.array(rows, dtype=np.uint8)
    sim = identity_matrix(X) >= T
    want = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]) <= 1
    assert np.array_equal(sim, want), "path fixture: a pair that is not consecutive is similar"
    assert all(int((X[k] == X[k + 1]).sum()) == T for k in range(n - 1))
    if shuffled:
        X = X[rng.permutation(n)]
    return X


def duplicates(n, L, q, seed, copies=3):
    """ceil(n / copies) distinct uniform rows, each `copies` times, in shuffled order"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, q, size=((n + copies - 1) // copies, L), dtype=np.uint8)
    X = np.repeat(base, copies, axis=0)[:n]
    return X[rng.permutation(n)]


def isolated(n, L, q, seed):
    return np.random.default_rng(seed).integers(0, q, size=(n, L), dtype=np.uint8)


def fixture_conditions(X, T, order=None):
    """What a GPU case must offer so that it cannot pass vacuously -> dict of booleans / figures"""
    ident = identity_matrix(X)
    n = ident.shape[0]
    keep, rep = greedy_filter(ident, T, order)
    lab = components(ident, T)
    off = ~np.eye(n, dtype=bool)
    sim = ident >= T
    chain = False
    for root in np.unique(lab):
        idx = np.nonzero(lab == root)[0]
        if idx.size >= 3 and not sim[np.ix_(idx, idx)].all():
            chain = True
            break
    # a removed row whose representative is not its first similar row in file order
    late = False
    for r in np.nonzero(keep == 0)[0]:
        first = np.nonzero(sim[r] & off[r])[0]
        if first.size and first[0] != rep[r]:
            late = True
            break
    return dict(kept_fraction=float(keep.sum()) / n, at_T=bool(((ident == T) & off).any()), below_T=bool(((ident == T - 1) & off).any()),
                chain=chain, late_representative=late)
