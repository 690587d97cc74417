"""numpy float64 reference of the principal-component entries (dca_pca_fit, dca_pca_project; include/dca_hip.h): the one-hot
covariance exactly as the contract defines it, its eigen-decomposition by LAPACK, and the projection in the contract's order."""
import numpy as np


def one_hot(X, q):
    X = np.asarray(X)
    N, L = X.shape
    H = np.zeros((N, L * q), dtype=np.float64)
    H[np.arange(N)[:, None], np.arange(L)[None, :] * q + X] = 1.0
    return H


def frequencies(X, w, q):
    """f(i,a) = sum_n w_n [s_ni = a] / Meff -> float64[L*q]"""
    w = np.asarray(w, dtype=np.float64)
    return (w[:, None] * one_hot(X, q)).sum(axis=0) / w.sum()


def covariance(X, w, q):
    """C = sum_n w_n (x_n - f)(x_n - f)^T / Meff -> (C float64[Lq, Lq], f float64[Lq])"""
    w = np.asarray(w, dtype=np.float64)
    f = frequencies(X, w, q)
    D = one_hot(X, q) - f[None, :]
    C = (D * w[:, None]).T @ D / w.sum()
    return 0.5 * (C + C.T), f


def sign_rule(v):
    """the entry of largest magnitude positive, ties to the smallest index"""
    v = np.array(v, dtype=np.float64)
    at = int(np.argmax(np.abs(v)))            # argmax returns the first of equal values
    return -v if v[at] < 0 else v


def eigh(X, w, q):
    """-> (eigenvalues descending float64[Lq], eigenvectors float64[Lq, Lq] (row m = v_m, sign rule applied), C, f)"""
    C, f = covariance(X, w, q)
    lam, U = np.linalg.eigh(C)
    lam, U = lam[::-1].copy(), U[:, ::-1].T.copy()
    for m in range(U.shape[0]):
        U[m] = sign_rule(U[m])
    return lam, U, C, f


def project(X, components, offsets):
    """p_m(s) = (sum over the sites ascending of v_m(i, s_i)) - c_m, one double chain per (sequence, component), then one
    subtraction.  components: float64[k, L, q] (or [k, L*q]); -> float64[n, k]"""
    X = np.asarray(X)
    n, L = X.shape
    k = len(offsets)
    v = np.asarray(components, dtype=np.float64).reshape(k, L, -1)
    out = np.zeros((n, k), dtype=np.float64)
    for m in range(k):
        s = np.zeros(n, dtype=np.float64)
        for i in range(L):
            s = s + v[m, i, X[:, i]]
        out[:, m] = s - offsets[m]
    return out


def gaps(lam):
    """distance of every eigenvalue to its nearest neighbour in the spectrum"""
    lam = np.asarray(lam, dtype=np.float64)
    d = np.abs(np.diff(lam))
    g = np.full(lam.size, np.inf)
    if lam.size > 1:
        g[:-1] = d
        g[1:] = np.minimum(g[1:], d)
    return g


def planted_alignment(q, L, N, k, seed):
    """A synthetic alignment with planted modes: independent columns drawn from Dirichlet(0.4) profiles; then for mode
    m = 0 .. min(k, 4) - 1 a random subset of about N / (2 (m + 1)) rows gets max(1, L // (2 + m)) random sites overwritten
    with one fixed state each.  -> uint8[N, L]"""
    rng = np.random.default_rng(seed)
    X = np.empty((N, L), dtype=np.uint8)
    for i in range(L):
        X[:, i] = rng.choice(q, size=N, p=rng.dirichlet(np.full(q, 0.4)))
    for m in range(min(k, 4)):
        rows = rng.choice(N, size=max(1, N // (2 * (m + 1))), replace=False)
        sites = rng.choice(L, size=max(1, L // (2 + m)), replace=False)
        X[np.ix_(rows, sites)] = rng.integers(0, q, size=sites.size, dtype=np.uint8)[None, :]
    return X
