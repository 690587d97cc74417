"""numpy float64 reference of the Hopfield-Potts entries (dca_mf_hopfield_fit, dca_hopfield_project; include/dca_hip.h, DESIGN.md
section 31): the correlation matrix of oracle/mf.py, the per-site Cholesky whitening, numpy.linalg.eigh, the selection rule, the
couplings, the fields and the overlaps in the contract's order.  A second formulation (whitening by the symmetric square root of
every diagonal block) measures the rounding of the reference itself: epsilon() is the largest difference between the two."""
import numpy as np

from oracle import mf as omf
import pca_reference

MARGIN = 8.0            # on the measured rounding of the reference


def corr_mat(X0, w, q, theta):
    """X0: uint8[N, L] codes, gap = q - 1 -> (C float64[n, n], regularised site frequencies float64[L, q])"""
    X = np.asarray(X0).astype(np.int32) + 1
    L = X.shape[1]
    w = np.asarray(w, dtype=np.float64)
    fi = omf.get_reg_single_site_freqs(omf.compute_single_site_freqs(X, q, w), L, q, theta)
    fij = omf.get_reg_pair_site_freqs(omf.compute_pair_site_freqs(X, q, w), L, q, theta)
    return omf.construct_corr_mat(fi, fij, L, q), fi


def blocks(C, L, qm):
    return [C[i * qm:(i + 1) * qm, i * qm:(i + 1) * qm] for i in range(L)]


def block_diag(mats):
    qm = mats[0].shape[0]
    out = np.zeros((len(mats) * qm, len(mats) * qm))
    for i, m in enumerate(mats):
        out[i * qm:(i + 1) * qm, i * qm:(i + 1) * qm] = m
    return out


def whiten_cholesky(C, L, qm):
    """-> (Gamma = R^-1 C R^-T, T = blockdiag(R^-T): u = T v)"""
    Rinv = [np.linalg.inv(np.linalg.cholesky(D)) for D in blocks(C, L, qm)]
    W = block_diag(Rinv)
    G = W @ C @ W.T
    return 0.5 * (G + G.T), W.T


def whiten_sqrt(C, L, qm):
    """the same with the symmetric inverse square root of every block in the place of R^-1"""
    S = []
    for D in blocks(C, L, qm):
        lam, Q = np.linalg.eigh(D)
        S.append((Q / np.sqrt(lam)) @ Q.T)
    W = block_diag(S)
    G = W @ C @ W
    return 0.5 * (G + G.T), W


def decompose(C, L, qm, whiten=whiten_cholesky):
    """-> (lambda descending float64[n], U float64[n, n]: column mu = u_mu with u^T D u = 1 and the sign rule, Gamma, T, V: the
    eigenvectors of Gamma as LAPACK returns them, in the same order)"""
    G, T = whiten(C, L, qm)
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1].copy(), V[:, ::-1].copy()
    U = T @ V
    at = np.argmax(np.abs(U), axis=0)                   # the sign rule: argmax returns the first of equal values
    U = U * np.where(U[at, np.arange(U.shape[1])] < 0, -1.0, 1.0)[None, :]
    return lam, U, G, T, V


def spectrum(C, L, qm, whiten=whiten_cholesky):
    return decompose(C, L, qm, whiten)[:4]


def gain(lam):
    lam = np.asarray(lam, dtype=np.float64)
    return 0.5 * (lam - 1.0 - np.log(lam))


def select_likelihood(lam_desc, p):
    """The p patterns of largest gain of a descending spectrum -> (p_plus, p_minus): that many of the largest and of the smallest
    eigenvalues.  Equal gains go to the attractive side."""
    lam = np.asarray(lam_desc, dtype=np.float64)
    g = gain(lam)
    i, j = 0, 0
    while i + j < p:
        if g[i] >= g[lam.size - 1 - j]:
            i += 1
        else:
            j += 1
    return i, j


def selected(n, a, r):
    """indices into the descending spectrum in the order of the outputs: the a largest descending, then the r smallest ascending"""
    return list(range(a)) + [n - 1 - j for j in range(r)]


def couplings(lam, U, idx):
    """J = sum over idx of (1 - 1 / lambda) u u^T (the diagonal blocks included, as the sum gives them)"""
    Us = U[:, idx]
    return (Us * (1.0 - 1.0 / lam[idx])) @ Us.T


def patterns(lam, U, idx):
    """-> (xi float64[p, n], signs int[p]) with J = sum s xi xi^T"""
    c = 1.0 - 1.0 / lam[idx]
    return (U[:, idx] * np.sqrt(np.abs(c))).T.copy(), np.where(c < 0, -1, 1)


def off_diagonal_mask(L, qm):
    m = np.ones((L * qm, L * qm), dtype=bool)
    for i in range(L):
        m[i * qm:(i + 1) * qm, i * qm:(i + 1) * qm] = False
    return m


def fields(J, reg_fi, L, q):
    return omf.compute_fields(J, reg_fi, L, q)


def overlaps(X0, xi, L, q):
    """x_mu(s) = sum over the sites ascending of xi_mu(i, s_i), a gap adding 0: one chain of doubles -> float64[n, p]"""
    X0 = np.asarray(X0)
    p = xi.shape[0]
    full = np.zeros((p, L, q))
    full[:, :, :q - 1] = np.asarray(xi).reshape(p, L, q - 1)
    return pca_reference.project(X0, full, np.zeros(p))


def energies(X0, J, h, L, q):
    """E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j), zero on the gap state"""
    qm = q - 1
    J4 = J.reshape(L, qm, L, qm)
    out = np.zeros(len(X0))
    for k, s in enumerate(np.asarray(X0)):
        e = 0.0
        for i in range(L):
            if s[i] == qm:
                continue
            e += h[i, s[i]]
            for j in range(i + 1, L):
                if s[j] != qm:
                    e += J4[i, s[i], j, s[j]]
        out[k] = e
    return out


def epsilon(C, L, qm, idx=None, third=True, first=None, second=None):
    """The rounding of the reference: the largest difference between the Cholesky-whitened and the square-root-whitened
    formulation -> dict(eigenvalues, couplings); couplings over the patterns idx (default: the whole spectrum), off the diagonal
    blocks.  third: the eigenvalues of the unsymmetric D^-1 C as well (O(n^3) with a large constant: left out at n in the
    thousands).  first / second: the two decompositions, where the caller has them already."""
    lam1, U1, G1, _, V1 = first if first is not None else decompose(C, L, qm, whiten_cholesky)
    lam2, U2, G2, _, V2 = second if second is not None else decompose(C, L, qm, whiten_sqrt)
    eig = float(np.abs(lam1 - lam2).max())
    if third:
        lam3 = np.sort(np.linalg.eigvals(np.linalg.solve(block_diag(blocks(C, L, qm)), C)).real)[::-1]
        eig = max(eig, float(np.abs(lam1 - lam3).max()))
    for G, V, lam in ((G1, V1, lam1), (G2, V2, lam2)):          # the residuals LAPACK leaves on the reference's own eigenpairs
        eig = max(eig, float(np.linalg.norm(G @ V - V * lam, axis=0).max()))
    idx = list(range(lam1.size)) if idx is None else idx
    mask = off_diagonal_mask(L, qm)
    return {"eigenvalues": eig, "couplings": float(np.abs(couplings(lam1, U1, idx) - couplings(lam2, U2, idx))[mask].max())}


def d_norm(x, C, L, qm):
    D = block_diag(blocks(C, L, qm))
    return float(np.sqrt(x @ D @ x))
