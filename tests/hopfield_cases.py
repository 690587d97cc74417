"""The inputs of tests/test_hopfield.py (GPU) and of the input conditions tests/test_hopfield_host.py checks on the CPU: synthetic
alignments with planted modes at every shape class of the fit, under the weights of compute_weights(0.8) and under random
weights, with the selection each case asks for, and the bounds of DESIGN.md section 31 derived from the reference."""
import functools

import numpy as np

from oracle import mf as omf
import hopfield_reference as href
import pca_reference

THETA = 0.5
TOL = 1e-10
U = 2.0 ** -53

# (L, q, N): n = L (q - 1) = 8 (below the block), 60 and 32 (at most 64), 140, 260 and 132 (off every tile multiple)
SHAPES = {"n8": (2, 5, 120), "n60": (3, 21, 200), "n32": (8, 5, 200), "n140": (7, 21, 300), "n260": (13, 21, 300), "n132": (33, 5, 300)}
# selection: ("explicit", a, r) or ("likelihood", p).  n32 asks for a block that is the whole space at the attractive end.
SELECTION = {"n8": ("explicit", 2, 2), "n60": ("likelihood", 6), "n32": ("explicit", 24, 8), "n140": ("explicit", 4, 4),
             "n260": ("likelihood", 8), "n132": ("explicit", 3, 5)}
CASES = [(shape, weights) for shape in SHAPES for weights in ("seqid", "random")]
# the identity with mfDCA: the whole spectrum as explicit splits (a, n - a).  At least one end's block is the whole space or close
# to it: a split through the middle of the spectrum, such as (30, 30) at n = 60, asks either end for eigenvalues from the bulk
# around 1, where the convergence factor lambda_(b+1) / lambda_k of subspace iteration is 0.99 and above (neither end converges
# in 1000 iterations there, and the fit says so).
IDENTITY = [("n60", 4), ("n60", 10), ("n60", 56), ("n32", 0), ("n32", 8), ("n32", 32)]


@functools.lru_cache(maxsize=None)
def inputs(shape, weights):
    """-> (X uint8[N, L] device codes, w float64[N], q)"""
    L, q, N = SHAPES[shape]
    X = pca_reference.planted_alignment(q, L, N, 3, 11 + L)
    if weights == "seqid":
        w = omf.compute_sequences_weight(X.astype(np.int32) + 1, 0.8)
    else:
        w = np.random.default_rng(100 + L).uniform(0.05, 1.0, N)
    return X, w, q


@functools.lru_cache(maxsize=None)
def reference(shape, weights):
    """The reference of one case, computed once and shared: dict with C, fi, lam (descending), U, G, T, eps (eigenvalue scale,
    margin applied), L, q, n."""
    X, w, q = inputs(shape, weights)
    L = X.shape[1]
    C, fi = href.corr_mat(X, w, q, THETA)
    lam, Um, G, T = href.spectrum(C, L, q - 1)
    eps = href.epsilon(C, L, q - 1)
    for a in (C, fi, lam, Um, G, T):
        a.setflags(write=False)
    return {"C": C, "fi": fi, "lam": lam, "U": Um, "G": G, "T": T, "eps": href.MARGIN * eps["eigenvalues"], "L": L, "q": q,
            "n": L * (q - 1), "X": X, "w": w}


def split(shape, weights):
    """(a, r) of the case: the explicit split, or the reference's for a likelihood selection"""
    sel = SELECTION[shape]
    if sel[0] == "explicit":
        return sel[1], sel[2]
    return href.select_likelihood(reference(shape, weights)["lam"], sel[1])


def residual_bound(ref, lam_mu):
    """What a converged fit may report for a pattern: tol lambda_1 at the attractive end; the repulsive end converges on the
    inverse, ||Gamma^-1 v - v / lambda|| <= tol / lambda_min, and Gamma v - lambda v = -lambda Gamma (Gamma^-1 v - v / lambda)."""
    lam = ref["lam"]
    return TOL * lam[0] * max(1.0, lam_mu / lam[-1])


def eigenvalue_gaps(ref):
    return pca_reference.gaps(ref["lam"])


def compared_patterns(ref, idx):
    """the selected patterns whose gap to the rest of the spectrum is at least 0.01 (lambda_max - lambda_min)"""
    lam, g = ref["lam"], eigenvalue_gaps(ref)
    return [k for k, m in enumerate(idx) if g[m] >= 0.01 * (lam[0] - lam[-1])]


def coupling_bound(ref, idx, residuals, eps_couplings):
    """Elementwise bound on J of the selected set idx.  In the whitened basis M = sum_S c(lambda) v v^T with c = 1 - 1 / lambda.
    With rho = (sum r_mu^2)^1/2 and delta the distance of the selected eigenvalues to the unselected ones, the computed subspace is
    within sin Theta <= rho / delta of the true one (Davis-Kahan), which moves M by at most 2 max|c| rho / delta; inside the
    subspace a rotation between two selected patterns by r / |lambda_mu - lambda_nu| changes M by (c_mu - c_nu) times that, at
    most max|c'| rho, and the eigenvalue errors by max|c'| rho again, c' = 1 / lambda^2.  J = T M T^T, so
    |dJ_ab| <= |T_a| |T_b| 2 rho (max|c| / delta + max|c'|) + the reference's own rounding."""
    lam, T, n = ref["lam"], ref["T"], ref["n"]
    sel = np.zeros(n, dtype=bool)
    sel[idx] = True
    rho = float(np.sqrt((np.asarray(residuals) ** 2).sum()))
    cmax = float(np.abs(1.0 - 1.0 / lam[sel]).max())
    dmax = float((1.0 / lam[sel] ** 2).max())
    term = dmax
    if (~sel).any():
        delta = float(np.abs(lam[sel][:, None] - lam[~sel][None, :]).min())
        term += cmax / delta
    t = np.linalg.norm(T, axis=1)
    return np.outer(t, t) * (2.0 * rho * term) + href.MARGIN * eps_couplings
