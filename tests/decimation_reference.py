"""numpy restatements for the sparse-bmDCA entries (dca_plm_bm_decimate, the masked update, dca_plm_zero_sum_gauge), in the
operation orders include/dca_hip.h states.  No GPU needed."""
import numpy as np


def pairs_of(L):
    return np.triu_indices(L, 1)


# ---------------------------------------------------------------- score
def score(J, p, dtype=np.float64):
    """D of every element in `dtype` (float64: the header's operation order; longdouble: the reference it is judged by)"""
    J = np.asarray(J, dtype=dtype)
    p = np.asarray(p, dtype=dtype)
    one = dtype(1)
    D = np.zeros(np.broadcast(J, p).shape, dtype=dtype)
    J, p = np.broadcast_to(J, D.shape), np.broadcast_to(p, D.shape)
    live = (p != 0) & (p != 1) & (J != 0)
    pos, neg = live & (J > 0), live & (J < 0)
    with np.errstate(over="ignore", under="ignore"):
        e = np.expm1(-J[pos])
        D[pos] = ((J[pos] * (-e)) * (p[pos] * (one - p[pos]))) / (one + p[pos] * e)
        e = np.expm1(J[neg])
        D[neg] = ((J[neg] * e) * (p[neg] * (one - p[neg]))) / (one + (one - p[neg]) * e)
    D[D == 0] = 0                      # -0 -> +0
    return D


def scores_with_mask(J, p, mask, dtype=np.float64):
    D = score(J, p, dtype)
    D[~np.asarray(mask, dtype=bool)] = -1
    return D


# ---------------------------------------------------------------- selection
def select(scores, remove):
    """offsets (ascending) of the `remove` active elements smallest under (bits of D as uint64, offset); active: D >= 0"""
    flat = np.ascontiguousarray(scores, dtype=np.float64).ravel()
    act = np.flatnonzero(~np.signbit(flat))
    keys = flat[act].view(np.uint64)
    order = np.argsort(keys, kind="stable")            # stable: ties keep ascending offset
    return np.sort(act[order[:remove]])


def selection_info(scores, remove):
    flat = np.ascontiguousarray(scores, dtype=np.float64).ravel()
    act = np.flatnonzero(~np.signbit(flat))
    keys = np.sort(flat[act].view(np.uint64))[:remove]
    s = 0.0
    for v in keys.view(np.float64):
        s += v
    return dict(active_before=act.size, removed=remove, active_after=act.size - remove,
                threshold=float(keys.view(np.float64)[-1]) if remove else 0.0, removed_sum=s)


# ---------------------------------------------------------------- masked update
def masked_update(x, fi, fij, gi, gij, rates, mask):
    """update of tests/test_boltzmann.py, then +0 at the removed coupling elements"""
    from test_boltzmann import update
    out = update(x, fi, fij, gi, gij, *rates)
    J = out[fi.size:]
    J[~np.asarray(mask, dtype=bool).ravel()] = 0
    return out


# ---------------------------------------------------------------- gauge
def zero_sum_gauge(x, L, q, details=False):
    """the stated order in float64, rounded once to x's dtype; details: also the addends' magnitudes, dict(row, col: sum over
    the 4 q addends |J| + |r| + |c| + |m| of every new block row / column (pairs x q), site: sum over the q (L + 1) addends
    |h| + sum_j |part| + |u| of every site's new fields (L))"""
    v = np.asarray(x).astype(np.float64)
    h, J = v[:L * q].reshape(L, q).copy(), v[L * q:].reshape(-1, q, q)
    P = J.shape[0]
    r, c = np.zeros((P, q)), np.zeros((P, q))
    for b in range(q):
        r = r + J[:, :, b]
    for a in range(q):
        c = c + J[:, a, :]
    r, c = r / float(q), c / float(q)
    m = np.zeros(P)
    for a in range(q):
        m = m + r[:, a]
    m = m / float(q)
    Jn = ((J - r[:, :, None]) - c[:, None, :]) + m[:, None, None]
    toi, toj = r - m[:, None], c - m[:, None]
    iu, ju = pairs_of(L)
    pid = -np.ones((L, L), dtype=np.int64)
    pid[iu, ju] = np.arange(P)
    site = np.zeros(L)
    for i in range(L):
        t = h[i].copy()
        mag = np.abs(t)
        for j in range(L):
            if j != i:
                part = toj[pid[j, i]] if j < i else toi[pid[i, j]]
                t = t + part
                mag = mag + np.abs(part)
        u = 0.0
        for a in range(q):
            u = u + t[a]
        h[i] = t - u / float(q)
        site[i] = mag.sum() + q * abs(u / float(q))
    out = np.concatenate([h.ravel(), Jn.ravel()]).astype(np.asarray(x).dtype)
    if not details:
        return out
    A = np.abs(J)
    row = A.sum(axis=2) + q * np.abs(r) + np.abs(c).sum(axis=1)[:, None] + q * np.abs(m)[:, None]
    col = A.sum(axis=1) + np.abs(r).sum(axis=1)[:, None] + q * np.abs(c) + q * np.abs(m)[:, None]
    return out, dict(row=row, col=col, site=site)


def energies(x, S, L, q):
    """E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j) in float64 -> (E, sum of |terms|)"""
    v = np.asarray(x, dtype=np.float64)
    h, J = v[:L * q].reshape(L, q), v[L * q:].reshape(-1, q, q)
    iu, ju = pairs_of(L)
    S = np.asarray(S, dtype=np.int64)
    th = h[np.arange(L)[None, :], S]
    tj = J[np.arange(iu.size)[None, :], S[:, iu], S[:, ju]]
    return th.sum(axis=1) + tj.sum(axis=1), np.abs(th).sum(axis=1) + np.abs(tj).sum(axis=1)
