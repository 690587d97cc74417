"""Numpy brute force of the three-site entries (include/dca_hip.h, dca_three_site_values / dca_three_site_scan), shared by
tests/test_three_site_host.py (which checks it on its own) and tests/test_three_site.py (which checks the GPU against it).
Counts are uint64 one-hot einsums over the integer weights; c_ijk is formed in the header's order, left to right."""
import itertools

import numpy as np


def quantised_weights(w):
    """llrint(w 2^40) as uint64 (np.rint rounds half to even, like llrint under the default rounding mode)"""
    return np.rint(np.asarray(w, dtype=np.float64) * 2.0 ** 40).astype(np.uint64)


def tile_side(q):
    """the header's rule for the scan's tile: the largest of 8, 4, 2 with TB^2 q^2 <= 7168"""
    for tb in (8, 4):
        if tb * tb * q * q <= 7168:
            return tb
    return 2


def all_elements(L, q, skip_state=-1):
    """int32[T, 6]: every (i, j, k, a, b, c), i < j < k, in ascending (linear-index) order, without the skipped state"""
    tri = np.array(list(itertools.combinations(range(L), 3)), dtype=np.int32).reshape(-1, 3)
    st = np.array([s for s in itertools.product(range(q), repeat=3) if skip_state not in s], dtype=np.int32).reshape(-1, 3)
    return np.concatenate([np.repeat(tri, st.shape[0], axis=0), np.tile(st, (tri.shape[0], 1))], axis=1)


def brute_force(X, wq, q):
    """X: uint8[N, L], wq: uint64[N] -> dict: denom (int), n1 uint64[L, q], n2 {(i, j): uint64[q, q]}, n3 / f3 / c3
    {(i, j, k): [q, q, q]} for every i < j < k"""
    X = np.asarray(X)
    wq = np.asarray(wq, dtype=np.uint64)
    N, L = X.shape
    oh = (X[:, :, None] == np.arange(q)[None, None, :]).astype(np.uint64)
    denom = int(wq.sum(dtype=np.uint64))
    M = np.float64(denom)
    n1 = np.einsum('n,nia->ia', wq, oh)
    n2 = {(i, j): np.einsum('n,na,nb->ab', wq, oh[:, i], oh[:, j]) for i, j in itertools.combinations(range(L), 2)}
    f1 = n1.astype(np.float64) / M
    f2 = {p: v.astype(np.float64) / M for p, v in n2.items()}
    n3, f3, c3 = {}, {}, {}
    for i, j, k in itertools.combinations(range(L), 3):
        n = np.einsum('n,na,nb,nc->abc', wq, oh[:, i], oh[:, j], oh[:, k])
        f = n.astype(np.float64) / M
        fi, fj, fk = f1[i][:, None, None], f1[j][None, :, None], f1[k][None, None, :]
        fij, fik, fjk = f2[i, j][:, :, None], f2[i, k][:, None, :], f2[j, k][None, :, :]
        n3[i, j, k], f3[i, j, k] = n, f
        c3[i, j, k] = f - fij * fk - fik * fj - fjk * fi + 2.0 * fi * fj * fk
    return {'denom': denom, 'n1': n1, 'n2': n2, 'n3': n3, 'f3': f3, 'c3': c3}


def flat(ref, name, L):
    """the values of all_elements(L, q) in its order"""
    return np.concatenate([ref[name][t].reshape(-1) for t in itertools.combinations(range(L), 3)])


def top_elements(ref, L, q, K, skip_state=-1):
    """(elements int32[found, 6], c3, f3): the stable sort by (-|c|, linear index) of the eligible elements, cut at K"""
    el = all_elements(L, q)
    c, f = flat(ref, 'c3', L), flat(ref, 'f3', L)
    if skip_state >= 0:
        keep = ~(el[:, 3:] == skip_state).any(axis=1)
        el, c, f = el[keep], c[keep], f[keep]
    o = np.argsort(-np.abs(c), kind='stable')[:K]
    return el[o], c[o], f[o]
