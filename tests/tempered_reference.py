"""A float64 numpy restatement of replica-exchange Gibbs sampling (dca_plm_sample_tempered), for
test_tempered_sampling_host.py (held there to exact enumeration and to the plain sampler's restatement) and
test_tempered_sampling.py (the device against it): gibbs_ref-style sweeps with a beta per chain, the exchange rule and the
Philox stream of the library (philox_np).  Needs no GPU."""
import numpy as np

from test_potts_sampling import random_start, uniforms

SWAP_TAG = 5


def energies_np(h, Jp, S):
    """E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j) in numpy's own order (the device tests pass the context's energies)."""
    L = h.shape[0]
    S = np.asarray(S, dtype=np.int64)
    iu, ju = np.triu_indices(L, 1)
    return h[np.arange(L)[None, :], S].sum(axis=1) + Jp[np.arange(iu.size)[None, :], S[:, iu], S[:, ju]].sum(axis=1)


def sweeps_per_chain_beta(h, Jp, beta, seed, chains, first_sweep, sweeps, S):
    """test_potts_sampling.gibbs_ref with chain c under beta[c]: S (int64[n, L]) is updated in place -> the smallest relative
    draw margin."""
    L, q = h.shape
    iu, ju = np.triu_indices(L, 1)
    pidx = np.zeros((L, L), dtype=np.int64)
    pidx[iu, ju] = np.arange(iu.size)
    pidx[ju, iu] = np.arange(iu.size)
    rows = np.arange(S.shape[0])
    beta = np.asarray(beta, dtype=np.float64)[:, None]
    margin = np.inf
    for t in range(sweeps):
        for i in range(L):
            Jrow = Jp[pidx[i]].copy()                                  # L x q x q, block (min, max)
            Jrow[:i] = Jrow[:i].transpose(0, 2, 1)                   # j < i: J(a, b) = block(j, i)[b, a]
            Jrow[i] = 0.0
            u = h[i][None, :] + Jrow[np.arange(L)[None, :], :, S].sum(axis=1)
            p = np.exp(beta * (u - u.max(axis=1, keepdims=True)))
            cum = np.cumsum(p, axis=1)
            T = cum[:, -1]
            r = uniforms(seed, chains, first_sweep + t, i, 0) * T
            above = cum > r[:, None]
            pick = np.where(above.any(axis=1), above.argmax(axis=1), q - 1 - np.argmax((p > 0)[:, ::-1], axis=1))
            margin = min(margin, float((np.abs(cum - r[:, None]) / T[:, None]).min()))
            S[rows, i] = pick
    return margin


def tempered_ref(h, Jp, betas, ladders, sweeps, swap_interval, seed, first_ladder=0, first_sweep=0, initial=None,
                 initial_levels=None, energy=None):
    """The whole scheme: M = ladders ladders of R = len(betas) walkers, walker r of ladder m at row m R + r with Philox chain
    (first_ladder + m) R + r, starting at level r (or initial_levels) from the tag-1 random state (or `initial`).  After the
    global sweep g with (g + 1) % I == 0, round rho = (g + 1) / I - 1: for k = rho (mod 2), k + 1 < R, a / b the walkers at
    levels k / k + 1, d = (betas[k+1] - betas[k]) * (E_a - E_b), U = Philox(ladder, rho, k, 5), accept iff d >= 0 or U < exp(d);
    accepting exchanges the levels.  energy: codes -> E (default energies_np).
    -> dict: codes uint8[n, L], levels int32[n], attempts / accepts uint64[R - 1], trace float64[rounds, M, R] (E of the walker
    at level k before the exchange), rounds, gibbs_margin, swap_margin (the smallest |U - exp(d)| over decisions with d < 0)."""
    L, q = h.shape
    betas = np.asarray(betas, dtype=np.float64)
    M, R, I = int(ladders), betas.size, int(swap_interval)
    n = M * R
    energy = energy or (lambda codes: energies_np(h, Jp, codes))
    chains = (first_ladder + np.arange(n) // R) * R + np.arange(n) % R
    S = (random_start(seed, chains, L, q) if initial is None else np.asarray(initial)).astype(np.int64).copy()
    level = (np.arange(n) % R if initial_levels is None else np.asarray(initial_levels, dtype=np.int64)).reshape(M, R).copy()
    walker_at = np.argsort(level, axis=1)
    attempts = np.zeros(max(R - 1, 0), dtype=np.uint64)
    accepts = np.zeros(max(R - 1, 0), dtype=np.uint64)
    trace = []
    gibbs_margin = swap_margin = np.inf
    lad = np.arange(M)
    for t in range(sweeps):
        g = first_sweep + t
        gibbs_margin = min(gibbs_margin, sweeps_per_chain_beta(h, Jp, betas[level.reshape(-1)], seed, chains, g, 1, S))
        if I <= 0 or (g + 1) % I:
            continue
        rho = (g + 1) // I - 1
        E = np.asarray(energy(S.astype(np.uint8)), dtype=np.float64).reshape(M, R)
        trace.append(E[lad[:, None], walker_at])
        for k in range(rho & 1, R - 1, 2):
            a, b = walker_at[:, k].copy(), walker_at[:, k + 1].copy()
            d = (betas[k + 1] - betas[k]) * (E[lad, a] - E[lad, b])
            U = uniforms(seed, first_ladder + lad, rho, k, SWAP_TAG)
            with np.errstate(over="ignore"):
                ed = np.exp(d)
            acc = (d >= 0) | (U < ed)
            if (d < 0).any():
                swap_margin = min(swap_margin, float(np.abs(U - ed)[d < 0].min()))
            attempts[k] += np.uint64(M)
            accepts[k] += np.uint64(int(acc.sum()))
            walker_at[acc, k], walker_at[acc, k + 1] = b[acc], a[acc]
            level[lad[acc], a[acc]] = k + 1
            level[lad[acc], b[acc]] = k
    return {"codes": S.astype(np.uint8), "levels": level.reshape(-1).astype(np.int32), "attempts": attempts, "accepts": accepts,
            "trace": np.array(trace, dtype=np.float64).reshape(len(trace), M, R), "rounds": len(trace),
            "gibbs_margin": gibbs_margin, "swap_margin": swap_margin}


def exact_distribution(h, Jp, beta):
    """All q^L states, their energies and P(s) ~ exp(beta E(s)) -> (states uint8[q^L, L], E, P)."""
    L, q = h.shape
    states = np.array(np.unravel_index(np.arange(q ** L), (q,) * L)).T.astype(np.uint8)
    E = energies_np(h, Jp, states)
    w = np.exp(beta * (E - E.max()))
    return states, E, w / w.sum()


def two_basin_model(L, q, strength, bias):
    """An enumerable model with two basins: J_ij(a, a) = strength for the states a = 0 and a = 1 on every pair, h_i(1) = bias,
    and every other state pushed down by h_i(a) = -strength -> (h, Jp, x: the plm parameter vector)."""
    h = np.zeros((L, q))
    h[:, 1] = bias
    h[:, 2:] = -strength
    Jp = np.zeros((L * (L - 1) // 2, q, q))
    Jp[:, 0, 0] = Jp[:, 1, 1] = strength
    return h, Jp, np.concatenate([h.reshape(-1), Jp.reshape(-1)])


def other_basin_share(codes):
    """the share of rows with more sites in state 1 than in state 0"""
    codes = np.asarray(codes)
    return float(((codes == 1).sum(axis=1) > (codes == 0).sum(axis=1)).mean())
