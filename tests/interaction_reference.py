"""Float64 numpy restatement of the inter-protein energies (include/dca_hip.h, dca_plm_interaction_energies) in the stated order,
the same sums in longdouble, the iterative pairing loop in numpy with an exhaustive assignment, and planted paired data.

A model is (Jp, L, q): Jp float64[pairs, q, q], the upper-triangle blocks in pair order, every stored value widened to double
(test_potts_sampling.plm_model / mf_model).  Elementwise numpy arithmetic in float64 is IEEE and never contracted, so a loop
over the summed index with whole-array adds is the sequential sum of the rule."""
import itertools

import numpy as np


def pair_index(L, i, j):
    return L * (L - 1) // 2 - (L - i) * (L - i - 1) // 2 + (j - i - 1)


def cross_blocks(Jp, L, split, dtype=np.float64):
    """J[i, j] = the stored block of the pair (i, split + j): [LA, LB, q, q]"""
    LA, LB = split, L - split
    idx = np.array([[pair_index(L, i, split + j) for j in range(LB)] for i in range(LA)], dtype=np.int64)
    return np.asarray(Jp)[idx].astype(dtype)


def zero_sum(J):
    """r(a) = (sum_b J(a, b)) / q, c(b) = (sum_a J(a, b)) / q, m = (sum_a r(a)) / q, each sum from 0.0 in ascending index;
    Jt = ((J - r(a)) - c(b)) + m; in J's dtype"""
    q = J.shape[-1]
    dq = J.dtype.type(q)
    r = np.zeros(J.shape[:-1], dtype=J.dtype)
    for b in range(q):
        r = r + J[..., :, b]
    r = r / dq
    c = np.zeros(J.shape[:-2] + (q,), dtype=J.dtype)
    for a in range(q):
        c = c + J[..., a, :]
    c = c / dq
    m = np.zeros(J.shape[:-2], dtype=J.dtype)
    for a in range(q):
        m = m + r[..., a]
    m = m / dq
    return ((J - r[..., :, None]) - c[..., None, :]) + m[..., None, None]


def cross_couplings(Jp, L, split, gauge, dtype=np.float64):
    J = cross_blocks(Jp, L, split, dtype)
    return zero_sum(J) if gauge else J


def cross_fields(Jt, XA):
    """phi[m, j, b] = sum over i ascending of Jt[i, j, XA[m, i], b], from 0.0; in Jt's dtype"""
    LA, LB, q, _ = Jt.shape
    XA = np.asarray(XA, dtype=np.int64)
    phi = np.zeros((XA.shape[0], LB, q), dtype=Jt.dtype)
    for i in range(LA):
        phi = phi + Jt[i][:, XA[:, i], :].transpose(1, 0, 2)
    return phi


def cross_energies(phi, XB):
    """E[m, n] = sum over j ascending of phi[m, j, XB[n, j]], from 0.0"""
    XB = np.asarray(XB, dtype=np.int64)
    E = np.zeros((phi.shape[0], XB.shape[0]), dtype=phi.dtype)
    for j in range(phi.shape[1]):
        E = E + phi[:, j, :][:, XB[:, j]]
    return E


def interaction_energies(Jp, L, split, XA, XB, gauge, offsets_a=None, offsets_b=None, dtype=np.float64):
    """the dense array, or with offsets the list of blocks"""
    Jt = cross_couplings(Jp, L, split, gauge, dtype)
    if offsets_a is None:
        return cross_energies(cross_fields(Jt, XA), XB)
    XA, XB = np.asarray(XA), np.asarray(XB)
    return [cross_energies(cross_fields(Jt, XA[offsets_a[g]:offsets_a[g + 1]]), XB[offsets_b[g]:offsets_b[g + 1]])
            for g in range(len(offsets_a) - 1)]


def addend_sums(Jt, XA, XB):
    """sum over i, j of |Jt_ij(a_i, b_j)| per pair (m, n), in longdouble: the addends of E(m, n)"""
    A = np.abs(Jt.astype(np.longdouble))
    return cross_energies(cross_fields(A, XA), XB)


def sum_bound(Jt, XA, XB):
    """(LA + LB) 2^-53 sum |addends|: a sequential sum of LA terms feeding one of LB terms, to first order"""
    LA, LB = Jt.shape[:2]
    return (LA + LB) * 2.0 ** -53 * addend_sums(Jt, XA, XB).astype(np.float64)


def full_energies(h, Jp, X, dtype=np.longdouble):
    """E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j) of concatenated rows, and the sum of |terms|"""
    X = np.asarray(X, dtype=np.int64)
    L = X.shape[1]
    iu, ju = np.triu_indices(L, 1)
    hv = np.asarray(h).astype(dtype)[np.arange(L)[None, :], X]
    Jv = np.asarray(Jp).astype(dtype)[np.arange(iu.size)[None, :], X[:, iu], X[:, ju]]
    return hv.sum(axis=1) + Jv.sum(axis=1), np.abs(hv).sum(axis=1) + np.abs(Jv).sum(axis=1)


# ---------------------------------------------------------------- assignment by exhaustive search
def brute_assignment(E, forbid=None):
    """(best total, col_of_row) over all matchings of size min(nr, nc); forbid = (r, c) may not be used; -inf / None if none"""
    E = np.asarray(E)
    nr, nc = E.shape
    best, arg = -np.inf, None
    if nr <= nc:
        for cols in itertools.permutations(range(nc), nr):
            if forbid is not None and cols[forbid[0]] == forbid[1]:
                continue
            t = sum(E[r, cols[r]] for r in range(nr))
            if t > best:
                best, arg = t, list(cols)
    else:
        for rows in itertools.permutations(range(nr), nc):
            if forbid is not None and rows[forbid[1]] == forbid[0]:
                continue
            t = sum(E[rows[c], c] for c in range(nc))
            if t > best:
                best = t
                arg = [-1] * nr
                for c, r in enumerate(rows):
                    arg[r] = c
    return best, arg


def brute_assign_with_gaps(E):
    """(col_of_row, total, gaps) as dca_assign_partners defines them"""
    E = np.asarray(E, dtype=np.float64)
    nr, nc = E.shape
    if nr == 0 or nc == 0:
        return np.full(nr, -1), 0.0, np.zeros(nr)
    total, cols = brute_assignment(E)
    gaps = np.zeros(nr)
    for r, c in enumerate(cols):
        if c >= 0:
            other, arg = brute_assignment(E, (r, c))
            gaps[r] = np.inf if arg is None else total - other
    return np.array(cols), total, gaps


# ---------------------------------------------------------------- planted paired data
def planted_pairs(G=80, per=4, LA=6, LB=7, q=5, copy=0.9, gaps=0.03, seed=0, sizes_b=None):
    """G species of `per` true pairs: A rows uniform over the q - 1 non-gap states; each B site copies a permuted A site (a
    fixed site map and a fixed state permutation per B site) with probability `copy`, else uniform; `gaps` of all entries are
    then set to the gap state q - 1.  The B rows of every species are shuffled: true_b_of_a[m] is the B row of A row m.
    sizes_b (optional, per species): extra unpaired B rows (rectangular blocks).
    -> XA uint8[nA, LA], XB uint8[nB, LB], species_a, species_b (labels per row), true_b_of_a"""
    rng = np.random.default_rng([seed, G, per, LA, LB, q])
    site_of = rng.integers(0, LA, size=LB)
    perms = np.stack([rng.permutation(q - 1) for _ in range(LB)])
    XA, XB, sa, sb, true_b = [], [], [], [], []
    nb = 0
    for g in range(G):
        A = rng.integers(0, q - 1, size=(per, LA))
        B = perms[np.arange(LB)[None, :], A[:, site_of]]
        noise = rng.integers(0, q - 1, size=(per, LB))
        B = np.where(rng.random((per, LB)) < copy, B, noise)
        extra = 0 if sizes_b is None else int(sizes_b[g]) - per
        if extra > 0:
            B = np.concatenate([B, rng.integers(0, q - 1, size=(extra, LB))])
        A = np.where(rng.random(A.shape) < gaps, q - 1, A)
        B = np.where(rng.random(B.shape) < gaps, q - 1, B)
        order = rng.permutation(B.shape[0])
        pos = np.empty_like(order)
        pos[order] = np.arange(order.size)
        XA.append(A)
        XB.append(B[order])
        sa += [g] * per
        sb += [g] * B.shape[0]
        true_b += [nb + int(pos[k]) for k in range(per)]
        nb += B.shape[0]
    return (np.concatenate(XA).astype(np.uint8), np.concatenate(XB).astype(np.uint8), np.array(sa), np.array(sb),
            np.array(true_b, dtype=np.int64))


# ---------------------------------------------------------------- the pairing loop
def group_rows(labels):
    """labels -> (species in order of first appearance, list of row-index arrays, stable)"""
    order, rows = [], {}
    for k, s in enumerate(labels):
        if s not in rows:
            rows[s] = []
            order.append(s)
        rows[s].append(k)
    return order, [np.array(rows[s], dtype=np.int64) for s in order]


def philox_np(ctr, key):
    """Philox4x32-10 on uint32[4] / uint32[2]"""
    c = [int(v) for v in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for r in range(10):
        if r > 0:
            k0 = (k0 + 0x9E3779B9) & 0xffffffff
            k1 = (k1 + 0xBB67AE85) & 0xffffffff
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xffffffff, p1 & 0xffffffff, ((p0 >> 32) ^ c[3] ^ k1) & 0xffffffff, p0 & 0xffffffff]
    return c


PAIRING_TAG = 6


def random_pairing(rows_a, rows_b, seed):
    """One-to-one random pairing within every species: Fisher-Yates over the species' B rows, position k = n - 1 .. 1 swapped
    with position floor(U n') for n' = k + 1, U from Philox4x32-10 with key (seed lo, seed hi) and counter (species index, k, 0,
    PAIRING_TAG), U = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53; the first min(nA, nB) A rows take the shuffled B rows in order."""
    pairs = []
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    for g, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        perm = list(rb)
        for k in range(len(perm) - 1, 0, -1):
            w = philox_np((g & 0xffffffff, k, 0, PAIRING_TAG), key)
            u = ((w[0] >> 5) * 67108864 + (w[1] >> 6)) * 2.0 ** -53
            t = int(u * (k + 1))
            perm[k], perm[t] = perm[t], perm[k]
        pairs += [(int(a), int(b)) for a, b in zip(ra, perm)]
    return pairs


def mf_model_of(X, q, pseudocount, seqid):
    """(Jp, L): the mean-field couplings of the alignment X (0-based codes) as pair-order q x q blocks, zero on the gap state"""
    from oracle import mf as omf
    X = np.asarray(X)
    L = X.shape[1]
    _, J = omf.mfdca_fn(X.astype(np.int32) + 1, q, pseudocount, seqid)
    qm = q - 1
    J4 = J.reshape(L, qm, L, qm)
    iu, ju = np.triu_indices(L, 1)
    Jp = np.zeros((iu.size, q, q))
    Jp[:, :qm, :qm] = J4[iu, :, ju, :]
    return Jp, L


def rank_pairs(assigned):
    """assigned: list of (a, b, energy, gap, species) -> ranked by gap descending, equal gaps in ascending A index"""
    return sorted(assigned, key=lambda t: (-t[3], t[0]))


def ipa_reference(XA, XB, species_a, species_b, q, training_pairs=None, n_increment=6, pseudocount=0.5, seqid=0.8, gauge=1, seed=0,
                  max_rounds=None, true_pairs=None, assign=brute_assign_with_gaps):
    """The iterative pairing loop in numpy; the rows of the training pairs leave the testing set.  -> dict(pairs, history); history[r]: training (the pairs trained on), assigned
    (ranked list), min_gap (smallest finite gap of a species' assigned rows, per species), max_abs_E, boundary (gap difference
    across the next round's selection boundary, or None)"""
    XA, XB = np.asarray(XA), np.asarray(XB)
    LA = XA.shape[1]
    order_a, rows_a_all = group_rows(list(species_a))
    order_b, rows_b_all = group_rows(list(species_b))
    in_b = dict(zip(order_b, rows_b_all))
    species = [s for s in order_a if s in in_b]
    rows_a = [r for s, r in zip(order_a, rows_a_all) if s in in_b]
    rows_b = [in_b[s] for s in species]
    training_pairs = [] if training_pairs is None else [(int(a), int(b)) for a, b in training_pairs]
    used_a, used_b = {a for a, _ in training_pairs}, {b for _, b in training_pairs}        # training rows leave the testing set
    rows_a = [np.array([r for r in ra if int(r) not in used_a], dtype=np.int64) for ra in rows_a]
    rows_b = [np.array([r for r in rb if int(r) not in used_b], dtype=np.int64) for rb in rows_b]
    start = training_pairs if training_pairs else random_pairing(rows_a, rows_b, seed)
    truth = None if true_pairs is None else set((int(a), int(b)) for a, b in true_pairs)
    history, ranked, rnd, took_all = [], [], 0, False
    while True:
        rnd += 1
        if rnd == 1:
            train = list(start)
        else:
            fixed = set(training_pairs)
            free = [(a, b) for a, b, _e, _g, _s in ranked if (a, b) not in fixed]
            extra = free[:(rnd - 1) * n_increment]
            took_all = len(extra) == len(free)       # every pair assigned in the previous round is trained on: the last round
            train = list(training_pairs) + extra
        X = np.concatenate([XA[[a for a, _ in train]], XB[[b for _, b in train]]], axis=1)
        Jp, L = mf_model_of(X, q, pseudocount, seqid)
        Jt = cross_couplings(Jp, L, LA, gauge)
        assigned, min_gaps, max_abs = [], [], 0.0
        for s, ra, rb in zip(species, rows_a, rows_b):
            if len(ra) == 0 or len(rb) == 0:
                min_gaps.append(np.inf)
                continue
            E = cross_energies(cross_fields(Jt, XA[ra]), XB[rb])
            max_abs = max(max_abs, float(np.abs(E).max()))
            cols, _total, gaps = assign(E)
            fin = [gaps[k] for k in range(len(ra)) if cols[k] >= 0 and np.isfinite(gaps[k])]
            min_gaps.append(min(fin) if fin else np.inf)
            assigned += [(int(ra[k]), int(rb[cols[k]]), float(E[k, cols[k]]), float(gaps[k]), s) for k in range(len(ra)) if cols[k] >= 0]
        ranked = rank_pairs(assigned)
        fixed = set(training_pairs)
        free = [t for t in ranked if (t[0], t[1]) not in fixed]
        cut = rnd * n_increment
        boundary = free[cut - 1][3] - free[cut][3] if 0 < cut < len(free) else None
        rec = dict(training=train, training_size=len(train), assigned=ranked, min_gap=min_gaps, max_abs_E=max_abs, boundary=boundary,
                   mean_gap=float(np.mean([t[3] for t in ranked if np.isfinite(t[3])])) if ranked else 0.0)
        if truth is not None:
            rec["true_positive_fraction"] = sum((t[0], t[1]) in truth for t in ranked) / max(len(ranked), 1)
        history.append(rec)
        if took_all or (max_rounds is not None and rnd >= max_rounds):
            break
    return dict(pairs=[(t[0], t[1]) for t in ranked], gaps=[t[3] for t in ranked], species=[t[4] for t in ranked], history=history)


# ---------------------------------------------------------------- the case table of tests/test_interaction_energies.py
# group sizes (nA_g, nB_g) of one call: 0, 1, 63, 64, 65 and 257 on either side, forty 5 x 5 species (items closed by the row
# limit), twenty rows of 256 partners (an item closed by the pair limit) and a 257 x 257 block (two windows, the second of one row)
MAIN_GROUPS = ([(0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 63), (257, 1), (1, 257), (0, 0)] + [(5, 5)] * 40 + [(20, 256), (257, 257),
               (3, 2)])
SMALL_GROUPS = [(1, 1), (0, 3), (65, 64), (2, 0), (3, 300), (7, 5)] + [(2, 3)] * 20
SPLITS = [(1, 1), (1, 7), (7, 1), (6, 7)]


def offsets_of(groups):
    oa = np.concatenate([[0], np.cumsum([a for a, _ in groups])]).astype(np.int32)
    ob = np.concatenate([[0], np.cumsum([b for _, b in groups])]).astype(np.int32)
    return oa, ob


def row_counts(groups):
    """the B-row count of every A-row, as interaction.hip hands it to cross_items"""
    return [b for a, b in groups for _ in range(a)]


def energy_cases(plan, q):
    """(LA, LB, groups) of every shape the GPU test runs at alphabet q; the two plan-dependent shapes come from the driver"""
    p = plan(q, 1)
    cases = [(LA, LB, MAIN_GROUPS if (LA, LB) == (6, 7) else SMALL_GROUPS) for LA, LB in SPLITS]
    cases.append((2, p["single_tile_dense"] + 1, [(17, 300)] + [(3, 3)] * 40))       # every item chunks over j
    cases.append((p["field_chunk"] + 1, 3, SMALL_GROUPS))                             # a second staging chunk of one site
    cases.append((2 * p["field_chunk"], 2, [(5, 4)]))                                 # two full staging chunks
    return cases
