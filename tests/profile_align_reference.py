"""Plain restatement of the profile-alignment contract of dca_profile_align (include/dca_hip.h): the
integer recurrence, the end-cell rule and the traceback state machine.  Python integers, no device, no library.

    D[i][j] = max(D[i-1][j] + del_extend[i], H[i-1][j] + del_open[i])        column i deleted
    I[i][j] = max(I[i][j-1] + ins_extend,    H[i][j-1] + ins_open)           residue j inserted
    H[i][j] = max(H[i-1][j-1] + match[i][s_j], D[i][j], I[i][j])             local mode: also 0

align_one is the definition, cell by cell.  align_batch runs the same recurrence for many queries at once (numpy over the
queries, the same loops over i and j) so that a GPU test's reference costs milliseconds; test_profile_align_host.py holds
the two equal."""
import numpy as np

LOCAL, GLOCAL = 0, 1
NEG = -(1 << 28)


def matrices(match, del_open, del_extend, ins_open, ins_extend, mode, seq):
    """H, D, I as lists of lists, (Lp + 1) x (len + 1); profile column i = 1..Lp is row i - 1 of the tables"""
    Lp, n = len(match), len(seq)
    H = [[0] * (n + 1) for _ in range(Lp + 1)]
    D = [[NEG] * (n + 1) for _ in range(Lp + 1)]
    I = [[NEG] * (n + 1) for _ in range(Lp + 1)]
    if mode == GLOCAL:
        for i in range(1, Lp + 1):
            H[i][0] = D[i][0] = int(del_open[0]) if i == 1 else H[i - 1][0] + int(del_extend[i - 1])
    for i in range(1, Lp + 1):
        for j in range(1, n + 1):
            D[i][j] = max(D[i - 1][j] + int(del_extend[i - 1]), H[i - 1][j] + int(del_open[i - 1]))
            I[i][j] = max(I[i][j - 1] + ins_extend, H[i][j - 1] + ins_open)
            h = max(H[i - 1][j - 1] + int(match[i - 1][seq[j - 1]]), D[i][j], I[i][j])
            H[i][j] = max(h, 0) if mode == LOCAL else h
    return H, D, I


def end_cell(H, mode):
    """(score, i, j): local -- the first maximum in row-major order, i outer (a zero matrix ends at (0, 0));
    glocal -- max_j H[Lp][j] at the smallest j"""
    Lp, n = len(H) - 1, len(H[0]) - 1
    if mode == GLOCAL:
        best, bj = H[Lp][0], 0
        for j in range(1, n + 1):
            if H[Lp][j] > best:
                best, bj = H[Lp][j], j
        return best, Lp, bj
    best, bi, bj = 0, 0, 0
    for i in range(1, Lp + 1):
        for j in range(1, n + 1):
            if H[i][j] > best:
                best, bi, bj = H[i][j], i, j
    return best, bi, bj


def traceback(H, D, I, match, del_open, ins_open, mode, seq, i, j):
    """residue_at[Lp] from the end cell (i, j): in H the diagonal, then D, then I (local: stop at H = 0); in D or I back to H
    whenever "open" is co-optimal with "extend"; at j = 0 the remaining columns are deletions"""
    Lp = len(H) - 1
    res = [-1] * Lp
    state = 0
    while i > 0 and j > 0:
        if state == 0:
            if mode == LOCAL and H[i][j] == 0:
                break
            if H[i][j] == H[i - 1][j - 1] + int(match[i - 1][seq[j - 1]]):
                res[i - 1] = j - 1
                i, j = i - 1, j - 1
            elif H[i][j] == D[i][j]:
                state = 1
            else:
                state = 2
        elif state == 1:
            if D[i][j] == H[i - 1][j] + int(del_open[i - 1]):
                state = 0
            i -= 1
        else:
            if I[i][j] == H[i][j - 1] + ins_open:
                state = 0
            j -= 1
    return res, i, j


def align_one(match, del_open, del_extend, ins_open, ins_extend, mode, seq):
    """-> (score, residue_at, (start_i, start_j), (end_i, end_j)); start: the cell the traceback stopped at"""
    seq = [int(c) for c in seq]
    H, D, I = matrices(match, del_open, del_extend, ins_open, ins_extend, mode, seq)
    score, bi, bj = end_cell(H, mode)
    res, si, sj = traceback(H, D, I, match, del_open, ins_open, mode, seq, bi, bj)
    return score, res, (si, sj), (bi, bj)


def align_batch(match, del_open, del_extend, ins_open, ins_extend, mode, seqs):
    """The same for a list of code arrays -> (int32[n] scores, int32[n, Lp] residue_at)"""
    match = np.asarray(match, dtype=np.int64)
    do, de = np.asarray(del_open, dtype=np.int64), np.asarray(del_extend, dtype=np.int64)
    Lp, n = match.shape[0], len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    W = int(lens.max()) if n else 0
    S = np.zeros((n, W + 1), dtype=np.int64)
    for k, s in enumerate(seqs):
        S[k, 1:1 + len(s)] = np.asarray(s, dtype=np.int64)
    H = np.zeros((Lp + 1, W + 1, n), dtype=np.int64)
    D = np.full((Lp + 1, W + 1, n), NEG, dtype=np.int64)
    I = np.full((Lp + 1, W + 1, n), NEG, dtype=np.int64)
    if mode == GLOCAL:
        for i in range(1, Lp + 1):
            H[i, 0] = D[i, 0] = do[0] if i == 1 else H[i - 1, 0] + de[i - 1]
    for i in range(1, Lp + 1):
        M = match[i - 1][S]                      # n x (W + 1)
        D[i, 1:] = np.maximum(D[i - 1, 1:] + de[i - 1], H[i - 1, 1:] + do[i - 1])
        for j in range(1, W + 1):
            I[i, j] = np.maximum(I[i, j - 1] + ins_extend, H[i, j - 1] + ins_open)
            h = np.maximum(np.maximum(H[i - 1, j - 1] + M[:, j], D[i, j]), I[i, j])
            H[i, j] = np.maximum(h, 0) if mode == LOCAL else h
    scores = np.zeros(n, dtype=np.int32)
    res = np.full((n, Lp), -1, dtype=np.int32)
    for k in range(n):
        ln = int(lens[k])
        Hk, Dk, Ik = (X[:, :ln + 1, k].tolist() for X in (H, D, I))
        score, bi, bj = end_cell(Hk, mode)
        scores[k] = score
        res[k], _si, _sj = traceback(Hk, Dk, Ik, match, do, ins_open, mode, [int(c) for c in seqs[k]], bi, bj)
    return scores, res


# ---- the query profile of the back-mapper's Smith-Waterman (dca_sw_scores / dca_sw_align): 26 letters plus "other"
def sw_profile(ref, sub, gap_open, gap_extend):
    """-> (match int32[len(ref), 27], del_open, del_extend, ins_open, ins_extend): match[i][b] = sub[ref_i][b]; a character that
    is no capital letter, in the reference or in a query, scores -4 against everything"""
    sub = np.asarray(sub)
    match = np.full((len(ref), 27), -4, dtype=np.int32)
    for i, c in enumerate(ref):
        a = ord(c) - 65
        if 0 <= a < 26:
            match[i, :26] = sub[a, :26]
    n = len(ref)
    return match, np.full(n, gap_open, dtype=np.int32), np.full(n, gap_extend, dtype=np.int32), int(gap_open), int(gap_extend)


def sw_codes(s):
    return np.array([ord(c) - 65 if 0 <= ord(c) - 65 < 26 else 26 for c in s], dtype=np.uint8)


def residue_at_from_pair(n_ref, aligned_a, aligned_b, start_a, start_b):
    """what dca_sw_align returned (the aligned region and its starts) as residue_at over the reference's positions"""
    res = [-1] * n_ref
    i, j = start_a, start_b
    for x, y in zip(aligned_a, aligned_b):
        if x != '-' and y != '-':
            res[i] = j
        i += x != '-'
        j += y != '-'
    return res
