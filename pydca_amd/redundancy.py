"""Redundancy filter, identity clusters and a cluster-wise hold-out split of an alignment.

Preprocessing next to the trimmer: file -> filtered / split file -> fit.  The compares run on the device
(dca_identity_filter, dca_identity_clusters; integer-exact); turning an identity fraction into a number of sites, the
priority orders and the split are host code here.

ident(m, n) = #{i : X_mi = X_ni}, the gap state counting like any other; two rows are similar iff ident >= T."""
import logging
import os

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)


def identity_threshold(L, identity=None, strict=False, min_identical_sites=None):
    """-> T, the number of identical sites from which two rows of length L are similar.
    min_identical_sites gives it directly (1 .. L + 1).  Else, default: the smallest k in 0..L with k / L >= identity in
    float64 (identity = 1.0 removes exact duplicates); strict: the smallest k with k / L > identity, the rule of the sequence
    weights.  No such k: L + 1 (nothing is similar to anything)."""
    L = int(L)
    if L < 1:
        raise ValueError("L must be >= 1, not %d" % L)
    if min_identical_sites is not None:
        if isinstance(min_identical_sites, (bool, np.bool_)) or not isinstance(min_identical_sites, (int, np.integer)):
            raise ValueError("min_identical_sites must be an integer, not %r" % (min_identical_sites,))
        T = int(min_identical_sites)
        if T < 1 or T > L + 1:
            raise ValueError("min_identical_sites must be in 1 .. L + 1 = %d, not %d" % (L + 1, T))
        return T
    if isinstance(identity, (bool, np.bool_)) or not isinstance(identity, (int, float, np.integer, np.floating)):
        raise ValueError("identity must be a number, not %r" % (identity,))
    ident = float(identity)
    if not np.isfinite(ident):
        raise ValueError("identity must be finite, not %r" % (identity,))
    T = L + 1
    for k in range(L + 1):
        v = np.float64(k) / np.float64(L)
        if (v > ident) if strict else (v >= ident):
            T = k
            break
    if T < 1:
        raise ValueError("identity %r makes rows without a common site similar; give an identity that needs one site at least" % (identity,))
    return T


def priority_order(X, q, priority='file'):
    """-> None (file order) or int32[n], the permutation in which the filter visits the rows.  'fewest_gaps': gap count (state
    q - 1) ascending, then row index; an integer array: taken as the order itself (checked to be a permutation)."""
    n = X.shape[0]
    if isinstance(priority, str):
        if priority == 'file':
            return None
        if priority == 'fewest_gaps':
            gaps = (X == q - 1).sum(axis=1)
            return np.lexsort((np.arange(n), gaps)).astype(np.int32)
        raise ValueError("priority must be 'file', 'fewest_gaps' or an integer array, not %r" % (priority,))
    raw = np.asarray(priority)
    if raw.ndim != 1 or raw.size != n or not np.issubdtype(raw.dtype, np.integer):
        raise ValueError("priority must hold the %d row indices as integers" % n)
    if not np.array_equal(np.sort(raw.astype(np.int64)), np.arange(n)):
        raise ValueError("priority is not a permutation of 0 .. %d" % (n - 1))
    return np.ascontiguousarray(raw, dtype=np.int32)


def cluster_summary(labels, rounds=None, degrees=None):
    labels = np.asarray(labels, dtype=np.int32)
    roots, counts = np.unique(labels, return_counts=True)
    out = dict(labels=labels, num_clusters=int(roots.size), sizes={int(r): int(c) for r, c in zip(roots, counts)}, rounds=rounds)
    if degrees is not None:
        out['degrees'] = degrees
    return out


def split_by_labels(labels, test_fraction=0.1, seed=0):
    """Whole clusters go to the test side in the order of numpy.random.default_rng(seed).permutation of the (ascending) cluster
    labels, until it holds at least test_fraction * n rows; a cluster that alone exceeds the remaining half of n -- that would
    lift the test side above n / 2 -- is skipped.  -> (train_idx, test_idx), ascending.  Host code."""
    labels = np.asarray(labels)
    n = labels.size
    if not (0.0 <= float(test_fraction) <= 0.5):
        raise ValueError("test_fraction must be in 0 .. 0.5, not %r" % (test_fraction,))
    roots, counts = np.unique(labels, return_counts=True)
    want = float(test_fraction) * n
    in_test = np.zeros(n, dtype=bool)
    held = 0
    for k in np.random.default_rng(seed).permutation(roots.size):
        if held >= want:
            break
        if held + int(counts[k]) > n / 2.0:
            continue
        in_test |= labels == roots[k]
        held += int(counts[k])
    idx = np.arange(n)
    return idx[~in_test], idx[in_test]


def _context_for(X, q, device):
    X = np.ascontiguousarray(X, dtype=np.uint8)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("the rows must be a uint8 array of shape (n, L)")
    ctx = _lib.Context(device, _lib.DCA_F64)
    ctx.set_msa(X, int(q))
    return ctx


def _filter(ctx, X, q, identity, priority, strict, min_identical_sites, return_representatives):
    T = identity_threshold(ctx.L, identity, strict, min_identical_sites)
    order = priority_order(X, q, priority)
    keep, rep, _info = ctx.identity_filter(T, None, order, return_representatives)
    kept = np.nonzero(keep)[0]
    return (kept, rep) if return_representatives else kept


def _clusters(ctx, identity, strict, min_identical_sites, return_degrees):
    T = identity_threshold(ctx.L, identity, strict, min_identical_sites)
    labels, degrees, info = ctx.identity_clusters(T, None, return_degrees)
    return cluster_summary(labels, info['rounds'], degrees if return_degrees else None)


def filter(X, q, identity=0.9, priority='file', strict=False, min_identical_sites=None, return_representatives=False, device=0):
    """The greedy redundancy filter of the encoded rows X (uint8[n, L], codes < q) -> the kept row indices, ascending (with
    return_representatives: and int32[n], each row's representative)."""
    ctx = _context_for(X, q, device)
    try:
        return _filter(ctx, np.asarray(X), q, identity, priority, strict, min_identical_sites, return_representatives)
    finally:
        ctx.close()


def clusters(X, q, identity=0.8, strict=False, min_identical_sites=None, return_degrees=False, device=0):
    """Single-linkage clusters of the encoded rows -> dict(labels, num_clusters, sizes, rounds[, degrees])"""
    ctx = _context_for(X, q, device)
    try:
        return _clusters(ctx, identity, strict, min_identical_sites, return_degrees)
    finally:
        ctx.close()


def split(X, q, identity=0.8, test_fraction=0.1, seed=0, strict=False, device=0):
    """(train_idx, test_idx): whole clusters at `identity` held out, so that no test row is similar to any train row"""
    return split_by_labels(clusters(X, q, identity, strict, device=device)['labels'], test_fraction, seed)


def write_fasta(path, records, indices):
    """The chosen (header, sequence) records, in the order of `indices`, one line per sequence"""
    with open(path, 'w') as fh:
        for k in indices:
            header, seq = records[int(k)]
            fh.write('>%s\n%s\n' % (header, seq))


class AlignmentRedundancy:
    """All records of a FASTA alignment, in file order and with their headers (no de-duplication: finding the duplicates is
    the point), on one GPU context that holds the alignment only."""

    def __init__(self, msa_file, biomolecule, device=0):
        from .msa_trimmer.msa_trimmer import read_fasta_records
        self.msa_file = msa_file
        self.biomolecule = biomolecule.strip().upper()
        if self.biomolecule not in ('PROTEIN', 'RNA'):
            raise ValueError('biomolecule {!r} is neither PROTEIN nor RNA'.format(biomolecule))
        self.q = 21 if self.biomolecule == 'PROTEIN' else 5
        self.records = [(r.id, r.seq) for r in read_fasta_records(msa_file)]
        L = len(self.records[0][1])
        # the mfDCA reader's table: upper-cased, characters outside it are the gap state
        self.X = _lib.encode_sequences([s.upper() for _h, s in self.records], _lib.PROTEIN if self.q == 21 else _lib.RNA, L, 1)
        self.num_sequences, self.sequences_len = self.X.shape
        self._ctx = _lib.Context(device, _lib.DCA_F64)
        self._ctx.set_msa(self.X, self.q)
        logger.info('\n\tRecords read from %s: %d of length %d', msa_file, self.num_sequences, L)

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def headers(self):
        return [h for h, _s in self.records]

    def threshold(self, identity=None, strict=False, min_identical_sites=None):
        return identity_threshold(self.sequences_len, identity, strict, min_identical_sites)

    def filter(self, identity=0.9, priority='file', strict=False, min_identical_sites=None, return_representatives=False):
        return _filter(self._ctx, self.X, self.q, identity, priority, strict, min_identical_sites, return_representatives)

    def clusters(self, identity=0.8, strict=False, min_identical_sites=None, return_degrees=False):
        return _clusters(self._ctx, identity, strict, min_identical_sites, return_degrees)

    def split(self, identity=0.8, test_fraction=0.1, seed=0, strict=False):
        return split_by_labels(self.clusters(identity, strict)['labels'], test_fraction, seed)

    def write_fasta(self, path, indices):
        write_fasta(path, self.records, indices)


# ---------------------------------------------------------------- the three sub-commands of `pydca`
REDUNDANCY_SUBCOMMANDS = ['filter_by_identity', 'cluster_sequences', 'split_by_clusters']
OUTPUT_PREFIX = {'filter_by_identity': 'Filtered_', 'cluster_sequences': 'Clusters_', 'split_by_clusters': 'Split_'}


def add_subparsers(subparsers):
    p = subparsers.add_parser('filter_by_identity', help='Keeps one representative of every group of sequences at or above --identity '
                              '(greedy, in file order or by --priority)')
    p.add_argument('--identity', type=float, default=0.9)
    p.add_argument('--priority', choices=['file', 'fewest_gaps'], default='file')
    p = subparsers.add_parser('cluster_sequences', help='Single-linkage clusters of the sequences at --identity')
    p.add_argument('--identity', type=float, default=0.8)
    p = subparsers.add_parser('split_by_clusters', help='Holds whole clusters at --identity out as a test alignment')
    p.add_argument('--identity', type=float, default=0.8)
    p.add_argument('--test_fraction', type=float, default=0.1)
    p.add_argument('--seed', type=int, default=0)
    for name in REDUNDANCY_SUBCOMMANDS:
        p = subparsers.choices[name]
        p.add_argument('biomolecule')
        p.add_argument('msa_file')
        p.add_argument('--strict', action='store_true', help='similar iff identity > the fraction (the rule of the sequence weights)')
        p.add_argument('--device', type=int, default=0)
        p.add_argument('--verbose', action='store_true')
        p.add_argument('--output_dir')


def execute(the_command, msa_file, biomolecule, identity=None, priority='file', strict=False, test_fraction=0.1, seed=0, output_dir=None,
            device=0, redundancy_class=None):
    """Runs one sub-command -> the list of files written.  redundancy_class: a stand-in for AlignmentRedundancy (tests)."""
    from .dca_utilities import dca_utilities
    cls = redundancy_class or AlignmentRedundancy
    if not output_dir:
        base, _ext = os.path.splitext(os.path.basename(msa_file))
        output_dir = OUTPUT_PREFIX[the_command] + base
    dca_utilities.create_directories(output_dir)

    def out(prefix, postfix):
        return dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix, postfix=postfix)
    red = cls(msa_file, biomolecule, device=device)
    try:
        headers = red.headers
        if the_command == 'filter_by_identity':
            kept, rep = red.filter(identity=0.9 if identity is None else identity, priority=priority, strict=strict,
                                   return_representatives=True)
            files = [out('Filtered_', '.fa'), out('Filtered_', '_representatives.txt')]
            red.write_fasta(files[0], kept)
            with open(files[1], 'w') as fh:
                fh.write('# row\theader\trepresentative row\n')
                for r, h in enumerate(headers):
                    fh.write('%d\t%s\t%d\n' % (r, h, rep[r]))
        elif the_command == 'cluster_sequences':
            res = red.clusters(identity=0.8 if identity is None else identity, strict=strict, return_degrees=True)
            files = [out('Clusters_', '.txt')]
            with open(files[0], 'w') as fh:
                fh.write('# clusters: %d\trounds: %s\n# row\theader\tlabel\tcluster size\tdegree\n' % (res['num_clusters'], res['rounds']))
                for r, h in enumerate(headers):
                    lab = int(res['labels'][r])
                    fh.write('%d\t%s\t%d\t%d\t%d\n' % (r, h, lab, res['sizes'][lab], res['degrees'][r]))
        elif the_command == 'split_by_clusters':
            train, test = red.split(identity=0.8 if identity is None else identity, test_fraction=test_fraction, seed=seed, strict=strict)
            files = [out('Train_', '.fa'), out('Test_', '.fa')]
            red.write_fasta(files[0], train)
            red.write_fasta(files[1], test)
        else:
            raise NotImplementedError('{} is not a redundancy sub-command'.format(the_command))
    finally:
        if hasattr(red, 'close'):
            red.close()
    return files
