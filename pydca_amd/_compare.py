"""Comparing sequence sets with the alignment: Hamming distances to the nearest natural sequence and the
agreement of one- and two-site frequencies and connected correlations.  Model-free -- the methods need the alignment and its
sequence weights, never fitted parameters -- so one mixin serves PlmDCA, MeanFieldDCA and ArDCA, before or after a fit."""
import numpy as np

from . import _potts


def distance_summary(dist):
    """(mean, median, min) of the distances >= 0 (a query without partner has -1) as floats; NaN for none."""
    d = np.asarray(dist)
    d = d[d >= 0]
    if not d.size:
        return float('nan'), float('nan'), float('nan')
    return float(d.mean()), float(np.median(d)), float(d.min())


def pairs_to_order(fij, order):
    """fij: pairs x q x q over the sites of a permuted alignment (position j holds file site order[j]) -> the same blocks in the
    pair order of the file's sites, each transposed where the permutation swaps its two sites."""
    order = np.asarray(order)
    L = order.size
    inv = np.argsort(order)
    iu, ju = np.triu_indices(L, 1)
    a, b = inv[iu], inv[ju]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    p = L * (L - 1) // 2 - (L - lo) * (L - lo - 1) // 2 + (hi - lo - 1)
    out = fij[p]
    swap = a > b
    out[swap] = np.transpose(out[swap], (0, 2, 1))
    return out


def _picked(dist, index, hist, return_index, return_histogram):
    if not return_index and not return_histogram:
        return dist
    return (dist,) + ((index,) if return_index else ()) + ((hist,) if return_histogram else ())


def _flag(name, v, exc_type):
    if not isinstance(v, (bool, np.bool_)):
        raise exc_type('{} must be True or False, not {!r}'.format(name, v))
    return bool(v)


class SequenceComparison:
    """A class supplies: _compare_exc (its exception type), _compare_logger, _compare_table (residue table of the encoder: 0 plm,
    1 mf), _compare_dims() -> (biomolecule code, L, q), _compare_devices() (None or the GPU list), _compare_context() -> a
    Context holding the alignment and its weights (no fit is run for it) and _compare_order() -> None, or the permutation under
    which that context holds the alignment's columns (position j = file site order[j])."""

    def _compare_one_gpu(self, what):
        devices = self._compare_devices()
        if devices and len(devices) > 1:
            self._compare_logger.error('\n\t{} runs on one GPU; devices={}'.format(what, devices))
            raise self._compare_exc('{} runs on one GPU, not on devices {}'.format(what, devices))

    def _compare_codes(self, sequences, what):
        if sequences is None:
            raise self._compare_exc('{} needs sequences: a FASTA file or a list of aligned strings'.format(what))
        bio, L, _q = self._compare_dims()
        X = _potts.query_codes(sequences, bio, L, self._compare_table, self._compare_exc)
        if X.shape[0] < 1:
            raise self._compare_exc('{} needs at least one sequence'.format(what))
        order = self._compare_order()
        return X if order is None else np.ascontiguousarray(X[:, order])       # the queries are permuted, never the answer

    def compute_distances_to_alignment(self, sequences, return_index=False, return_histogram=False):
        """Hamming distance of every sequence to the nearest sequence of the alignment -> int32[n]; with return_index also
        int32[n], the smallest row index that attains it; with return_histogram also uint64[L + 1], the number of (query,
        alignment row) pairs at every distance 0..L.  sequences: a FASTA path or a list of aligned strings.  The reference set,
        and the meaning of the index, are the encoded rows the instance fits on: for PlmDCA and ArDCA the alignment after the
        reader's de-duplication (first occurrences, file order), for MeanFieldDCA the rows of its alignment as read.  Distances
        count differing sites, gaps included as a state; they do not depend on a model's site order."""
        ri, rh = _flag('return_index', return_index, self._compare_exc), _flag('return_histogram', return_histogram, self._compare_exc)
        self._compare_one_gpu('compute_distances_to_alignment')
        Q = self._compare_codes(sequences, 'compute_distances_to_alignment')
        self._compare_logger.info('\n\tNearest alignment sequence of {} sequences'.format(Q.shape[0]))
        d, i, h = self._compare_context().hamming_nearest(Q, None, False, return_index=ri, return_histogram=rh)
        return _picked(d, i, h, ri, rh)

    def compute_alignment_self_distances(self, return_index=False, return_histogram=False):
        """Every row of the alignment (as in compute_distances_to_alignment) against all OTHER rows: the natural baseline the
        distances of a sample are plotted against.  Same returns; a one-row alignment gives -1."""
        ri, rh = _flag('return_index', return_index, self._compare_exc), _flag('return_histogram', return_histogram, self._compare_exc)
        self._compare_one_gpu('compute_alignment_self_distances')
        d, i, h = self._compare_context().hamming_nearest(None, None, True, return_index=ri, return_histogram=rh)
        return _picked(d, i, h, ri, rh)

    def compute_set_diversity(self, sequences):
        """The set against itself -> (int32[n] distance to the nearest OTHER member, int32[n] its index, uint64[L + 1] histogram of
        all ordered pairs of different members): a collapsed chain population shows here."""
        self._compare_one_gpu('compute_set_diversity')
        Q = self._compare_codes(sequences, 'compute_set_diversity')
        return self._compare_context().hamming_nearest(None, Q, True)

    def compare_with_alignment(self, sequences, return_frequencies=False):
        """Do the sequences reproduce the alignment's statistics?  -> dict: pearson_fi / pearson_fij / pearson_cij, slope_* and
        max_abs_diff_* of the set's one-site frequencies, two-site frequencies and connected correlations c_ij(a, b) = f_ij(a, b)
        - f_i(a) f_j(b) against the alignment's under its sequence weights (no pseudocount; x = alignment, y = set; all states,
        gap included); num_sequences; nearest_distance (int32[n], compute_distances_to_alignment) with nearest_distance_mean /
        _median / _min and fraction_identical (distance 0); alignment_self_distance_mean / _median / _min
        (compute_alignment_self_distances).  return_frequencies adds fi (L x q) and fij (pairs x q x q, pair order) of the set,
        sites in file order."""
        rf = _flag('return_frequencies', return_frequencies, self._compare_exc)
        self._compare_one_gpu('compare_with_alignment')
        Q = self._compare_codes(sequences, 'compare_with_alignment')
        ctx = self._compare_context()
        fi, fij, cmp_ = ctx.sequence_statistics(Q, frequencies=rf, compare=True)
        out = {'num_sequences': int(Q.shape[0])}
        for name in ('pearson', 'slope', 'max_abs_diff'):
            for k, what in enumerate(('fi', 'fij', 'cij')):
                out['{}_{}'.format(name, what)] = float(cmp_[name][k])
        d = ctx.hamming_nearest(Q, None, False, return_index=False, return_histogram=False)[0]
        s = ctx.hamming_nearest(None, None, True, return_index=False, return_histogram=False)[0]
        out['nearest_distance'] = d
        out['nearest_distance_mean'], out['nearest_distance_median'], out['nearest_distance_min'] = distance_summary(d)
        out['fraction_identical'] = float(np.mean(d == 0))
        out['alignment_self_distance_mean'], out['alignment_self_distance_median'], out['alignment_self_distance_min'] = distance_summary(s)
        if rf:
            order = self._compare_order()
            if order is not None:
                full = np.empty_like(fi)
                full[order] = fi
                fi, fij = full, pairs_to_order(fij, order)
            out['fi'], out['fij'] = fi, fij
        return out


def run_compare(instance, prefix, msa_file, output_dir, metadata, query_file, exc_type):
    """compare_sequences of the plmdca, mfdca and ardca command lines -> the path of <output_dir>/<prefix>_sequence_comparison_
    <alignment base>.txt (dca_utilities.write_sequence_comparison).  No fit is run."""
    from .dca_utilities import dca_utilities
    if not query_file:
        raise exc_type('compare_sequences needs --query_file')
    dca_utilities.create_directories(output_dir)
    summary = instance.compare_with_alignment(query_file)
    dist, index, hist = instance.compute_distances_to_alignment(query_file, return_index=True, return_histogram=True)
    _d, self_hist = instance.compute_alignment_self_distances(return_histogram=True)
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_sequence_comparison_', postfix='.txt')
    dca_utilities.write_sequence_comparison(path, summary, dist, index, hist, self_hist, int(instance.sequences_len), metadata=metadata,
                                            query_file=query_file)
    return path
