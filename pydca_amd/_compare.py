"""Comparing sequence sets with the alignment (DESIGN.md sections 17, 20 and 21): Hamming distances to the nearest natural sequence,
the agreement of one- and two-site frequencies and connected correlations, beyond what a pairwise fit has seen, of the
strongest three-site connected correlations, and the principal components of the reweighted alignment with the projections
of natural and generated sequences onto them.  Model-free -- the methods need the alignment and its
sequence weights, never fitted parameters -- so one mixin serves PlmDCA, MeanFieldDCA and ArDCA, before or after a fit."""
import numpy as np

from . import _lib, _potts


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


def _relabel_elements(elements, site_map):
    el = np.asarray(elements)
    sites = np.asarray(site_map)[el[:, :3]]
    o = np.argsort(sites, axis=1, kind='stable')
    out = np.empty(el.shape, dtype=np.int32)
    out[:, :3] = np.take_along_axis(sites, o, axis=1)
    out[:, 3:] = np.take_along_axis(el[:, 3:], o, axis=1)
    return out


def elements_from_order(elements, order):
    """Three-site elements (i, j, k, a, b, c) over the columns of a permuted alignment (position j holds file site order[j]) ->
    the same elements over the file's sites: every site relabelled, then the three (site, state) pairs sorted by site, so
    i < j < k again and every state follows its site.  The rows keep their order."""
    return _relabel_elements(elements, np.asarray(order))


def elements_to_order(elements, order):
    """The inverse of elements_from_order: elements over the file's sites -> over the permuted alignment's columns."""
    return _relabel_elements(elements, np.argsort(np.asarray(order)))


def centred_fit(x, y):
    """(pearson, slope, max |x - y|) of two vectors with the analytic mean 0, as dca_set_comparison defines them: Sxx = sum x^2,
    Syy, Sxy; pearson = Sxy / sqrt(Sxx Syy) (0 when Sxx Syy <= 0), slope = Sxy / Sxx (0 when Sxx == 0).  In double."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    sxx, syy, sxy = float(np.dot(x, x)), float(np.dot(y, y)), float(np.dot(x, y))
    vv = sxx * syy
    return (float(sxy / np.sqrt(vv)) if vv > 0.0 else 0.0, sxy / sxx if sxx > 0.0 else 0.0,
            float(np.max(np.abs(x - y))) if x.size else 0.0)


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

    def _three_site_count(self, name, v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise self._compare_exc('{} must be an integer, not {!r}'.format(name, v))
        return int(v)

    def _three_site_skip(self, include_gaps, name='include_gaps'):
        # the encoders of both residue tables give the gap the last code, q - 1
        return -1 if _flag(name, include_gaps, self._compare_exc) else self._compare_dims()[2] - 1

    def _three_site_scan(self, ctx, K, Q, skip):
        el, c3, f3 = ctx.three_site_scan(K, Q, skip)
        order = self._compare_order()
        return (el if order is None else elements_from_order(el, order)), c3, f3

    def _three_site_elements(self, elements):
        _bio, L, q = self._compare_dims()
        try:
            return _lib.three_site_elements(elements, L, q)
        except ValueError as e:
            raise self._compare_exc(str(e))

    def compute_top_three_site_correlations(self, num_top=10000, sequences=None, include_gaps=True):
        """The num_top strongest three-site connected correlations c_ijk(a, b, c) = f_ijk - f_ij f_k - f_ik f_j - f_jk f_i +
        2 f_i f_j f_k, found by scanning ALL site triples and states, of the alignment under its sequence weights (sequences None)
        or of a sequence set (a FASTA path or a list of aligned strings; unit weights) -> dict: elements int32[K, 6], rows
        (i, j, k, a, b, c) with the sites in file order and i < j < k; c3 and f3 float64[K].  Sorted by |c3| descending; equal
        values in ascending order of the row as the context holds it (for ArDCA that is the model's site order, so ties may
        come in another order than from PlmDCA).  K = min(num_top, number of elements).  include_gaps=False leaves every
        element that names the gap state out.  Counts are integers: the alignment's weights enter as llrint(w 2^40)."""
        K = self._three_site_count('num_top', num_top)
        if K < 1:
            raise self._compare_exc('num_top must be >= 1, not {}'.format(K))
        skip = self._three_site_skip(include_gaps)
        self._compare_one_gpu('compute_top_three_site_correlations')
        if self._compare_dims()[1] < 3:
            raise self._compare_exc('three-site correlations need at least three sites')
        Q = None if sequences is None else self._compare_codes(sequences, 'compute_top_three_site_correlations')
        el, c3, f3 = self._three_site_scan(self._compare_context(), K, Q, skip)
        return {'elements': el, 'c3': c3, 'f3': f3}

    def compute_three_site_correlations(self, elements, sequences=None):
        """(f3, c3), float64[T] each, at the listed elements: int[T, 6] rows (i, j, k, a, b, c), sites in file order with
        i < j < k, states as the encoder codes them -- of the alignment under its weights (sequences None) or of a set."""
        el = self._three_site_elements(elements)
        self._compare_one_gpu('compute_three_site_correlations')
        Q = None if sequences is None else self._compare_codes(sequences, 'compute_three_site_correlations')
        order = self._compare_order()
        _count, _denom, f3, c3 = self._compare_context().three_site_values(el if order is None else elements_to_order(el, order), Q)
        return f3, c3

    def _pca_fit(self, num_components, tolerance, max_iterations, seed):
        """The fit in the context's column order, cached per argument tuple."""
        _bio, L, q = self._compare_dims()
        try:
            key = _lib.pca_arguments(num_components, tolerance, max_iterations, seed, L, q)
        except ValueError as e:
            raise self._compare_exc(str(e))
        self._compare_one_gpu('compute_principal_components')
        cache = self.__dict__.setdefault('_pca_cache', {})
        if key not in cache:
            k, tol, iters, sd = key
            self._compare_logger.info('\n\t{} principal components of the reweighted alignment'.format(k))
            fit = self._compare_context().pca_fit(k, tol, iters, sd)
            if not fit['converged']:
                lam1 = float(fit['eigenvalues'][0])
                worst = int(np.argmax(fit['residuals']))
                raise self._compare_exc('the principal components did not converge in {} iterations: component {} has the residual '
                                        '{:.3e}, above tolerance * lambda_1 = {:.3e}'.format(fit['iterations'], worst,
                                                                                            float(fit['residuals'][worst]), tol * lam1))
            cache[key] = fit
        return cache[key]

    def compute_principal_components(self, num_components=2, tolerance=1e-10, max_iterations=1000, seed=0):
        """The num_components largest eigenpairs of the covariance C = sum_n w_n (x_n - f)(x_n - f)^T / Meff of the one-hot
        alignment under its sequence weights (all q states, the gap included; include/dca_hip.h: dca_pca_fit) -> dict:
        eigenvalues float64[k] (descending), components float64[k, L, q] (unit vectors, sites in file order, the entry of largest
        magnitude positive), offsets float64[k] (c_m = sum f v_m), explained_variance_ratio (eigenvalues / total_variance),
        total_variance (the trace of C), residuals float64[k] (||C v - lambda v||) and iterations.  The fit stops when every
        residual is <= tolerance * lambda_1; a component with lambda <= tolerance * lambda_1 is null (zeros).  Cached per
        argument tuple; a fit that does not converge within max_iterations raises.  seed picks the start block."""
        fit = self._pca_fit(num_components, tolerance, max_iterations, seed)
        comp = fit['components']
        order = self._compare_order()
        if order is not None:
            full = np.empty_like(comp)
            full[:, order, :] = comp
            comp = full
        total = float(fit['total_variance'])
        lam = fit['eigenvalues'].copy()
        return {'eigenvalues': lam, 'components': comp.copy(), 'offsets': fit['offsets'].copy(),
                'explained_variance_ratio': lam / total if total > 0.0 else np.zeros_like(lam), 'total_variance': total,
                'residuals': fit['residuals'].copy(), 'iterations': int(fit['iterations'])}

    def project_sequences(self, sequences=None, num_components=2, tolerance=1e-10, max_iterations=1000, seed=0):
        """Coordinates of the sequences (a FASTA path or a list of aligned strings; None: the rows of the alignment the instance
        fits on) along the principal components of compute_principal_components(num_components, ...) -> float64[n, k]:
        p_m(s) = sum_i v_m(i, s_i) - c_m, so the alignment's weighted mean is 0 and its weighted variance lambda_m.  A sequence
        has the same coordinates alone and in any batch."""
        fit = self._pca_fit(num_components, tolerance, max_iterations, seed)
        Q = None if sequences is None else self._compare_codes(sequences, 'project_sequences')
        return self._compare_context().pca_project(fit['components'], fit['offsets'], Q)

    def compare_with_alignment(self, sequences, return_frequencies=False, three_site=0, three_site_include_gaps=True, pca=0):
        """Do the sequences reproduce the alignment's statistics?  -> dict: pearson_fi / pearson_fij / pearson_cij, slope_* and
        max_abs_diff_* of the set's one-site frequencies, two-site frequencies and connected correlations c_ij(a, b) = f_ij(a, b)
        - f_i(a) f_j(b) against the alignment's under its sequence weights (no pseudocount; x = alignment, y = set; all states,
        gap included); num_sequences; nearest_distance (int32[n], compute_distances_to_alignment) with nearest_distance_mean /
        _median / _min and fraction_identical (distance 0); alignment_self_distance_mean / _median / _min
        (compute_alignment_self_distances).  return_frequencies adds fi (L x q) and fij (pairs x q x q, pair order) of the set,
        sites in file order.  three_site = K > 0 adds the check on a statistic the fit never saw: the alignment's K strongest
        three-site connected correlations (compute_top_three_site_correlations, with three_site_include_gaps) against the set's
        values at the same elements -- pearson_cijk, slope_cijk, max_abs_diff_cijk (same definitions, analytic mean 0) and
        three_site_terms, the number of elements compared.  pca = K > 0 adds pca_eigenvalues (the alignment's K largest,
        compute_principal_components) and pca_set_mean / pca_set_variance, float64[K]: the set's unweighted mean and variance
        along each component (the alignment's own, under its weights, are 0 and the eigenvalue)."""
        rf = _flag('return_frequencies', return_frequencies, self._compare_exc)
        K3 = self._three_site_count('three_site', three_site)
        if K3 < 0:
            raise self._compare_exc('three_site must be >= 0, not {}'.format(K3))
        skip3 = self._three_site_skip(three_site_include_gaps, 'three_site_include_gaps')
        Kp = self._three_site_count('pca', pca)
        if Kp < 0:
            raise self._compare_exc('pca must be >= 0, not {}'.format(Kp))
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
        if K3 > 0:
            el, x3, _f3 = ctx.three_site_scan(K3, None, skip3)         # the context's column order serves both calls
            y3 = ctx.three_site_values(el, Q)[3] if el.shape[0] else np.zeros(0)
            out['pearson_cijk'], out['slope_cijk'], out['max_abs_diff_cijk'] = centred_fit(x3, y3)
            out['three_site_terms'] = int(el.shape[0])
        if Kp > 0:
            fit = self._pca_fit(Kp, 1e-10, 1000, 0)
            p = ctx.pca_project(fit['components'], fit['offsets'], Q)
            mean = p.mean(axis=0)
            out['pca_eigenvalues'] = fit['eigenvalues'].copy()
            out['pca_set_mean'], out['pca_set_variance'] = mean, ((p - mean[None, :]) ** 2).mean(axis=0)
        if rf:
            order = self._compare_order()
            if order is not None:
                full = np.empty_like(fi)
                full[order] = fi
                fi, fij = full, pairs_to_order(fij, order)
            out['fi'], out['fij'] = fi, fij
        return out


def run_compare(instance, prefix, msa_file, output_dir, metadata, query_file, exc_type, three_site=0, three_site_include_gaps=True,
                pca=0):
    """compare_sequences of the plmdca, mfdca and ardca command lines -> the path of <output_dir>/<prefix>_sequence_comparison_
    <alignment base>.txt (dca_utilities.write_sequence_comparison).  pca = K > 0 adds the header lines pca_eigenvalues_<m>,
    pca_set_mean_<m> and pca_set_variance_<m>, m = 1..K.  No fit is run."""
    from .dca_utilities import dca_utilities
    if not query_file:
        raise exc_type('compare_sequences needs --query_file')
    dca_utilities.create_directories(output_dir)
    extra = dict(three_site=int(three_site), three_site_include_gaps=bool(three_site_include_gaps)) if three_site else {}
    if pca:
        extra['pca'] = int(pca)
    summary = dict(instance.compare_with_alignment(query_file, **extra))
    for key in ('pca_eigenvalues', 'pca_set_mean', 'pca_set_variance'):        # the header takes scalars: one line per component
        for m, v in enumerate(summary.pop(key, ())):
            summary['{}_{}'.format(key, m + 1)] = float(v)
    dist, index, hist = instance.compute_distances_to_alignment(query_file, return_index=True, return_histogram=True)
    _d, self_hist = instance.compute_alignment_self_distances(return_histogram=True)
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_sequence_comparison_', postfix='.txt')
    dca_utilities.write_sequence_comparison(path, summary, dist, index, hist, self_hist, int(instance.sequences_len), metadata=metadata,
                                            query_file=query_file)
    return path


def add_pca_arguments(p):
    """The options of the compute_pca sub-command of the plmdca, mfdca and ardca command lines."""
    p.add_argument('--num_components', type=int, default=2, help='number of principal components, 1 .. 64 (addition)')
    p.add_argument('--query_file', help='FASTA file of aligned sequences to project besides the alignment (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the start block of the subspace iteration (addition)')


def run_pca(instance, prefix, msa_file, output_dir, metadata, query_file=None, num_components=None, seed=None):
    """compute_pca of the plmdca, mfdca and ardca command lines -> the paths written under <output_dir>:
    <prefix>_pca_<alignment base>.txt (per component: eigenvalue, explained ratio, residual; the iterations in the header),
    <prefix>_pca_components_<alignment base>.npy (float64[k, L, q]), <prefix>_pca_projections_<alignment base>.txt (row, weight,
    coordinates of every alignment row) and, with a query file, <prefix>_pca_query_projections_<alignment base>.txt (record,
    coordinates).  No model is fitted."""
    from .dca_utilities import dca_utilities
    dca_utilities.create_directories(output_dir)
    k = 2 if num_components is None else num_components
    sd = 0 if seed is None else seed
    fit = instance.compute_principal_components(num_components=k, seed=sd)
    proj = instance.project_sequences(None, num_components=k, seed=sd)
    weights = instance._compare_context().weights()
    path = lambda what, postfix: dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_' + what + '_', postfix=postfix)
    rule = '#' + '=' * 100
    g = lambda v: '%.17g' % float(v)

    def write(name, header, rows):
        with open(name, 'w') as fh:
            for line in header:
                fh.write(line + '\n')
            for row in rows:
                fh.write(row + '\n')

    summary, comps, projections = path('pca', '.txt'), path('pca_components', '.npy'), path('pca_projections', '.txt')
    head = [rule] + list(metadata or []) + [
        '#\tPrincipal components of the reweighted one-hot alignment: {}'.format(len(fit['eigenvalues'])),
        '#\tTotal variance (trace of the covariance): {}'.format(g(fit['total_variance'])),
        '#\tIterations: {}'.format(int(fit['iterations'])),
        '# The First column is the component (1-based), the Second its eigenvalue, the Third the explained variance ratio',
        '# and the Fourth the residual ||C v - lambda v||', rule]
    write(summary, head, ('{0:<5} {1} {2} {3}'.format(m + 1, g(fit['eigenvalues'][m]), g(fit['explained_variance_ratio'][m]),
                                                       g(fit['residuals'][m])) for m in range(len(fit['eigenvalues']))))
    np.save(comps, fit['components'])
    head = [rule] + list(metadata or []) + [
        '# The First column is the alignment row (0-based), the Second its sequence weight, then its coordinate along every component',
        rule]
    write(projections, head, ('{0:<7} {1} {2}'.format(n, g(weights[n]), ' '.join(g(v) for v in proj[n])) for n in range(proj.shape[0])))
    out = [summary, comps, projections]
    if query_file:
        qp = instance.project_sequences(query_file, num_components=k, seed=sd)
        queries = path('pca_query_projections', '.txt')
        head = [rule] + list(metadata or []) + ['#\tQuery sequences: {}'.format(query_file),
                                                '# The First column is the record number (1-based) of the query sequence, then its coordinate along every component',
                                                rule]
        write(queries, head, ('{0:<7} {1}'.format(n + 1, ' '.join(g(v) for v in qp[n])) for n in range(qp.shape[0])))
        out.append(queries)
    return tuple(out)
