"""Query sequences of the energy methods of PlmDCA and MeanFieldDCA, encoded for the context (dca_encode_sequences)."""
import operator
import os

import numpy as np

from . import _lib
from .fasta_reader import fasta_reader


def _records(source):
    if isinstance(source, (str, bytes, os.PathLike)):
        return fasta_reader.get_alignment_from_fasta_file(os.fsdecode(source), same_length=False)    # file order, duplicates kept
    return [str(getattr(rec, 'seq', rec)) for rec in source]


def query_codes(sequences, biomolecule, L, table, exc_type):
    """sequences: a FASTA path or a list of aligned strings -> uint8[n, L]; a rejected record raises exc_type naming it (1-based)."""
    seqs = _records(sequences)
    try:
        return _lib.encode_sequences(seqs, biomolecule, L, table)
    except _lib.EncodeError as exc:
        what = 'its length is not {}'.format(L) if exc.code == _lib.DCA_ERR_ARG else 'it holds a character outside the residue table'
        raise exc_type('query record {} is rejected: {} ({})'.format(exc.record + 1, what, exc))


def wildtype_codes(wildtype, biomolecule, L, table, exc_type):
    """wildtype: an aligned string of length L or a FASTA file with one record -> uint8[L]."""
    if isinstance(wildtype, (str, bytes, os.PathLike)) and os.path.isfile(os.fsdecode(wildtype)):
        seqs = fasta_reader.get_alignment_from_fasta_file(os.fsdecode(wildtype), same_length=False)
        if len(seqs) != 1:
            raise exc_type('the wild-type file {} holds {} records, not one'.format(os.fsdecode(wildtype), len(seqs)))
    elif isinstance(wildtype, str):
        seqs = [wildtype]
    else:
        raise exc_type('the wild type must be an aligned string or a FASTA file with one record')
    return query_codes(seqs, biomolecule, L, table, exc_type)[0]


def initial_codes(initial, num_sequences, biomolecule, L, table, exc_type):
    """Starting sequences of the samplers -> uint8[num_sequences, L], or None (random starts).  initial: None, an aligned
    string (every chain starts from it), a list of num_sequences aligned strings, or a FASTA file holding 1 or
    num_sequences records (one record is replicated)."""
    if initial is None:
        return None
    if isinstance(initial, (str, bytes, os.PathLike)) and os.path.isfile(os.fsdecode(initial)):
        seqs = fasta_reader.get_alignment_from_fasta_file(os.fsdecode(initial), same_length=False)
        where = 'the initial-sequence file {}'.format(os.fsdecode(initial))
    elif isinstance(initial, str):
        seqs, where = [initial], 'the initial sequence'
    else:
        seqs, where = [str(getattr(rec, 'seq', rec)) for rec in initial], 'the list of initial sequences'
    if len(seqs) not in (1, num_sequences):
        raise exc_type('{} holds {} records; sampling {} sequences needs 1 or {}'.format(where, len(seqs), num_sequences,
                                                                                       num_sequences))
    X = query_codes(seqs, biomolecule, L, table, exc_type)
    return X if X.shape[0] == num_sequences else np.repeat(X, num_sequences, axis=0)


def conditional_sites(free_sites, fixed_sites, L, exc_type):
    """The free sites of sample_sequences_conditional -> int32[F], strictly ascending.  Exactly one of free_sites and fixed_sites
    (iterables of 0-based ints, in any order) is given; fixed_sites names the complement.  A duplicate, an index outside
    [0, L) or a value that is not an integer raises exc_type.  Needs no device."""
    if (free_sites is None) == (fixed_sites is None):
        raise exc_type('give exactly one of free_sites and fixed_sites')
    name, given = ('free_sites', free_sites) if fixed_sites is None else ('fixed_sites', fixed_sites)
    try:
        idx = sorted(operator.index(v) for v in given)
    except TypeError:
        raise exc_type('{} must be an iterable of integers, not {!r}'.format(name, given))
    for a, b in zip(idx, idx[1:]):
        if a == b:
            raise exc_type('{} names site {} twice'.format(name, a))
    if idx and (idx[0] < 0 or idx[-1] >= L):
        raise exc_type('{} holds site {}; the 0-based sites are 0 .. {}'.format(name, idx[0] if idx[0] < 0 else idx[-1], L - 1))
    if fixed_sites is not None:
        idx = sorted(set(range(L)) - set(idx))
    return np.asarray(idx, dtype=np.int32)


def parse_site_ranges(text, exc_type):
    """'10-30,45' -> [9, 10, ..., 29, 44]: comma-separated 1-based sites and inclusive ranges, as the written files number the
    sites -> 0-based ints in the order written (conditional_sites sorts and checks them).  An empty list, a site < 1, a range
    that runs backwards or anything else raises exc_type."""
    out = []
    for part in str(text).split(','):
        part = part.strip()
        lo, sep, hi = part.partition('-')
        try:
            first = int(lo)
            last = int(hi) if sep else first
        except ValueError:
            raise exc_type('sites are written like 10-30,45 (1-based, inclusive), not {!r}'.format(text))
        if first < 1 or last < first:
            raise exc_type('sites are 1-based and ranges ascend: {!r} in {!r}'.format(part, text))
        out.extend(range(first - 1, last))
    return out


def template_codes(template, num_sequences, biomolecule, L, table, exc_type):
    """template of sample_sequences_conditional (an aligned string, a list of them or a FASTA file; initial_codes) ->
    uint8[n, L], n = num_sequences or, when that is None, the number of template records."""
    if template is None:
        raise exc_type('sample_sequences_conditional needs a template: an aligned string, a list of them or a FASTA file')
    if num_sequences is None:
        one = isinstance(template, str) and not os.path.isfile(template)
        n = 1 if one else len(_records(template))
    else:
        n = operator.index(num_sequences)
        if n < 0:
            raise exc_type('num_sequences must be >= 0, not {}'.format(num_sequences))
    return initial_codes(template, n, biomolecule, L, table, exc_type)


def sampling_beta(temperature, exc_type):
    """beta = 1 / temperature for a finite temperature > 0."""
    t = float(temperature)
    if not (0.0 < t < float('inf')):
        raise exc_type('the temperature must be finite and > 0, not {}'.format(temperature))
    return 1.0 / t


def temperature_ladder(t_min, t_max, num):
    """A geometric ladder of `num` temperatures from t_min to t_max (both included; finite, 0 < t_min <= t_max): neighbours keep
    the ratio (t_max / t_min)^(1 / (num - 1)), the usual first choice for replica exchange -> float64[num], ascending.  num = 1
    gives [t_min].  ValueError otherwise.  Needs no device."""
    if isinstance(num, (bool, np.bool_)) or not isinstance(num, (int, np.integer)) or int(num) < 1:
        raise ValueError('num must be an integer >= 1, not {!r}'.format(num))
    lo, hi = float(t_min), float(t_max)
    if not (0.0 < lo <= hi < float('inf')):
        raise ValueError('the ladder needs finite temperatures with 0 < t_min <= t_max, not {!r} and {!r}'.format(t_min, t_max))
    num = int(num)
    if num == 1:
        return np.array([lo])
    if lo == hi:
        raise ValueError('{} distinct temperatures need t_min < t_max'.format(num))
    t = lo * (hi / lo) ** (np.arange(num, dtype=np.float64) / (num - 1))
    t[0], t[-1] = lo, hi
    return t


def tempered_options(num_sequences, temperatures, num_sweeps, swap_interval, seed, burn_in_sweeps, exc_type):
    """Checks the arguments of sample_sequences_tempered (host only) -> dict: n, temperatures float64[T] (the caller's order),
    betas float64[R] (the distinct 1 / T, ascending; 0 for T = inf), level int64[T] (each temperature's index into betas),
    num_sweeps, swap_interval, seed, burn_in (None: num_sweeps // 2)."""
    def count(name, v, low):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < low:
            raise exc_type('{} must be an integer >= {}, not {!r}'.format(name, low, v))
        return int(v)
    opts = dict(n=count('num_sequences', num_sequences, 0), num_sweeps=count('num_sweeps', num_sweeps, 0),
                swap_interval=count('swap_interval', swap_interval, 0), seed=count('seed', seed, 0))
    opts['burn_in'] = opts['num_sweeps'] // 2 if burn_in_sweeps is None else count('burn_in_sweeps', burn_in_sweeps, 0)
    try:
        t = np.array([float(v) for v in temperatures], dtype=np.float64)
    except (TypeError, ValueError):
        raise exc_type('temperatures must be a sequence of numbers, not {!r}'.format(temperatures))
    if t.size < 1:
        raise exc_type('temperatures must hold at least one value')
    if np.isnan(t).any() or not (t > 0.0).all():
        raise exc_type('every temperature must be finite and > 0, or inf (beta = 0), not {}'.format(t.tolist()))
    betas, level = np.unique(np.where(np.isinf(t), 0.0, 1.0 / np.where(np.isinf(t), 1.0, t)), return_inverse=True)
    if opts['n'] * betas.size > 1 << 24:
        raise exc_type('num_sequences x distinct temperatures must be <= 2^24 walkers, not {} x {}'.format(opts['n'], betas.size))
    opts.update(temperatures=t, betas=betas, level=np.asarray(level, dtype=np.int64).reshape(-1))
    return opts


def tempered_result(opts, res, text):
    """The dict of sample_sequences_tempered from the checked options, the dict of Context.{plm,mf}_sample_tempered (with its
    trace) and text(codes) -> sequences.  Level k's sample of ladder m is the walker sitting at level k at the end."""
    n, betas, level = opts['n'], opts['betas'], opts['level']
    R = betas.size
    at = np.argsort(np.asarray(res['levels']).reshape(n, R), axis=1)               # at[m, k]: the walker of ladder m at level k
    rows = np.arange(n)[:, None] * R + at                                           # ... its row
    codes = np.asarray(res['codes'])[rows]                                          # [m, k, L]
    energies = np.asarray(res['energies'])[rows]                                    # [m, k]
    attempts = np.asarray(res['attempts'], dtype=np.uint64)
    with np.errstate(invalid='ignore', divide='ignore'):
        acceptance = np.where(attempts > 0, np.asarray(res['accepts'], dtype=np.float64) / attempts.astype(np.float64), np.nan)
    trace = np.asarray(res['trace'])                                                # [round, m, k]; round j ends sweep (j + 1) I - 1
    keep = (np.arange(trace.shape[0]) + 1) * opts['swap_interval'] > opts['burn_in']
    mean = np.full(R, np.nan)
    cap = np.full(R, np.nan)
    if n and keep.any():
        e = trace[keep].reshape(-1, R)
        mean = e.mean(axis=0)
        cap = betas * betas * e.var(axis=0)
    return {'temperatures': opts['temperatures'], 'sequences': [text(codes[:, k]) for k in level],
            'energies': np.ascontiguousarray(energies.T[level]), 'swap_acceptance': acceptance, 'swap_attempts': attempts,
            'mean_energy': mean[level], 'heat_capacity': cap[level], 'num_rounds': int(res['rounds'])}


def state_letters(biomolecule):
    """Letter of every 0-based state (gap last), for the CLI's mutation-effect rows and sampled sequences."""
    return list('ACDEFGHIKLMNPQRSTVWY-') if biomolecule == _lib.DCA_BIOMOLECULE_PROTEIN else list('ACGU-')



def ais_options(num_chains, num_temperatures, sweeps_per_temperature, seed, pseudocount, exc_type):
    """Checks the AIS arguments of compute_log_partition_function (host only) -> dict of the checked values."""
    def count(name, v, low):
        if isinstance(v, bool) or int(v) != v or int(v) < low:
            raise exc_type('{} must be an integer >= {}, not {!r}'.format(name, low, v))
        return int(v)
    opts = dict(num_chains=count('num_chains', num_chains, 1), num_temperatures=count('num_temperatures', num_temperatures, 1),
                sweeps_per_temperature=count('sweeps_per_temperature', sweeps_per_temperature, 0), seed=count('seed', seed, 0),
                pseudocount=None)
    if opts['num_chains'] > 1 << 24:
        raise exc_type('num_chains must be <= 2^24, not {}'.format(num_chains))
    if pseudocount is not None:
        opts['pseudocount'] = float(pseudocount)
        if not (0.0 < opts['pseudocount'] <= 1.0):
            raise exc_type('pseudocount must lie in (0, 1], not {!r}'.format(pseudocount))
    return opts


def profile_fields(X, weights, q, pseudocount=None):
    """h0 = log((1 - lambda) f + lambda / q) of the weighted single-site frequencies f of the alignment X (codes, N x L) with
    weights w: f_i(a) = sum_n w_n [X_ni = a] / Meff, Meff = sum_n w_n; lambda = pseudocount, or 1 / Meff -> float64[L, q]."""
    X = np.asarray(X)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    meff = float(w.sum())
    lam = 1.0 / meff if pseudocount is None else float(pseudocount)
    f = np.stack([(w[:, None] * (X == a)).sum(axis=0) for a in range(q)], axis=1) / meff
    return np.log((1.0 - lam) * f + lam / q)


def ais_base(base, X, weights, L, q, pseudocount, exc_type):
    """base of compute_log_partition_function: 'profile' (the training profile, profile_fields), 'fields' (None: the model's own
    fields) or an L x q array of finite values -> float64[L, q] or None."""
    if isinstance(base, str):
        if base == 'profile':
            h0 = profile_fields(X, weights, q, pseudocount)
        elif base == 'fields':
            return None
        else:
            raise exc_type("base must be 'profile', 'fields' or an L x q array, not {!r}".format(base))
    else:
        h0 = base
    try:
        return _lib.ais_base_fields(h0, L, q)
    except ValueError as exc:
        raise exc_type(str(exc))


def log_partition_function(run_ais, opts, base_fields):
    """run_ais(n, K, s, seed, h0) -> (log weights, log Z0, _) of the context's AIS entry; -> the dict of
    compute_log_partition_function."""
    logw, log_z0, _ = run_ais(opts['num_chains'], opts['num_temperatures'], opts['sweeps_per_temperature'], opts['seed'], base_fields)
    log_z, ess, stderr = _lib.ais_estimate(logw, log_z0)
    return {'log_z': log_z, 'log_z_stderr': stderr, 'ess': ess, 'log_z_base': log_z0, 'log_weights': logw}


def log_likelihood(energies, weights, meff, log_z):
    """(sum_n w_n E(s_n)) / Meff - log Z"""
    return float(np.dot(np.asarray(weights, dtype=np.float64), np.asarray(energies, dtype=np.float64))) / float(meff) - float(log_z)


POTTS_SUBCOMMANDS = ('compute_energies', 'compute_mutation_effects', 'sample_sequences', 'compute_log_likelihood',
                     'compute_pseudo_log_likelihood', 'compare_sequences', 'compute_pca', 'sample_conditional', 'find_local_maxima',
                     'sample_tempered', 'compute_interaction_energies')


def pll_flag(per_site, exc_type):
    """per_site of compute_sequence_pseudo_log_likelihoods: a bool (host check, before any device work)."""
    if not isinstance(per_site, (bool, np.bool_)):
        raise exc_type('per_site must be True or False, not {!r}'.format(per_site))
    return bool(per_site)


def single_query(sequences, exc_type):
    """sequences of compute_conditional_log_probabilities -> True for one aligned string (the result drops its first axis),
    False for a FASTA path or a list of aligned strings."""
    if sequences is None:
        raise exc_type('compute_conditional_log_probabilities needs sequences: an aligned string, a list of them or a FASTA file')
    return isinstance(sequences, str) and not os.path.isfile(sequences)


def pseudo_log_likelihood(plls, weights, meff):
    """(sum_n w_n PLL(s_n)) / Meff"""
    return float(np.dot(np.asarray(weights, dtype=np.float64), np.asarray(plls, dtype=np.float64))) / float(meff)


def ascent_options(free_sites, fixed_sites, max_steps, min_gain, L, exc_type):
    """Checks the arguments of find_local_maxima (host only) -> (free sites int32[F] ascending, max_steps, min_gain).  With
    neither site argument every site is free; max_steps None means 4 F."""
    if free_sites is None and fixed_sites is None:
        sites = np.arange(L, dtype=np.int32)
    else:
        sites = conditional_sites(free_sites, fixed_sites, L, exc_type)
    if max_steps is None:
        max_steps = 4 * int(sites.size)
    elif isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or int(max_steps) < 0:
        raise exc_type('max_steps must be an integer >= 0 or None, not {!r}'.format(max_steps))
    try:
        gain = float(min_gain)
    except (TypeError, ValueError):
        raise exc_type('min_gain must be a finite number >= 0, not {!r}'.format(min_gain))
    if not (0.0 <= gain < float('inf')):
        raise exc_type('min_gain must be a finite number >= 0, not {!r}'.format(min_gain))
    return sites, int(max_steps), gain


def basins(codes, converged, energies):
    """The distinct final rows among the converged chains -> (maxima uint8[M, L], basin int64[n]: each chain's index into them or
    -1 when unconverged, basin_sizes int64[M]).  The distinct rows come from np.unique over rows and
    are ordered by descending energy, then lexicographic codes."""
    codes = np.asarray(codes, dtype=np.uint8)
    converged = np.asarray(converged, dtype=bool)
    energies = np.asarray(energies, dtype=np.float64)
    basin = np.full(codes.shape[0], -1, dtype=np.int64)
    idx = np.flatnonzero(converged)
    if idx.size == 0:
        return codes[:0].copy(), basin, np.zeros(0, dtype=np.int64)
    rows, first, inverse, counts = np.unique(codes[idx], axis=0, return_index=True, return_inverse=True, return_counts=True)
    e = energies[idx][first]
    order = np.argsort(-e, kind='stable')                      # np.unique's rows are lexicographic: the stable sort keeps that among ties
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    basin[idx] = rank[np.asarray(inverse).reshape(-1)]
    return rows[order], basin, counts[order].astype(np.int64)


def group_species(labels):
    """species labels (arbitrary hashables, one per row) -> (species in order of first appearance, their row-index arrays);
    stable: a species' rows keep their order"""
    order, rows = [], {}
    for k, s in enumerate(labels):
        if s not in rows:
            rows[s] = []
            order.append(s)
        rows[s].append(k)
    return order, [np.asarray(rows[s], dtype=np.int64) for s in order]


def species_blocks(species_a, species_b, nA, nB, exc_type):
    """-> (species present on both sides, rows_a, rows_b, species dropped because one side lacks them); None, None: one block
    of all rows"""
    if species_a is None and species_b is None:
        return [None], [np.arange(nA, dtype=np.int64)], [np.arange(nB, dtype=np.int64)], []
    if species_a is None or species_b is None:
        raise exc_type('give the species labels of both proteins or of neither')
    species_a, species_b = list(species_a), list(species_b)
    if len(species_a) != nA or len(species_b) != nB:
        raise exc_type('{} and {} species labels for {} and {} sequences'.format(len(species_a), len(species_b), nA, nB))
    order_a, rows_a = group_species(species_a)
    order_b, rows_b = group_species(species_b)
    in_b = dict(zip(order_b, rows_b))
    in_a = set(order_a)
    both = [s for s in order_a if s in in_b]
    dropped = [s for s in order_a if s not in in_b] + [s for s in order_b if s not in in_a]
    return both, [r for s, r in zip(order_a, rows_a) if s in in_b], [in_b[s] for s in both], dropped


def grouped_rows(XA, XB, rows_a, rows_b):
    """the rows of every species gathered side by side -> (XA', XB', offsets_a, offsets_b)"""
    ia = np.concatenate(rows_a) if rows_a else np.zeros(0, dtype=np.int64)
    ib = np.concatenate(rows_b) if rows_b else np.zeros(0, dtype=np.int64)
    oa = np.concatenate([[0], np.cumsum([len(r) for r in rows_a])]).astype(np.int32)
    ob = np.concatenate([[0], np.cumsum([len(r) for r in rows_b])]).astype(np.int32)
    return np.ascontiguousarray(XA[ia]), np.ascontiguousarray(XB[ib]), oa, ob


def rank_matches(blocks, rows_a, rows_b, species):
    """dca_assign_partners on every species' block -> the assigned pairs of all species ranked by gap (descending; equal gaps in
    ascending A index): dict of pairs int64[n, 2] (A row, B row), energies, gaps float64[n], species (list)"""
    found = []
    for E, ra, rb, s in zip(blocks, rows_a, rows_b, species):
        cols, _total, gaps = _lib.assign_partners(E)
        found += [(int(ra[k]), int(rb[cols[k]]), float(E[k, cols[k]]), float(gaps[k]), s) for k in range(len(ra)) if cols[k] >= 0]
    found.sort(key=lambda t: (-t[3], t[0]))
    return dict(pairs=np.array([(t[0], t[1]) for t in found], dtype=np.int64).reshape(-1, 2),
                energies=np.array([t[2] for t in found], dtype=np.float64), gaps=np.array([t[3] for t in found], dtype=np.float64),
                species=[t[4] for t in found])


class PottsModel:
    """The fitted model of PlmDCA and MeanFieldDCA as a sequence model: energies, single-mutant effects, Gibbs samples, log Z and
    pseudo-log-likelihoods, local maxima, replica exchange (DESIGN.md sections 11, 12, 14, 15, 23, 24 and 25; no reference counterpart).  E includes the gap state for PlmDCA
    (after fit_boltzmann: the refined model); under MeanFieldDCA couplings and fields are zero on the gap state, and the
    couplings of the current pseudocount are computed first if none are there yet.

    A class supplies: _potts_exc (its exception type), _potts_table (residue table of the encoder: 0 plm, 1 mf),
    _potts_dims() -> (biomolecule code, L, q), _potts_default_source() (the training file or alignment), _potts_devices(),
    _potts_training() -> (X, weights, meff) of the fit, and _potts_call(name, *args, **kw), which runs Context.plm_<name> /
    Context.mf_<name> on the fitted model."""

    def _query(self, sequences):
        bio, L, _q = self._potts_dims()
        src = self._potts_default_source() if sequences is None else sequences
        return query_codes(src, bio, L, self._potts_table, self._potts_exc)

    def _one_gpu(self, what):
        devices = self._potts_devices()
        if devices and len(devices) > 1:
            self._potts_logger.error('\n\t{} runs on one GPU; devices={}'.format(what, devices))
            raise self._potts_exc('{} runs on one GPU, not on devices {}'.format(what, devices))

    def compute_sequence_energies(self, sequences=None):
        """Statistical energies E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j) of the fitted parameters -> float64[n], higher
        is more probable.  sequences: None (every record of the training alignment, in file order, duplicates kept), a FASTA
        path or a list of aligned strings."""
        X = self._query(sequences)
        self._potts_logger.info('\n\tStatistical energies of {} sequences'.format(X.shape[0]))
        return self._potts_call('energies', X)

    def _interaction_inputs(self, sequences_a, sequences_b, split, species_a, species_b, gauge):
        bio, L, _q = self._potts_dims()
        split = operator.index(split)
        if not 1 <= split <= L - 1:
            raise self._potts_exc('split must lie in [1, {}], not {}'.format(L - 1, split))
        if gauge not in _lib.GAUGES:
            raise self._potts_exc('gauge must be one of {}'.format(sorted(_lib.GAUGES)))
        XA = query_codes(sequences_a, bio, split, self._potts_table, self._potts_exc)
        XB = query_codes(sequences_b, bio, L - split, self._potts_table, self._potts_exc)
        species, rows_a, rows_b, dropped = species_blocks(species_a, species_b, XA.shape[0], XB.shape[0], self._potts_exc)
        if dropped:
            self._potts_logger.warning('\n\tSpecies on one side only are left out: {}'.format(dropped))
        return split, XA, XB, species, rows_a, rows_b, dropped

    def compute_interaction_energies(self, sequences_a, sequences_b, split, species_a=None, species_b=None, gauge='zero_sum'):
        """Inter-protein interaction energies under a model fitted on a concatenated alignment: sites [0, split) are protein A,
        the rest protein B; E(m, n) = sum over A sites i and B sites j of J_ij(a^m_i, b^n_j), no fields, higher is more
        favourable.  sequences_a / sequences_b: FASTA paths or lists of aligned strings of lengths split and L - split (nothing
        is de-duplicated).  gauge: 'zero_sum' (the couplings' zero-sum form over all states) or 'as_stored'.
        Without species labels -> float64[nA, nB], all against all.  With one label per sequence (arbitrary hashables) -> a
        dict: species (in order of first appearance, those present on both sides), rows_a / rows_b (their row indices, in
        order), energies (one float64[nA_s, nB_s] per species) and dropped (species on one side only)."""
        self._one_gpu('compute_interaction_energies')
        split, XA, XB, species, rows_a, rows_b, dropped = self._interaction_inputs(sequences_a, sequences_b, split, species_a,
                                                                                      species_b, gauge)
        self._potts_logger.info('\n\tInteraction energies of {} x {} sequences in {} blocks'.format(XA.shape[0], XB.shape[0], len(species)))
        if species == [None]:
            return self._potts_call('interaction_energies', XA, XB, split, gauge=gauge)
        GA, GB, oa, ob = grouped_rows(XA, XB, rows_a, rows_b)
        blocks = self._potts_call('interaction_energies', GA, GB, split, oa, ob, gauge=gauge)
        return dict(species=species, rows_a=rows_a, rows_b=rows_b, energies=blocks, dropped=dropped)

    def match_partners(self, sequences_a, sequences_b, split, species_a=None, species_b=None, gauge='zero_sum'):
        """Pairs every A sequence with a B sequence of its species: one maximum-weight assignment of the interaction energies per
        species (compute_interaction_energies; dca_assign_partners).  -> dict: pairs int64[n, 2] (A row, B row), energies and
        gaps float64[n] (the loss in a species' total when the pair is forbidden; +inf in a 1 x 1 species), species (per pair),
        ranked by gap (descending; equal gaps in ascending A index), and dropped."""
        self._one_gpu('match_partners')
        split, XA, XB, species, rows_a, rows_b, dropped = self._interaction_inputs(sequences_a, sequences_b, split, species_a,
                                                                                      species_b, gauge)
        GA, GB, oa, ob = grouped_rows(XA, XB, rows_a, rows_b)
        blocks = self._potts_call('interaction_energies', GA, GB, split, oa, ob, gauge=gauge)
        res = rank_matches(blocks, rows_a, rows_b, species)
        res['dropped'] = dropped
        return res

    def compute_single_mutant_effects(self, wildtype):
        """dE(i, a) = E(wildtype with site i set to state a) - E(wildtype) for every site and state (gap last)
        -> float64[L, q]; dE(i, w_i) = 0.  wildtype: an aligned string of length L or a FASTA file with one record."""
        bio, L, _q = self._potts_dims()
        w = wildtype_codes(wildtype, bio, L, self._potts_table, self._potts_exc)
        self._potts_logger.info('\n\tSingle-mutant effects of the wild type')
        return self._potts_call('mutation_scan', w)

    def sample_sequences(self, num_sequences, num_sweeps=1000, seed=0, temperature=1.0, initial=None, return_codes=False):
        """Draws num_sequences sequences from P(s) ~ exp(E(s) / temperature) by systematic-scan Gibbs sampling on the GPU:
        one independent chain per sequence, num_sweeps sweeps over all sites (E as in compute_sequence_energies).
        initial: None (random starts), an aligned string (every chain starts from it), a list of num_sequences aligned
        strings, or a FASTA file with 1 or num_sequences records.  The draws follow a counter-based generator of `seed`:
        the same arguments give the same sequences.  -> aligned strings (gap '-'), or uint8[n, L] codes with
        return_codes."""
        n = int(num_sequences)
        beta = sampling_beta(temperature, self._potts_exc)
        bio, L, _q = self._potts_dims()
        X0 = initial_codes(initial, n, bio, L, self._potts_table, self._potts_exc)
        self._potts_logger.info('\n\tGibbs sampling of {} sequences, {} sweeps'.format(n, num_sweeps))
        codes = self._potts_call('sample', n, num_sweeps, seed=seed, beta=beta, initial=X0)
        if return_codes:
            return codes
        letters = state_letters(bio)
        return [''.join(letters[c] for c in row) for row in codes]

    def sample_sequences_conditional(self, template, free_sites=None, fixed_sites=None, num_sequences=None, num_sweeps=1000, seed=0,
                                     temperature=1.0, randomize=True, return_codes=False):
        """Draws sequences from P(s_free | s_fixed) ~ exp(E(s) / temperature) by systematic-scan Gibbs sampling over the free
        sites only: every other site keeps the template's residue.  template: an aligned string, a list
        of aligned strings or a FASTA file with 1 or num_sequences records (one record is replicated; num_sequences defaults
        to the number of records), so every chain can carry its own background.  Exactly one of free_sites and fixed_sites
        (iterables of 0-based site indices, any order) says which sites are redrawn.  randomize: the free sites start from
        random residues (the plain sampler's start at those sites) instead of the template's.  A sweep reads (F / L)^2 of a
        full one's couplings for F free sites.  -> aligned strings (gap '-'), or uint8[n, L] codes with return_codes."""
        beta = sampling_beta(temperature, self._potts_exc)
        bio, L, _q = self._potts_dims()
        sites = conditional_sites(free_sites, fixed_sites, L, self._potts_exc)
        self._one_gpu('sample_sequences_conditional')
        X0 = template_codes(template, num_sequences, bio, L, self._potts_table, self._potts_exc)
        self._potts_logger.info('\n\tConditional Gibbs sampling of {} sequences, {} free sites of {}, {} sweeps'.format(
            X0.shape[0], sites.size, L, num_sweeps))
        codes = self._potts_call('sample_conditional', X0, sites, num_sweeps, seed=seed, beta=beta, random_start=bool(randomize))
        if return_codes:
            return codes
        letters = state_letters(bio)
        return [''.join(letters[c] for c in row) for row in codes]

    def sample_sequences_tempered(self, num_sequences, temperatures, num_sweeps=1000, swap_interval=1, seed=0, initial=None,
                                  burn_in_sweeps=None, return_codes=False):
        """Draws num_sequences sequences at every temperature of a ladder by replica-exchange (parallel-tempering) Gibbs sampling
        on the GPU: num_sequences independent ladders, each with one walker per distinct temperature;
        every walker does the sweep of sample_sequences under its current temperature, and after every swap_interval sweeps
        walkers at neighbouring temperatures exchange temperatures by the Metropolis rule, so that the cold samples inherit the
        mixing of the hot ones (swap_interval 0: no exchange, independent chains).  temperatures: finite values > 0, or inf
        (beta = 0), in any order; the result follows that order.  initial: as in sample_sequences; record m starts every walker
        of ladder m.  burn_in_sweeps (None: num_sweeps // 2): the exchange rounds up to that sweep are left out of the averages.
        -> {'temperatures', 'sequences' (per temperature num_sequences aligned strings, or uint8[n, L] codes with return_codes:
        the walkers sitting at that temperature at the end, in ladder order), 'energies' (float64[T, n], E of those sequences),
        'swap_acceptance' (float64[R - 1], between neighbours of the ladder in ascending beta over the R distinct temperatures;
        NaN where nothing was attempted), 'swap_attempts', 'mean_energy' and 'heat_capacity' (float64[T]: <E> and
        C = beta^2 Var E over all ladders and the rounds past burn-in, NaN without such rounds), 'num_rounds'}."""
        opts = tempered_options(num_sequences, temperatures, num_sweeps, swap_interval, seed, burn_in_sweeps, self._potts_exc)
        self._one_gpu('sample_sequences_tempered')
        bio, L, _q = self._potts_dims()
        n, R = opts['n'], opts['betas'].size
        X0 = initial_codes(initial, n, bio, L, self._potts_table, self._potts_exc)
        self._potts_logger.info('\n\tReplica-exchange Gibbs sampling: {} ladders of {} temperatures, {} sweeps, exchange every {}'.format(
            n, R, opts['num_sweeps'], opts['swap_interval']))
        res = self._potts_call('sample_tempered', n, opts['betas'], opts['num_sweeps'], swap_interval=opts['swap_interval'],
                               seed=opts['seed'], initial=None if X0 is None else np.repeat(X0, R, axis=0), trace=True)
        letters = state_letters(bio)

        def text(codes):
            return np.ascontiguousarray(codes) if return_codes else [''.join(letters[c] for c in row) for row in codes]
        return tempered_result(opts, res, text)

    def find_local_maxima(self, sequences=None, free_sites=None, fixed_sites=None, max_steps=None, min_gain=0.0, return_paths=False):
        """Greedy ascent of every sequence to a local maximum of E (as in compute_sequence_energies) on the GPU: a chain
        repeatedly applies the single mutation of a free site with the largest gain in E (ties: the smallest site, then the
        smallest state) until none gains more than min_gain or max_steps moves are made.  sequences: as
        in compute_sequence_energies (None: the training alignment's rows).  free_sites / fixed_sites: as in
        sample_sequences_conditional, at most one of them; with neither, every site is free.  max_steps None: 4 F.
        -> {'sequences' (aligned strings), 'energies', 'start_energies' (float64[n], of compute_sequence_energies), 'num_steps',
        'converged', 'gains' (the summed gains of the applied moves), 'maxima' (the distinct final sequences among the converged
        chains, by descending energy, then codes), 'basin' (each chain's index into maxima, -1 when unconverged),
        'basin_sizes'} and, with return_paths, 'paths': per chain a list of (site, letter, gain)."""
        bio, L, _q = self._potts_dims()
        sites, max_steps, min_gain = ascent_options(free_sites, fixed_sites, max_steps, min_gain, L, self._potts_exc)
        self._one_gpu('find_local_maxima')
        X = self._query(sequences)
        self._potts_logger.info('\n\tGreedy ascent of {} sequences, {} free sites of {}, at most {} steps'.format(
            X.shape[0], sites.size, L, max_steps))
        res = self._potts_call('ascend', X, sites, max_steps=max_steps, min_gain=min_gain, paths=bool(return_paths))
        codes = res['codes']
        energies = self._potts_call('energies', codes)
        start = self._potts_call('energies', X)
        maxima, basin, sizes = basins(codes, res['converged'], energies)
        letters = state_letters(bio)

        def text(rows):
            return [''.join(letters[c] for c in row) for row in rows]
        out = {'sequences': text(codes), 'energies': energies, 'start_energies': start, 'num_steps': res['steps'],
               'converged': res['converged'], 'gains': res['gains'], 'maxima': text(maxima), 'basin': basin,
               'basin_sizes': sizes}
        if return_paths:
            out['paths'] = [[(int(res['path'][k, t, 0]), letters[res['path'][k, t, 1]], float(res['path_gains'][k, t]))
                             for t in range(int(res['steps'][k]))] for k in range(codes.shape[0])]
        return out

    def compute_log_partition_function(self, num_chains=1000, num_temperatures=1000, sweeps_per_temperature=1, seed=0, base='profile',
                                       pseudocount=None):
        """log Z = log sum_s exp(E(s)) of the fitted model (E as in compute_sequence_energies) by annealed importance sampling
        on the GPU: num_chains chains start from the independent-site base model and anneal through beta_k = k / K
        (K = num_temperatures) with sweeps_per_temperature Gibbs sweeps per intermediate temperature.  base: 'profile' (log of
        the training alignment's weighted single-site frequencies, regularised by (1 - lambda) f + lambda / q, lambda =
        pseudocount or 1 / Meff), 'fields' (the model's own fields) or an L x q array.
        -> {'log_z', 'log_z_stderr', 'ess', 'log_z_base', 'log_weights'}"""
        self._one_gpu('compute_log_partition_function')
        opts = ais_options(num_chains, num_temperatures, sweeps_per_temperature, seed, pseudocount, self._potts_exc)
        _bio, L, q = self._potts_dims()
        X, weights, _meff = self._potts_training() if isinstance(base, str) and base == 'profile' else (None, None, None)
        h0 = ais_base(base, X, weights, L, q, opts['pseudocount'], self._potts_exc)
        self._potts_logger.info('\n\tlog Z by annealed importance sampling: {} chains, {} temperatures, {} sweeps per temperature'.format(
            opts['num_chains'], opts['num_temperatures'], opts['sweeps_per_temperature']))
        return log_partition_function(
            lambda n, K, s, sd, h: self._potts_call('ais', n, K, sweeps_per_temperature=s, seed=sd, base_fields=h), opts, h0)

    def compute_sequence_log_probabilities(self, sequences=None, log_z=None, **ais_kwargs):
        """log P(s) = E(s) - log Z -> float64[n] (sequences as in compute_sequence_energies).  log_z None: estimated first by
        compute_log_partition_function(**ais_kwargs)."""
        self._one_gpu('compute_sequence_log_probabilities')
        if log_z is None:
            log_z = self.compute_log_partition_function(**ais_kwargs)['log_z']
        return self.compute_sequence_energies(sequences) - float(log_z)

    def compute_log_likelihood(self, log_z=None, **ais_kwargs):
        """(sum_n w_n E(s_n)) / Meff - log Z over the alignment and weights of the fit -> float.  log_z None: estimated first
        by compute_log_partition_function(**ais_kwargs)."""
        self._one_gpu('compute_log_likelihood')
        if log_z is None:
            log_z = self.compute_log_partition_function(**ais_kwargs)['log_z']
        X, weights, meff = self._potts_training()
        return log_likelihood(self._potts_call('energies', X), weights, meff, log_z)

    def compute_sequence_pseudo_log_likelihoods(self, sequences=None, per_site=False):
        """PLL(s) = sum_i log P(s_i | s_-i) of the fitted parameters, with log P(s_i = a | s_-i) = u_i(a) - log sum_b exp u_i(b),
        u_i(a) = h_i(a) + sum_{j != i} J_ij(a, s_j) -> float64[n], or (float64[n], float64[n, L] of log P(s_i | s_-i)) with
        per_site.  sequences: as in compute_sequence_energies.  This is the true pseudo-log-likelihood, not the fx a PlmDCA fit
        reports: under the reference's carry-over of the gradient the fit's objective differs from it by
        design."""
        per_site = pll_flag(per_site, self._potts_exc)
        self._one_gpu('compute_sequence_pseudo_log_likelihoods')
        X = self._query(sequences)
        self._potts_logger.info('\n\tPseudo-log-likelihoods of {} sequences'.format(X.shape[0]))
        return self._potts_call('pseudo_likelihood', X, per_site=per_site)

    def compute_conditional_log_probabilities(self, sequences):
        """log P(s_i = a | s_-i) for every site i and state a (gap last) of each sequence (as in
        compute_sequence_pseudo_log_likelihoods) -> float64[n, L, q], or float64[L, q] for a single aligned string.
        sequences: an aligned string, a list of aligned strings or a FASTA path."""
        single = single_query(sequences, self._potts_exc)
        self._one_gpu('compute_conditional_log_probabilities')
        X = self._query([sequences] if single else sequences)
        _pll, cond = self._potts_call('pseudo_likelihood', X, conditionals=True)
        return cond[0] if single else cond

    def compute_pseudo_log_likelihood(self):
        """(sum_n w_n PLL(s_n)) / Meff over the alignment and weights of the fit -> float: the unregularised
        pseudo-log-likelihood per effective sequence (compute_sequence_pseudo_log_likelihoods), comparable with
        compute_log_likelihood.  Not a PlmDCA fit's reported fx."""
        self._one_gpu('compute_pseudo_log_likelihood')
        X, weights, meff = self._potts_training()
        return pseudo_log_likelihood(self._potts_call('pseudo_likelihood', X), weights, meff)


def add_sampling_arguments(p):
    """The options of the sample_sequences sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--num_sequences', type=int, required=True, help='number of sequences (independent chains) to draw (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps over all sites per chain (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator (addition)')
    p.add_argument('--temperature', type=float, default=1.0, help='sampling temperature T, P(s) ~ exp(E(s) / T) (addition)')
    p.add_argument('--initial_file', help='FASTA file with 1 or num_sequences aligned starting sequences (default: random) (addition)')


def add_conditional_arguments(p):
    """The options of the sample_conditional sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--template_file', required=True, help='FASTA file with 1 or num_sequences aligned template sequences: the '
                   'sites that are not free keep its residues (addition)')
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument('--free_sites', help='sites to redraw, 1-based inclusive ranges such as 10-30,45 (addition)')
    g.add_argument('--fixed_sites', help='sites to keep, in the same notation; every other site is redrawn (addition)')
    p.add_argument('--num_sequences', type=int, help='number of sequences (default: the records of template_file) (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps over the free sites per chain (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator (addition)')
    p.add_argument('--temperature', type=float, default=1.0, help='sampling temperature T, P(s) ~ exp(E(s) / T) (addition)')
    p.add_argument('--keep_template_start', action='store_true', help='start the free sites from the template instead of from '
                   'random residues (addition)')


CONDITIONAL_OPTIONS = ('template_file', 'free_sites', 'fixed_sites', 'num_sequences', 'num_sweeps', 'seed', 'temperature',
                       'keep_template_start')


def run_sample_conditional(instance, prefix, msa_file, output_dir, biomolecule, exc_type, opts):
    """sample_conditional of the plmdca and mfdca command lines -> the path of <output_dir>/<prefix>_conditional_samples_
    <alignment base>.fa: '#' lines that name the free sites (1-based), then the records of sample_sequences."""
    from .dca_utilities import dca_utilities
    opts = dict(opts or {})
    if not opts.get('template_file'):
        raise exc_type('sample_conditional needs --template_file')
    if (opts.get('free_sites') is None) == (opts.get('fixed_sites') is None):
        raise exc_type('sample_conditional needs exactly one of --free_sites and --fixed_sites')
    which = 'free_sites' if opts.get('free_sites') is not None else 'fixed_sites'
    sites = {which: parse_site_ranges(opts[which], exc_type)}

    def opt(name, default):
        return default if opts.get(name) is None else opts[name]
    L = int(instance.sequences_len)
    free = conditional_sites(sites.get('free_sites'), sites.get('fixed_sites'), L, exc_type)
    dca_utilities.create_directories(output_dir)
    codes = instance.sample_sequences_conditional(opts['template_file'], num_sequences=opts.get('num_sequences'),
                                                  num_sweeps=opt('num_sweeps', 1000), seed=opt('seed', 0),
                                                  temperature=opt('temperature', 1.0), randomize=not opts.get('keep_template_start'),
                                                  return_codes=True, **sites)
    letters = state_letters(biomolecule)
    seqs = [''.join(letters[c] for c in row) for row in codes]
    energies = instance.compute_sequence_energies(seqs) if seqs else []
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_conditional_samples_', postfix='.fa')
    header = ['# Conditional Gibbs samples: template {}, {} free sites of {}'.format(opts['template_file'], free.size, L),
              '# Free sites (1-based): {}'.format(','.join(str(int(i) + 1) for i in free))]
    dca_utilities.write_sampled_sequences(path, seqs, energies, header=header)
    return path


def add_tempered_arguments(p):
    """The options of the sample_tempered sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--num_sequences', type=int, required=True, help='sequences per temperature (independent ladders) (addition)')
    p.add_argument('--temperatures', required=True, help='the ladder, comma separated, such as 0.5,0.7,1,1.5 (inf allowed) (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps over all sites per walker (addition)')
    p.add_argument('--swap_interval', type=int, default=1, help='sweeps between exchange rounds; 0: no exchange (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator (addition)')
    p.add_argument('--initial_file', help='FASTA file with 1 or num_sequences aligned starting sequences (default: random) (addition)')


TEMPERED_OPTIONS = ('num_sequences', 'temperatures', 'num_sweeps', 'swap_interval', 'seed', 'initial_file')


def parse_temperatures(text, exc_type):
    """'0.5,0.7,1,1.5' -> [0.5, 0.7, 1.0, 1.5] ('inf' allowed; tempered_options checks the values)."""
    try:
        return [float(part) for part in str(text).split(',')]
    except ValueError:
        raise exc_type('temperatures are written like 0.5,0.7,1,1.5, not {!r}'.format(text))


def run_sample_tempered(instance, prefix, msa_file, output_dir, metadata, biomolecule, exc_type, opts):
    """sample_tempered of the plmdca and mfdca command lines -> the paths of <output_dir>/<prefix>_tempered_samples_<alignment
    base>.fa (per temperature, then per sample: a record whose name carries both and the energy) and <prefix>_tempered_sampling_
    <alignment base>.txt (one row per temperature: T, mean energy, heat capacity, acceptance to the next colder temperature)."""
    from .dca_utilities import dca_utilities
    opts = dict(opts or {})
    if opts.get('num_sequences') is None or opts.get('temperatures') is None:
        raise exc_type('sample_tempered needs --num_sequences and --temperatures')

    def opt(name, default):
        return default if opts.get(name) is None else opts[name]
    temps = parse_temperatures(opts['temperatures'], exc_type)
    dca_utilities.create_directories(output_dir)
    res = instance.sample_sequences_tempered(opts['num_sequences'], temps, num_sweeps=opt('num_sweeps', 1000),
                                             swap_interval=opt('swap_interval', 1), seed=opt('seed', 0),
                                             initial=opts.get('initial_file'), return_codes=True)
    letters = state_letters(biomolecule)
    seqs = [[''.join(letters[c] for c in row) for row in codes] for codes in res['sequences']]
    # each temperature's level on the ladder of distinct temperatures (descending T is ascending beta), then its acceptance
    t = np.asarray(res['temperatures'], dtype=np.float64)
    level = np.asarray(np.unique(-t, return_inverse=True)[1]).reshape(-1)
    acc = np.append(np.asarray(res['swap_acceptance'], dtype=np.float64), np.nan)
    fa = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_tempered_samples_', postfix='.fa')
    txt = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_tempered_sampling_', postfix='.txt')
    dca_utilities.write_tempered_samples(fa, res['temperatures'], seqs, res['energies'])
    dca_utilities.write_tempered_summary(txt, res, acc[level], metadata=metadata)
    return fa, txt


def add_ascent_arguments(p):
    """The options of the find_local_maxima sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--query_file', help='FASTA file of aligned starting sequences (default: the records of msa_file) (addition)')
    g = p.add_mutually_exclusive_group()
    g.add_argument('--free_sites', help='sites that may mutate, 1-based inclusive ranges such as 10-30,45 (default: all) (addition)')
    g.add_argument('--fixed_sites', help='sites to keep, in the same notation; every other site may mutate (addition)')
    p.add_argument('--max_steps', type=int, help='moves per sequence at most (default: 4 x the number of free sites) (addition)')
    p.add_argument('--min_gain', type=float, default=0.0, help='a move must gain more than this in E (addition)')


ASCENT_OPTIONS = ('free_sites', 'fixed_sites', 'max_steps', 'min_gain')


def run_find_local_maxima(instance, prefix, msa_file, output_dir, metadata, exc_type, query_file, opts):
    """find_local_maxima of the plmdca and mfdca command lines -> the paths of <output_dir>/<prefix>_local_maxima_<alignment
    base>.fa (the final sequences; a record's name carries its start record and its energy) and <prefix>_local_maxima_
    <alignment base>.txt (one line per input: start energy, final energy, steps, converged, basin)."""
    from .dca_utilities import dca_utilities
    opts = dict(opts or {})
    if opts.get('free_sites') is not None and opts.get('fixed_sites') is not None:
        raise exc_type('find_local_maxima takes at most one of --free_sites and --fixed_sites')
    sites = {k: parse_site_ranges(opts[k], exc_type) for k in ('free_sites', 'fixed_sites') if opts.get(k) is not None}
    dca_utilities.create_directories(output_dir)
    res = instance.find_local_maxima(query_file, max_steps=opts.get('max_steps'),
                                     min_gain=0.0 if opts.get('min_gain') is None else opts['min_gain'], **sites)
    fa = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_local_maxima_', postfix='.fa')
    txt = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_local_maxima_', postfix='.txt')
    dca_utilities.write_local_maxima_sequences(fa, res['sequences'], res['energies'])
    dca_utilities.write_local_maxima(txt, res, metadata=metadata, query_file=query_file or msa_file)
    return fa, txt


def add_interaction_arguments(p):
    """The options of the compute_interaction_energies sub-command (plmdca and mfdca command lines): msa_file is the
    concatenated alignment the model is fitted on."""
    p.add_argument('--query_file_a', required=True, help='FASTA file of aligned protein-A sequences (addition)')
    p.add_argument('--query_file_b', required=True, help='FASTA file of aligned protein-B sequences (addition)')
    p.add_argument('--split', type=int, required=True, help='number of protein-A sites: the first --split columns of msa_file (addition)')
    p.add_argument('--species_a', help='file with one species label per record of --query_file_a, in file order (addition)')
    p.add_argument('--species_b', help='the same for --query_file_b (addition)')
    p.add_argument('--gauge', choices=sorted(_lib.GAUGES), default='zero_sum', help='gauge of the inter-protein couplings (addition)')


INTERACTION_OPTIONS = ('query_file_a', 'query_file_b', 'split', 'species_a', 'species_b', 'gauge')


def read_labels(path):
    """one label per non-empty line"""
    with open(path) as fh:
        return [ln.strip() for ln in fh if ln.strip()]


def run_interaction_energies(instance, prefix, msa_file, output_dir, metadata, exc_type, opts):
    """compute_interaction_energies of the plmdca and mfdca command lines -> the path of <output_dir>/<prefix>_interaction_energies_
    <alignment base>.txt: one line per within-species pair (A record, B record, 1-based, species, energy)."""
    from .dca_utilities import dca_utilities
    opts = dict(opts or {})
    for k in ('query_file_a', 'query_file_b', 'split'):
        if opts.get(k) is None:
            raise exc_type('compute_interaction_energies needs --{}'.format(k))
    if (opts.get('species_a') is None) != (opts.get('species_b') is None):
        raise exc_type('give both --species_a and --species_b or neither')
    sa = read_labels(opts['species_a']) if opts.get('species_a') else None
    sb = read_labels(opts['species_b']) if opts.get('species_b') else None
    gauge = opts.get('gauge') or 'zero_sum'
    res = instance.compute_interaction_energies(opts['query_file_a'], opts['query_file_b'], opts['split'], sa, sb, gauge=gauge)
    if sa is None:
        res = dict(species=['all'], rows_a=[np.arange(res.shape[0])], rows_b=[np.arange(res.shape[1])], energies=[res], dropped=[])
    dca_utilities.create_directories(output_dir)
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_interaction_energies_', postfix='.txt')
    with open(path, 'w') as fh:
        fh.write('# Inter-protein interaction energies ({} gauge); split {}\n'.format(gauge, opts['split']))
        for line in metadata or []:
            fh.write('{}\n'.format(line))
        fh.write('# A records: {}\n# B records: {}\n'.format(opts['query_file_a'], opts['query_file_b']))
        if res['dropped']:
            fh.write('# Species on one side only (left out): {}\n'.format(', '.join(str(s) for s in res['dropped'])))
        fh.write('# A record\tB record\tspecies\tenergy\n')
        for s, ra, rb, E in zip(res['species'], res['rows_a'], res['rows_b'], res['energies']):
            for k, a in enumerate(ra):
                for l, b in enumerate(rb):
                    fh.write('{}\t{}\t{}\t{!r}\n'.format(int(a) + 1, int(b) + 1, s, float(E[k, l])))
    return path


def add_ais_arguments(p):
    """The options of the compute_log_likelihood sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--num_chains', type=int, default=1000, help='AIS chains (addition)')
    p.add_argument('--num_temperatures', type=int, default=1000, help='K, annealing steps beta_k = k / K (addition)')
    p.add_argument('--sweeps_per_temperature', type=int, default=1, help='Gibbs sweeps per intermediate temperature (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator (addition)')
    p.add_argument('--base', choices=('profile', 'fields'), default='profile',
                   help='base model: the training profile or the model\'s own fields (addition)')
    p.add_argument('--base_pseudocount', type=float, help='pseudocount of the profile base (default: 1 / Meff) (addition)')


AIS_OPTIONS = ('num_chains', 'num_temperatures', 'sweeps_per_temperature', 'seed', 'base', 'base_pseudocount')


def run_log_likelihood(instance, prefix, msa_file, output_dir, metadata, opts):
    """compute_log_likelihood of the plmdca and mfdca command lines -> the path of <output_dir>/<prefix>_log_likelihood_
    <alignment base>.txt: a header with log Z, its stderr, the ESS, log Z0 and the schedule, the average log-likelihood of the
    training alignment, then one log P(s) = E(s) - log Z per training record (file order)."""
    from .dca_utilities import dca_utilities
    opts = {k: v for k, v in dict(opts or {}).items() if v is not None}
    kw = dict(num_chains=opts.get('num_chains', 1000), num_temperatures=opts.get('num_temperatures', 1000),
              sweeps_per_temperature=opts.get('sweeps_per_temperature', 1), seed=opts.get('seed', 0), base=opts.get('base', 'profile'),
              pseudocount=opts.get('base_pseudocount'))
    dca_utilities.create_directories(output_dir)
    res = instance.compute_log_partition_function(**kw)
    ll = instance.compute_log_likelihood(log_z=res['log_z'])
    logp = instance.compute_sequence_log_probabilities(log_z=res['log_z'])
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_log_likelihood_', postfix='.txt')
    dca_utilities.write_log_likelihood(path, res, ll, logp, kw, metadata=metadata)
    return path


def run_subcommand(instance, the_command, prefix, msa_file, output_dir, metadata, biomolecule, table, exc_type,
                   query_file=None, wildtype_file=None, sampling=None, ais=None, three_site=0, three_site_no_gaps=False, pca=None,
                   conditional=None, ascent=None, tempered=None, interaction=None):
    """compute_energies / compute_mutation_effects / sample_sequences / compute_pseudo_log_likelihood / compare_sequences of the
    plmdca and mfdca command lines -> the path of the file written: <output_dir>/<prefix>_energies_<alignment base>.txt,
    <prefix>_mutation_effects_<alignment base>.txt, <prefix>_samples_<alignment base>.fa,
    <prefix>_pseudo_log_likelihoods_<alignment base>.txt or <prefix>_sequence_comparison_<alignment base>.txt; compute_pca -> the
    paths of _compare.run_pca (pca: its options num_components and seed, and the K of compare_sequences --pca).  sampling: the sample_sequences options (num_sequences, num_sweeps, seed,
    temperature, initial_file); conditional: the sample_conditional options (CONDITIONAL_OPTIONS; run_sample_conditional)."""
    from .dca_utilities import dca_utilities
    if the_command == 'compute_log_likelihood':
        return run_log_likelihood(instance, prefix, msa_file, output_dir, metadata, ais)
    if the_command == 'sample_conditional':
        return run_sample_conditional(instance, prefix, msa_file, output_dir, biomolecule, exc_type, conditional)
    if the_command == 'sample_tempered':        # tempered: its options (TEMPERED_OPTIONS; run_sample_tempered)
        return run_sample_tempered(instance, prefix, msa_file, output_dir, metadata, biomolecule, exc_type, tempered)
    if the_command == 'find_local_maxima':      # ascent: its options (ASCENT_OPTIONS; run_find_local_maxima)
        return run_find_local_maxima(instance, prefix, msa_file, output_dir, metadata, exc_type, query_file, ascent)
    if the_command == 'compute_interaction_energies':      # interaction: its options (INTERACTION_OPTIONS)
        return run_interaction_energies(instance, prefix, msa_file, output_dir, metadata, exc_type, interaction)
    if the_command == 'compare_sequences':
        from . import _compare
        return _compare.run_compare(instance, prefix, msa_file, output_dir, metadata, query_file, exc_type, three_site=int(three_site or 0),
                                    three_site_include_gaps=not three_site_no_gaps, pca=int((pca or {}).get('pca') or 0))
    if the_command == 'compute_pca':
        from . import _compare
        opts = dict(pca or {})
        return _compare.run_pca(instance, prefix, msa_file, output_dir, metadata, query_file=query_file,
                                num_components=opts.get('num_components'), seed=opts.get('seed'))
    dca_utilities.create_directories(output_dir)
    if the_command == 'sample_sequences':
        opts = dict(sampling or {})
        if opts.get('num_sequences') is None:
            raise exc_type('sample_sequences needs --num_sequences')

        def opt(name, default):
            return default if opts.get(name) is None else opts[name]
        codes = instance.sample_sequences(opts['num_sequences'], num_sweeps=opt('num_sweeps', 1000), seed=opt('seed', 0),
                                          temperature=opt('temperature', 1.0), initial=opts.get('initial_file'), return_codes=True)
        letters = state_letters(biomolecule)
        seqs = [''.join(letters[c] for c in row) for row in codes]
        energies = instance.compute_sequence_energies(seqs) if seqs else []
        path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_samples_', postfix='.fa')
        dca_utilities.write_sampled_sequences(path, seqs, energies)
        return path
    if the_command == 'compute_pseudo_log_likelihood':
        plls = instance.compute_sequence_pseudo_log_likelihoods(query_file)
        weighted = None if query_file else instance.compute_pseudo_log_likelihood()
        path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_pseudo_log_likelihoods_', postfix='.txt')
        dca_utilities.write_pseudo_log_likelihoods(path, plls, metadata=metadata, query_file=query_file or msa_file, weighted=weighted)
        return path
    if the_command == 'compute_energies':
        energies = instance.compute_sequence_energies(query_file)
        path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_energies_', postfix='.txt')
        dca_utilities.write_sequence_energies(path, energies, metadata=metadata, query_file=query_file or msa_file)
        return path
    if not wildtype_file:
        raise exc_type('compute_mutation_effects needs --wildtype_file')
    L = int(instance.sequences_len)
    w = wildtype_codes(wildtype_file, biomolecule, L, table, exc_type)
    dE = instance.compute_single_mutant_effects(wildtype_file)
    letters = state_letters(biomolecule)
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_mutation_effects_', postfix='.txt')
    dca_utilities.write_mutation_effects(path, dE, [letters[c] for c in w], letters, metadata=metadata, wildtype_file=wildtype_file)
    return path


def add_boltzmann_arguments(p):
    """The options of the plmdca fit_boltzmann sub-command (PlmDCA.fit_boltzmann; --lambda_h / --lambda_J stay the
    pseudo-likelihood fit's penalties, the L2 weights of the refinement are --bm_lambda_h / --bm_lambda_J)."""
    p.add_argument('--iterations', type=int, default=500, help='Boltzmann-learning iterations (addition)')
    p.add_argument('--num_chains', type=int, default=1000, help='persistent Gibbs chains (addition)')
    p.add_argument('--sweeps_per_iteration', type=int, default=10, help='Gibbs sweeps of every chain per iteration (addition)')
    p.add_argument('--equilibration_sweeps', type=int, default=100, help='sweeps before the first iteration (addition)')
    p.add_argument('--learning_rate', type=float, default=0.05, help='gradient step of fields and couplings (addition)')
    p.add_argument('--bm_lambda_h', type=float, default=1e-4, help='L2 weight of the fields in the refinement (addition)')
    p.add_argument('--bm_lambda_J', type=float, default=1e-4, help='L2 weight of the couplings in the refinement (addition)')
    p.add_argument('--pseudocount', type=float, help='pseudocount of the data frequencies (default: 1 / Meff) (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the chains\' counter-based generator (addition)')
    p.add_argument('--init', choices=('plm', 'zero'), default='plm', help='start from the pseudo-likelihood fit or from zero (addition)')
    p.add_argument('--num_samples', type=int, help='also draw this many sequences from the refined model (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps of each of those samples (addition)')


BOLTZMANN_OPTIONS = ('iterations', 'num_chains', 'sweeps_per_iteration', 'equilibration_sweeps', 'learning_rate', 'bm_lambda_h',
                     'bm_lambda_J', 'pseudocount', 'seed', 'init', 'num_samples', 'num_sweeps')


def add_decimation_arguments(p):
    """The options of the plmdca decimate_boltzmann sub-command (PlmDCA.decimate_boltzmann; the L2 weights of the learning are
    --bm_lambda_h / --bm_lambda_J, as under fit_boltzmann)."""
    p.add_argument('--target_density', type=float, default=0.02, help='fraction of the coupling elements to keep (addition)')
    p.add_argument('--drop_fraction', type=float, default=0.01, help='fraction of the active elements removed per round (addition)')
    p.add_argument('--pearson_target', type=float, default=0.95, help='learn until the connected correlations correlate this well (addition)')
    p.add_argument('--iterations_per_check', type=int, default=10, help='iterations between two looks at the correlation (addition)')
    p.add_argument('--max_iterations_per_round', type=int, default=500, help='iterations after a decimation at most (addition)')
    p.add_argument('--warmup_iterations', type=int, default=500, help='iterations before the first decimation at most (addition)')
    p.add_argument('--gauge', choices=('zero_sum', 'keep'), default='zero_sum', help='move the model to the zero-sum gauge first (addition)')
    p.add_argument('--num_chains', type=int, default=1000, help='persistent Gibbs chains (addition)')
    p.add_argument('--sweeps_per_iteration', type=int, default=10, help='Gibbs sweeps of every chain per iteration (addition)')
    p.add_argument('--equilibration_sweeps', type=int, default=100, help='sweeps before the first iteration (addition)')
    p.add_argument('--learning_rate', type=float, default=0.05, help='gradient step of fields and couplings (addition)')
    p.add_argument('--bm_lambda_h', type=float, default=1e-4, help='L2 weight of the fields in the learning (addition)')
    p.add_argument('--bm_lambda_J', type=float, default=1e-4, help='L2 weight of the couplings in the learning (addition)')
    p.add_argument('--pseudocount', type=float, help='pseudocount of the data frequencies (default: 1 / Meff) (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the chains\' counter-based generator (addition)')
    p.add_argument('--init', choices=('plm', 'zero'), default='plm', help='start from the pseudo-likelihood fit or from zero (addition)')
    p.add_argument('--num_samples', type=int, help='also draw this many sequences from the sparse model (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps of each of those samples (addition)')


DECIMATION_OPTIONS = ('target_density', 'drop_fraction', 'pearson_target', 'iterations_per_check', 'max_iterations_per_round',
                      'warmup_iterations', 'gauge', 'num_chains', 'sweeps_per_iteration', 'equilibration_sweeps', 'learning_rate',
                      'bm_lambda_h', 'bm_lambda_J', 'pseudocount', 'seed', 'init', 'num_samples', 'num_sweeps')


def run_decimation(instance, prefix, msa_file, output_dir, metadata, biomolecule, opts):
    """plmdca decimate_boltzmann -> the paths written: <output_dir>/<prefix>_decimation_<alignment base>.txt (the rounds),
    <prefix>_decimation_params_<alignment base>.npy (the sparse x), <prefix>_decimation_mask_<alignment base>.npy (bool[pairs, q,
    q]) and, with num_samples, <prefix>_decimation_samples_<alignment base>.fa (the sample_sequences format)."""
    from .dca_utilities import dca_utilities
    import numpy as np
    opts = dict(opts or {})
    dca_utilities.create_directories(output_dir)
    kw = dict(pseudocount=opts.get('pseudocount'))
    for key in DECIMATION_OPTIONS:
        name = {'bm_lambda_h': 'lambda_h', 'bm_lambda_J': 'lambda_J'}.get(key, key)
        if key not in ('pseudocount', 'num_samples', 'num_sweeps') and opts.get(key) is not None:
            kw[name] = opts[key]
    fit = instance.decimate_boltzmann(**kw)

    def path(middle, postfix):
        return dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_decimation_' + middle, postfix=postfix)
    table, params, mask = path('', '.txt'), path('params_', '.npy'), path('mask_', '.npy')
    dca_utilities.write_decimation_rounds(table, fit['rounds'], fit['density'], metadata=metadata)
    np.save(params, fit['fields_and_couplings'])
    np.save(mask, fit['mask'])
    paths = [table, params, mask]
    if opts.get('num_samples'):
        codes = instance.sample_sequences(int(opts['num_samples']), num_sweeps=opts.get('num_sweeps') or 1000,
                                          seed=opts.get('seed') or 0, return_codes=True)
        letters = state_letters(biomolecule)
        seqs = [''.join(letters[c] for c in row) for row in codes]
        samples = path('samples_', '.fa')
        dca_utilities.write_sampled_sequences(samples, seqs, instance.compute_sequence_energies(seqs))
        paths.append(samples)
    return tuple(paths)


def run_boltzmann(instance, prefix, msa_file, output_dir, metadata, biomolecule, opts):
    """plmdca fit_boltzmann -> the paths written: <output_dir>/<prefix>_boltzmann_<alignment base>.txt (learning curve),
    <prefix>_boltzmann_params_<alignment base>.npy (the refined x) and, with num_samples, <prefix>_boltzmann_samples_
    <alignment base>.fa (the sample_sequences format)."""
    from .dca_utilities import dca_utilities
    import numpy as np
    opts = dict(opts or {})
    dca_utilities.create_directories(output_dir)
    kw = dict(pseudocount=opts.get('pseudocount'), init=opts.get('init') or 'plm')
    for key, name in (('iterations', 'iterations'), ('num_chains', 'num_chains'), ('sweeps_per_iteration', 'sweeps_per_iteration'),
                      ('equilibration_sweeps', 'equilibration_sweeps'), ('learning_rate', 'learning_rate'),
                      ('bm_lambda_h', 'lambda_h'), ('bm_lambda_J', 'lambda_J'), ('seed', 'seed')):
        if opts.get(key) is not None:
            kw[name] = opts[key]
    fit = instance.fit_boltzmann(**kw)
    curve = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_boltzmann_', postfix='.txt')
    dca_utilities.write_boltzmann_history(curve, fit['history'], metadata=metadata)
    params = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_boltzmann_params_', postfix='.npy')
    np.save(params, fit['fields_and_couplings'])
    paths = [curve, params]
    if opts.get('num_samples'):
        codes = instance.sample_sequences(int(opts['num_samples']), num_sweeps=opts.get('num_sweeps') or 1000,
                                          seed=opts.get('seed') or 0, return_codes=True)
        letters = state_letters(biomolecule)
        seqs = [''.join(letters[c] for c in row) for row in codes]
        samples = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix=prefix + '_boltzmann_samples_', postfix='.fa')
        dca_utilities.write_sampled_sequences(samples, seqs, instance.compute_sequence_energies(seqs))
        paths.append(samples)
    return tuple(paths)
