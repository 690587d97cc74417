"""File output of the command lines.  The TEXT these functions write is the contract with the reference
(pydca/dca_utilities/dca_utilities.py: metadata lines :109-201, score files :236-266, couplings / fields CSV :293-359,
frequency files :362-436, trimmed alignments :581-607) and is reproduced character for character -- rule lines of
'#' + 70 '=', the metadata wording, 1-based sites, '{0:<7} {1:<14} {2:<35}' score rows, comma-separated rows without
padding.  How the text is produced is this module's own: every writer builds its header and hands an iterator of
rows to one routine that streams them out."""
import errno
import logging
import os

import numpy as np

from ..fasta_reader import fasta_reader

logger = logging.getLogger(__name__)

_RULE = '#' + '=' * 70


def create_directories(the_path):
    """mkdir -p; an existing directory is fine (dca_utilities.py:9-27)."""
    try:
        os.makedirs(the_path)
    except OSError as exc:
        if exc.errno != errno.EEXIST:
            logger.error('cannot create the output directory {}'.format(the_path))
            raise


def get_dca_output_file_path(output_dir, msa_file_name, prefix='', postfix=''):
    """<output_dir>/<prefix><alignment file name without extension><postfix> (dca_utilities.py:29-57)."""
    stem = os.path.splitext(os.path.basename(msa_file_name))[0]
    return os.path.join(output_dir, ''.join(part.strip() for part in (prefix, stem, postfix)))


def _stream(file_name, header, rows, what):
    """Writes the header lines and then the rows (already formatted, without line ends) to file_name."""
    logger.info('\n\twriting {} to {}'.format(what, file_name))
    with open(file_name, 'w') as fh:
        fh.writelines(line + '\n' for line in header)
        fh.writelines(row + '\n' for row in rows)


def _described(label_width_prefix, instance, fields):
    return ['# PARAMETERS USED FOR THIS COMPUTATION: '] + [
        '#{}{}: {}'.format(label_width_prefix, label, getattr(instance, attr)) for label, attr in fields]


def mfdca_param_metadata(mfdca_instance):
    return _described('      ', mfdca_instance, (
        ('Sequence type', 'biomolecule'),
        ('Total number of sequences in alignment data', 'num_sequences'),
        ('Length of sequences in alignment data', 'sequences_len'),
        ('Effective number of sequences', 'effective_num_sequences'),
        ('Value of sequence identity', 'sequence_identity'),
        ('Value of relative pseudocount', 'pseudocount')))


def plmdca_param_metadata(plmdca_instance):
    return _described('\t', plmdca_instance, (
        ('Sequence type', 'biomolecule'),
        ('Total number of sequences in alignment data', 'num_sequences'),
        ('Length of sequences in alignment data', 'sequences_len'),
        ('Value of sequence identity', 'sequence_identity'),
        ('lambda_h', 'lambda_h'),
        ('lambda_J', 'lambda_J'),
        ('Number of gradient decent iterations', 'max_iterations')))      # sic: the reference's wording, part of the file format


def mfdca_residue_repr_metadata(biomolecule):
    """'# RESIDUES IDENTIFICATION' and the integer -> letter table as Python tuples, five per line, plus the line the
    reference's range(len // 5 + 1) adds at the end (empty but for '# ' when the table divides by five)."""
    table = sorted(fasta_reader.res_to_char(biomolecule).items())
    lines = ['# RESIDUES IDENTIFICATION']
    for first in range(0, 5 * (len(table) // 5 + 1), 5):
        lines.append('# ' + ''.join(map(str, table[first:first + 5])))
    return lines


def write_sorted_dca_scores(file_name, sorted_DI, metadata=None, score_type=None):
    header = [_RULE] + list(metadata or []) + [
        '# The First and Second columns represent sites and the',
        '# Third column is {} DCA score'.format(score_type), _RULE]
    rows = ('{0:<7} {1:<14} {2:<35}'.format(pair[0] + 1, pair[1] + 1, score) for pair, score in sorted_DI)
    _stream(file_name, header, rows, 'ranked scores')


def write_sequence_energies(file_name, energies, metadata=None, query_file=None):
    """One row per query record: its number (1-based, input order) and its statistical energy (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    if query_file:
        header.append('#\tQuery sequences: {}'.format(query_file))
    header += ['# The First column is the record number (1-based) of the query sequence and the',
               '# Second its statistical energy E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j) (higher is more probable)', _RULE]
    rows = ('{0:<7} {1}'.format(k + 1, float(e)) for k, e in enumerate(energies))
    _stream(file_name, header, rows, 'sequence energies')


def write_pseudo_log_likelihoods(file_name, plls, metadata=None, query_file=None, weighted=None):
    """One row per query record: its number (1-based, input order) and its pseudo-log-likelihood PLL(s) = sum_i log P(s_i | s_-i);
    weighted (the training records' sum_n w_n PLL(s_n) / Meff) adds a header line (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    if query_file:
        header.append('#\tQuery sequences: {}'.format(query_file))
    if weighted is not None:
        header.append('#\tWeighted pseudo-log-likelihood per effective sequence: {}'.format('%.17g' % float(weighted)))
    header += ['# The First column is the record number (1-based) of the query sequence and the',
               '# Second its pseudo-log-likelihood PLL(s) = sum_i log P(s_i | s_-i) under the model', _RULE]
    rows = ('{0:<7} {1}'.format(k + 1, '%.17g' % float(v)) for k, v in enumerate(plls))
    _stream(file_name, header, rows, 'pseudo-log-likelihoods')


def write_sequence_comparison(file_name, summary, dist, index, hist, self_hist, seqs_len, metadata=None, query_file=None):
    """Header: the summary of compare_with_alignment (one '#\t<name>: <value>' line per scalar, %.17g) and the non-zero bins of the
    two distance histograms ('#\tdistance <d>: <query-alignment pairs> <alignment-alignment pairs>'); then one row per query record:
    its number (1-based, input order), the Hamming distance to the nearest alignment sequence, that sequence's row index
    (0-based, smallest on ties) and the identity 1 - d / L (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    if query_file:
        header.append('#\tQuery sequences: {}'.format(query_file))
    for key in sorted(summary):
        v = summary[key]
        if np.ndim(v) == 0:
            header.append('#\t{}: {}'.format(key, int(v) if isinstance(v, (int, np.integer)) else '%.17g' % float(v)))
    header.append('# Pairs at every Hamming distance with at least one: query against alignment, alignment against itself (other rows)')
    for d in range(len(hist)):
        if int(hist[d]) or int(self_hist[d]):
            header.append('#\tdistance {}: {} {}'.format(d, int(hist[d]), int(self_hist[d])))
    header += ['# The First column is the record number (1-based) of the query sequence, the Second its Hamming distance',
               '# to the nearest alignment sequence, the Third that sequence\'s row (0-based) and the Fourth the identity 1 - d / L', _RULE]
    L = float(seqs_len)
    rows = ('{0:<7} {1:<5} {2:<7} {3}'.format(k + 1, int(d), int(m), '%.17g' % (1.0 - int(d) / L)) for k, (d, m) in enumerate(zip(dist, index)))
    _stream(file_name, header, rows, 'sequence comparison')


def write_mutation_effects(file_name, dE, wildtype_letters, state_letters, metadata=None, wildtype_file=None):
    """One row per (site, state), site-major: site (1-based), wild-type letter, mutant letter and
    dE = E(mutant) - E(wild type) (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    if wildtype_file:
        header.append('#\tWild-type sequence: {}'.format(wildtype_file))
    header += ['# The First column is the site (1-based), the Second the wild-type residue, the Third the',
               '# mutant residue and the Fourth dE = E(mutant) - E(wild type) (positive: the mutant is more probable)', _RULE]
    L, q = dE.shape
    rows = ('{0:<7} {1} {2} {3}'.format(i + 1, wildtype_letters[i], state_letters[a], float(dE[i, a])) for i in range(L) for a in range(q))
    _stream(file_name, header, rows, 'single-mutant effects')


def write_sampled_sequences(file_name, sequences, energies, header=None):
    """FASTA of sampled sequences: one record '>sample_<k> energy=<E>' per sequence (k from 1, E written with %.17g so
    that it reads back to the same double), the aligned sequence on one line; header: '#' lines written first
    (sample_conditional names its free sites there).  No reference counterpart."""
    rows = ('>sample_{} energy={}\n{}'.format(k + 1, '%.17g' % float(e), seq) for k, (seq, e) in enumerate(zip(sequences, energies)))
    _stream(file_name, list(header or []), rows, 'sampled sequences')


def write_tempered_samples(file_name, temperatures, sequences, energies):
    """FASTA of sample_sequences_tempered: per temperature (the caller's order), then per sample, one record
    '>sample_<k> temperature=<T> energy=<E>' (k from 1 within its temperature; T and E written with %.17g), the aligned
    sequence on one line.  No reference counterpart."""
    rows = ('>sample_{} temperature={} energy={}\n{}'.format(k + 1, '%.17g' % float(t), '%.17g' % float(e), seq)
            for t, seqs, es in zip(temperatures, sequences, energies) for k, (seq, e) in enumerate(zip(seqs, es)))
    _stream(file_name, [], rows, 'tempered samples')


def write_tempered_summary(file_name, result, colder_acceptance, metadata=None):
    """One row per temperature of sample_sequences_tempered (the caller's order): T, the mean energy and the heat capacity over
    the exchange rounds past burn-in, and the acceptance of exchanges with the next colder temperature of the ladder (nan for
    the coldest and where nothing was attempted), each written with %.17g (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    header += ['#\tExchange rounds: {}'.format(int(result['num_rounds'])),
               '# Columns: temperature T, mean energy <E>, heat capacity C = Var(E) / T^2 (both over all ladders and the exchange',
               '# rounds past burn-in) and the accepted fraction of exchanges with the next colder temperature', _RULE]
    rows = ('{} {} {} {}'.format(*('%.17g' % float(v) for v in rec))
            for rec in zip(result['temperatures'], result['mean_energy'], result['heat_capacity'], colder_acceptance))
    _stream(file_name, header, rows, 'tempered sampling summary')


def write_local_maxima_sequences(file_name, sequences, energies):
    """FASTA of the final sequences of find_local_maxima: one record '>maximum_of_<k> energy=<E>' per input record k (from 1,
    input order; E written with %.17g), the aligned sequence on one line.  No reference counterpart."""
    rows = ('>maximum_of_{} energy={}\n{}'.format(k + 1, '%.17g' % float(e), seq) for k, (seq, e) in enumerate(zip(sequences, energies)))
    _stream(file_name, [], rows, 'local maxima')


def write_local_maxima(file_name, result, metadata=None, query_file=None):
    """One row per input record of find_local_maxima: its number (1-based, input order), start energy, final energy, steps,
    converged (1 / 0) and basin (1-based index of its maximum by descending energy, 0 when unconverged); energies written with
    %.17g.  The header counts the distinct maxima (no reference counterpart)."""
    header = [_RULE] + list(metadata or [])
    if query_file:
        header.append('#\tStarting sequences: {}'.format(query_file))
    header += ['#\tDistinct local maxima among the converged sequences: {}'.format(len(result['basin_sizes'])),
               '# Columns: record number (1-based), start energy, final energy, steps, converged (1 / 0) and basin: the 1-based',
               '# rank of its local maximum by descending energy (0: not converged within max_steps)', _RULE]
    rows = ('{0:<7} {1} {2} {3} {4} {5}'.format(k + 1, '%.17g' % float(result['start_energies'][k]), '%.17g' % float(result['energies'][k]),
                                                int(result['num_steps'][k]), int(bool(result['converged'][k])), int(result['basin'][k]) + 1)
            for k in range(len(result['energies'])))
    _stream(file_name, header, rows, 'local maxima')


def write_boltzmann_history(file_name, history, metadata=None):
    """Learning curve of PlmDCA.fit_boltzmann: one row per iteration t (0-based) with eps_h, eps_J and pearson, each
    written with %.17g (no reference counterpart)."""
    header = [_RULE] + list(metadata or []) + [
        '# Columns: iteration t (0-based), eps_h = max |f_i - g_i|, eps_J = max |f_ij - g_ij| and the Pearson correlation',
        '# of the connected correlations of the data (f) and of the model chains (g), measured before the update of t', _RULE]
    rows = ('{} {} {} {}'.format(t, *('%.17g' % float(v) for v in rec)) for t, rec in enumerate(history))
    _stream(file_name, header, rows, 'Boltzmann learning curve')


def write_decimation_rounds(file_name, rounds, density, metadata=None):
    """Rounds of PlmDCA.decimate_boltzmann: one row per decimation with the iteration index it came after, the active coupling
    elements before it, the number removed, the density after it, the largest removed score and the Pearson correlation before
    it; the reals written with %.17g (no reference counterpart)."""
    header = [_RULE] + list(metadata or []) + [
        '#\tFinal density of the couplings: {}'.format('%.17g' % float(density)),
        '# Columns: iterations run before the decimation, active coupling elements before it, elements removed, density after it,',
        '# threshold = the largest removed symmetrised Kullback-Leibler score, Pearson correlation of the connected correlations',
        '# of the data and of the model chains before it', _RULE]
    rows = ('{} {} {} {} {} {}'.format(int(r[0]), int(r[1]), int(r[2]), *('%.17g' % float(v) for v in r[3:])) for r in rounds)
    _stream(file_name, header, rows, 'decimation rounds')


def write_log_likelihood(file_name, result, log_likelihood, log_probabilities, options, metadata=None):
    """log Z by annealed importance sampling and the log-likelihood of the training alignment (compute_log_likelihood
    sub-command): a header with log Z, its stderr, the ESS, log Z0 and the schedule, the line 'average_log_likelihood <value>',
    then one log P(s) = E(s) - log Z per training record in file order, every value written with %.17g (no reference
    counterpart)."""
    g = lambda v: '%.17g' % float(v)
    header = [_RULE] + list(metadata or []) + [
        '#\tlog Z (annealed importance sampling): {}'.format(g(result['log_z'])),
        '#\tstderr of log Z: {}'.format(g(result['log_z_stderr'])),
        '#\teffective sample size: {}'.format(g(result['ess'])),
        '#\tlog Z of the base model: {}'.format(g(result['log_z_base'])),
        '#\tschedule: {} chains, K = {} temperatures beta_k = k / K, {} sweeps per temperature, seed {}, base {}'.format(
            options['num_chains'], options['num_temperatures'], options['sweeps_per_temperature'], options['seed'],
            options['base'] if isinstance(options['base'], str) else 'array'),
        '# Below: the average log-likelihood (sum_n w_n E(s_n)) / Meff - log Z of the training alignment, then one',
        '# log-probability E(s) - log Z per training record (file order)', _RULE]
    rows = ['average_log_likelihood {}'.format(g(log_likelihood))] + [g(v) for v in log_probabilities]
    _stream(file_name, header, rows, 'log-likelihood')


def _csv(prefix_values, values):
    # '{}'.format(v), not str(v): numpy scalars of the two print differently (a float32 is widened by format)
    return ','.join('{}'.format(v) for v in list(prefix_values) + list(values))


def write_couplings_csv(file_name, couplings, metadata=None):
    """One row per site pair: i, j (1-based) and the (q-1)^2 couplings of the pair."""
    header = [_RULE] + (list(metadata) + [_RULE] if metadata else [])
    rows = (_csv((pair[0] + 1, pair[1] + 1), block) for pair, block in couplings)
    _stream(file_name, header, rows, 'couplings')


def write_fields_csv(file_name, fields, metadata=None):
    """One row per site: i (1-based) and its q-1 fields.  Without metadata only the rule line is written: in the
    reference the rows are produced inside the metadata branch (dca_utilities.py:346-357) and every caller passes it."""
    header = [_RULE]
    rows = ()
    if metadata is not None:
        header += list(metadata) + [_RULE]
        rows = (_csv((site + 1,), site_fields) for site, site_fields in fields)
    _stream(file_name, header, rows, 'fields')


def write_single_site_freqs(file_name, fi, seqs_len=None, num_site_states=None, metadata=None):
    header = [_RULE]
    if metadata:
        header += list(metadata) + [
            '# Below, the First integer refers to the site, the ',
            '# Second the residue at that site, and the Third is the ',
            '# frequency. Residue numbers are mapped as shown above.', _RULE]
    rows = ('{},{},{}'.format(i + 1, a + 1, fi[i, a]) for i in range(seqs_len) for a in range(num_site_states))
    _stream(file_name, header, rows, 'single-site frequencies')


def write_pair_site_freqs(file_name, fij, seqs_len=None, num_site_states=None, metadata=None):
    """Pair frequencies without the gap state; fij is indexed [pair in (0,1),(0,2),... order, a, b]."""
    header = [_RULE]
    if metadata:
        header += list(metadata) + [
            '# Below, the First and Second integers refer to sites, the ',
            '# Third and Fourth residues, and the Last one is frequency for pairs.',
            '# Residue numbers are mapped as shown above.', _RULE]
    states = range(num_site_states - 1)
    pairs = ((i, j) for i in range(seqs_len - 1) for j in range(i + 1, seqs_len))
    rows = ('{},{},{},{},{}'.format(i + 1, j + 1, a + 1, b + 1, fij[p, a, b])
            for p, (i, j) in enumerate(pairs) for a in states for b in states)
    _stream(file_name, header, rows, 'pair-site frequencies (gap state left out)')


def write_trimmed_msa(file_name, msa_trimmer=None, columns_to_remove=None, metadata=None):
    """FASTA with one line per sequence; the listed columns are left out of every record."""
    dropped = frozenset(columns_to_remove)
    rows = ('>{}\n{}'.format(record.id, ''.join(ch for col, ch in enumerate(record.seq) if col not in dropped))
            for record in msa_trimmer.alignment_data)
    _stream(file_name, [], rows, 'the trimmed alignment')
