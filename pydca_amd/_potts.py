"""Query sequences of the energy methods of PlmDCA and MeanFieldDCA, encoded for the context (dca_encode_sequences)."""
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


def sampling_beta(temperature, exc_type):
    """beta = 1 / temperature for a finite temperature > 0."""
    t = float(temperature)
    if not (0.0 < t < float('inf')):
        raise exc_type('the temperature must be finite and > 0, not {}'.format(temperature))
    return 1.0 / t


def state_letters(biomolecule):
    """Letter of every 0-based state (gap last), for the CLI's mutation-effect rows and sampled sequences."""
    return list('ACDEFGHIKLMNPQRSTVWY-') if biomolecule == _lib.DCA_BIOMOLECULE_PROTEIN else list('ACGU-')



POTTS_SUBCOMMANDS = ('compute_energies', 'compute_mutation_effects', 'sample_sequences')


def add_sampling_arguments(p):
    """The options of the sample_sequences sub-command (plmdca and mfdca command lines)."""
    p.add_argument('--num_sequences', type=int, required=True, help='number of sequences (independent chains) to draw (addition)')
    p.add_argument('--num_sweeps', type=int, default=1000, help='Gibbs sweeps over all sites per chain (addition)')
    p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator (addition)')
    p.add_argument('--temperature', type=float, default=1.0, help='sampling temperature T, P(s) ~ exp(E(s) / T) (addition)')
    p.add_argument('--initial_file', help='FASTA file with 1 or num_sequences aligned starting sequences (default: random) (addition)')


def run_subcommand(instance, the_command, prefix, msa_file, output_dir, metadata, biomolecule, table, exc_type,
                   query_file=None, wildtype_file=None, sampling=None):
    """compute_energies / compute_mutation_effects / sample_sequences of the plmdca and mfdca command lines -> the path of
    the file written: <output_dir>/<prefix>_energies_<alignment base>.txt, <prefix>_mutation_effects_<alignment base>.txt
    or <prefix>_samples_<alignment base>.fa.  sampling: the sample_sequences options (num_sequences, num_sweeps, seed,
    temperature, initial_file)."""
    from .dca_utilities import dca_utilities
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
