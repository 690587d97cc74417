"""`hopfield` command line: the Hopfield-Potts model (pydca_amd/hopfield_dca).  compute_fn ranks the site pairs by the Frobenius
norm of the low-rank couplings, compute_patterns writes the selected patterns, project_sequences the overlaps of a query set with
them; the sequence-model sub-commands are those of `mfdca`, on the Hopfield-Potts couplings."""
import logging
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _compare, _lib, _potts
from .dca_utilities import dca_utilities
from .hopfield_dca import hopfield_dca
from .sequence_backmapper.sequence_backmapper import SequenceBackmapper

logger = logging.getLogger(__name__)
SUBCOMMANDS = ('compute_fn', 'compute_patterns', 'project_sequences')
_RULE = '#' + '-' * 100


def configure_logging():
    logging.basicConfig(level=logging.INFO, format='%(levelname)s %(name)s: %(message)s')


def selection_metadata(fit):
    return ['#\tAttractive patterns (eigenvalue > 1): {}'.format(fit['num_attractive']),
            '#\tRepulsive patterns (eigenvalue < 1): {}'.format(fit['num_repulsive']),
            '#\tSubspace iterations (attractive end, repulsive end): {}, {}'.format(*fit['iterations']),
            '#\tConverged (attractive end, repulsive end): {}, {}'.format(*fit['converged'])]


def write_patterns(instance, msa_file, output_dir, metadata):
    """-> (text path, npy path): one row per pattern (number, eigenvalue, likelihood gain, sign, residual) and the patterns
    float64[p, L, q - 1] in the same order."""
    fit = instance.compute_patterns()
    text = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='HOPFIELD_patterns_', postfix='.txt')
    npy = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='HOPFIELD_patterns_', postfix='.npy')
    with open(text, 'w') as fh:
        for line in [_RULE] + list(metadata) + selection_metadata(fit) + [
                '# Columns: pattern number (1-based), eigenvalue, likelihood gain (eigenvalue - 1 - ln eigenvalue) / 2, sign of',
                '# 1 - 1 / eigenvalue (+1 attractive, -1 repulsive), residual ||Gamma v - eigenvalue v||', _RULE]:
            fh.write(line + '\n')
        for m in range(len(fit['eigenvalues'])):
            fh.write('{0:<7} {1!r:<26} {2!r:<26} {3:<3} {4!r}\n'.format(m + 1, float(fit['eigenvalues'][m]), float(fit['gains'][m]),
                                                                       int(fit['signs'][m]), float(fit['residuals'][m])))
    np.save(npy, fit['patterns'])
    return text, npy


def write_overlaps(instance, msa_file, output_dir, metadata, query_file):
    """-> the path: one row per query record, its number (1-based) and its overlap with every pattern."""
    x = instance.project_on_patterns(query_file)
    path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='HOPFIELD_overlaps_', postfix='.txt')
    with open(path, 'w') as fh:
        for line in [_RULE] + list(metadata) + ['#\tQuery sequences: {}'.format(query_file),
                                                '# The First column is the record number (1-based) of the query sequence, the others',
                                                '# its overlaps with the patterns in the order of compute_patterns', _RULE]:
            fh.write(line + '\n')
        for k, row in enumerate(x):
            fh.write('{0:<7} {1}\n'.format(k + 1, ' '.join(repr(float(v)) for v in row)))
    return path


def execute_from_command_line(msa_file=None, biomolecule=None, seqid=None, pseudocount=None, the_command=None, refseq_file=None,
                              verbose=False, output_dir=None, apc=False, device=0, num_patterns=None, num_attractive=None,
                              num_repulsive=None, tolerance=None, max_iterations=None, fit_seed=None, query_file=None, wildtype_file=None,
                              sampling=None, ais=None, three_site=0, three_site_no_gaps=False, pca=None, conditional=None, ascent=None,
                              tempered=None, interaction=None):
    if verbose:
        configure_logging()
    if num_patterns is None and num_attractive is None and num_repulsive is None:
        raise hopfield_dca.HopfieldPottsDCAException('give --num_patterns or --num_attractive / --num_repulsive')
    instance = hopfield_dca.HopfieldPottsDCA(
        msa_file, biomolecule, pseudocount=pseudocount, seqid=seqid, num_patterns=num_patterns, num_attractive=num_attractive,
        num_repulsive=num_repulsive, tolerance=1e-10 if tolerance is None else tolerance,
        max_iterations=1000 if max_iterations is None else max_iterations, seed=0 if fit_seed is None else fit_seed, device=device)
    the_command = the_command.strip()
    metadata = dca_utilities.mfdca_param_metadata(instance)
    if not output_dir:
        output_dir = 'HOPFIELD_output_' + os.path.splitext(os.path.basename(msa_file))[0]
    dca_utilities.create_directories(output_dir)
    if the_command in _potts.POTTS_SUBCOMMANDS:
        bio = _lib.DCA_BIOMOLECULE_PROTEIN if instance.num_site_states == 21 else _lib.DCA_BIOMOLECULE_RNA
        return _potts.run_subcommand(instance, the_command, 'HOPFIELD', msa_file, output_dir, metadata, bio, 1,
                                     hopfield_dca.HopfieldPottsDCAException, query_file=query_file, wildtype_file=wildtype_file,
                                     sampling=sampling, ais=ais, three_site=three_site, three_site_no_gaps=bool(three_site_no_gaps), pca=pca,
                                     conditional=conditional, ascent=ascent, tempered=tempered, interaction=interaction)
    if the_command == 'compute_patterns':
        return write_patterns(instance, msa_file, output_dir, metadata)
    if the_command == 'project_sequences':
        if not query_file:
            raise hopfield_dca.HopfieldPottsDCAException('project_sequences needs --query_file')
        return write_overlaps(instance, msa_file, output_dir, metadata, query_file)
    seqbackmapper = None
    if refseq_file:
        seqbackmapper = SequenceBackmapper(alignment_data=instance.alignment, refseq_file=refseq_file, biomolecule=instance.biomolecule)
    if apc:
        score_type = 'Hopfield-Potts Frobenius norm, average product corrected (APC)'
        ranked = instance.compute_sorted_FN_APC(seqbackmapper=seqbackmapper)
        path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='HOPFIELD_apc_fn_scores_', postfix='.txt')
    else:
        score_type = 'Hopfield-Potts raw Frobenius norm'
        ranked = instance.compute_sorted_FN(seqbackmapper=seqbackmapper)
        path = dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='HOPFIELD_raw_fn_scores_', postfix='.txt')
    dca_utilities.write_sorted_dca_scores(path, ranked, metadata=metadata + selection_metadata(instance.compute_patterns()),
                                          score_type=score_type)
    return path


def run_hopfield_dca(argv=None):
    parser = ArgumentParser(prog='hopfield')
    subparsers = parser.add_subparsers(dest='subcommand_name')
    for name in SUBCOMMANDS + _potts.POTTS_SUBCOMMANDS:
        p = subparsers.add_parser(name)
        p.add_argument('biomolecule')
        p.add_argument('msa_file')
        p.add_argument('--seqid', type=float)
        p.add_argument('--pseudocount', type=float)
        p.add_argument('--output_dir')
        p.add_argument('--verbose', action='store_true')
        p.add_argument('--num_patterns', type=int, help='the patterns of largest likelihood gain over the whole spectrum')
        p.add_argument('--num_attractive', type=int, help='that many of the largest eigenvalues (at most 64)')
        p.add_argument('--num_repulsive', type=int, help='that many of the smallest eigenvalues (at most 64)')
        p.add_argument('--tolerance', type=float, help='residual of a pattern relative to the largest Ritz value (1e-10)')
        p.add_argument('--max_iterations', type=int, help='subspace iterations per end (1000)')
        p.add_argument('--fit_seed', type=int, help='seed of the start block of the subspace iterations (0)')
        p.add_argument('--device', type=int, default=0, help='GPU index')
        if name == 'compute_fn':
            p.add_argument('--apc', action='store_true')
            p.add_argument('--refseq_file')
        if name == 'project_sequences':
            p.add_argument('--query_file', required=True, help='FASTA file of aligned query sequences')
        if name in ('compute_energies', 'compute_pseudo_log_likelihood'):
            p.add_argument('--query_file', help='FASTA file of aligned query sequences (default: the records of msa_file)')
        if name == 'compare_sequences':
            p.add_argument('--query_file', required=True)
            p.add_argument('--three_site', type=int, default=0)
            p.add_argument('--three_site_no_gaps', action='store_true')
            p.add_argument('--pca', type=int, default=0)
        if name == 'compute_pca':
            _compare.add_pca_arguments(p)
        if name == 'compute_mutation_effects':
            p.add_argument('--wildtype_file', required=True, help='FASTA file with one aligned wild-type sequence')
        if name == 'sample_sequences':
            _potts.add_sampling_arguments(p)
        if name == 'sample_conditional':
            _potts.add_conditional_arguments(p)
        if name == 'find_local_maxima':
            _potts.add_ascent_arguments(p)
        if name == 'compute_interaction_energies':
            _potts.add_interaction_arguments(p)
        if name == 'sample_tempered':
            _potts.add_tempered_arguments(p)
        if name == 'compute_log_likelihood':
            _potts.add_ais_arguments(p)
    argv = sys.argv[1:] if argv is None else argv
    args = vars(parser.parse_args(args=argv if argv else ['--help']))
    return execute_from_command_line(
        biomolecule=args.get('biomolecule'), msa_file=args.get('msa_file'), seqid=args.get('seqid'), pseudocount=args.get('pseudocount'),
        the_command=args.get('subcommand_name'), refseq_file=args.get('refseq_file'), verbose=args.get('verbose'),
        output_dir=args.get('output_dir'), apc=args.get('apc'), device=args.get('device'), num_patterns=args.get('num_patterns'),
        num_attractive=args.get('num_attractive'), num_repulsive=args.get('num_repulsive'), tolerance=args.get('tolerance'),
        max_iterations=args.get('max_iterations'), fit_seed=args.get('fit_seed'), query_file=args.get('query_file'),
        wildtype_file=args.get('wildtype_file'),
        sampling={k: args.get(k) for k in ('num_sequences', 'num_sweeps', 'seed', 'temperature', 'initial_file')},
        ais={k: args.get(k) for k in _potts.AIS_OPTIONS},
        three_site=args.get('three_site') or 0, three_site_no_gaps=bool(args.get('three_site_no_gaps')),
        pca={k: args.get(k) for k in ('pca', 'num_components', 'seed')},
        conditional={k: args.get(k) for k in _potts.CONDITIONAL_OPTIONS},
        ascent={k: args.get(k) for k in _potts.ASCENT_OPTIONS},
        tempered={k: args.get(k) for k in _potts.TEMPERED_OPTIONS},
        interaction={k: args.get(k) for k in _potts.INTERACTION_OPTIONS})


if __name__ == '__main__':
    run_hopfield_dca()
