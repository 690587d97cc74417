"""`ardca` command line: fit, compute_log_probabilities, compute_log_likelihood, sample_sequences, compute_mutation_effects,
compare_sequences, compute_fn and compute_epistasis of the autoregressive model (ArDCA), with the argument names, output directory and file naming of the plmdca / mfdca
sub-commands: <output_dir>/ARDCA_<what>_<alignment base>.txt / .fa / .npy.  No pydca counterpart."""
import logging
import os
import sys
from argparse import ArgumentParser

import numpy as np

from . import _compare, _lib, _potts
from .ardca import ardca
from .dca_utilities import dca_utilities

logger = logging.getLogger(__name__)
ARDCA_SUBCOMMANDS = ('fit', 'compute_log_probabilities', 'compute_log_likelihood', 'sample_sequences', 'compute_mutation_effects',
                    'compare_sequences', 'compute_fn', 'compute_epistasis', 'compute_pca')
_RULE = '#' + '=' * 70


def ardca_param_metadata(instance):
    """'# PARAMETERS USED FOR THIS COMPUTATION: ' and one line per parameter of the ArDCA instance."""
    fields = (('Sequence type', 'biomolecule'), ('Total number of sequences in alignment data', 'num_sequences'),
              ('Length of sequences in alignment data', 'sequences_len'), ('Value of sequence identity', 'sequence_identity'),
              ('lambda_h', 'lambda_h'), ('lambda_J', 'lambda_J'), ('Maximum number of L-BFGS iterations', 'max_iterations'),
              ('epsilon', 'epsilon'), ('Site order', 'order'))
    return ['# PARAMETERS USED FOR THIS COMPUTATION: '] + ['#\t{}: {}'.format(label, getattr(instance, attr)) for label, attr in fields]


def _write(path, header, rows):
    with open(path, 'w') as fh:
        fh.writelines(line + '\n' for line in header)
        fh.writelines(row + '\n' for row in rows)


def write_fit(path, status, site_order, metadata=None):
    """The fit's status lines, then one row per model position j (0-based): j and the file site (1-based) it holds."""
    header = [_RULE] + list(metadata or []) + ['#\t{}: {}'.format(k, v) for k, v in sorted(status.items())] + [
        '# The First column is the model position (0-based) and the Second the file site (1-based) placed there', _RULE]
    _write(path, header, ('{0:<7} {1}'.format(j, int(i) + 1) for j, i in enumerate(site_order)))


def write_log_probabilities(path, logp, metadata=None, query_file=None, weighted=None):
    """One row per query record: its number (1-based, input order) and its exact log P(s) (%.17g); weighted adds the header
    line 'Weighted log-likelihood per effective sequence: <value>'."""
    header = [_RULE] + list(metadata or [])
    if query_file:
        header.append('#\tQuery sequences: {}'.format(query_file))
    if weighted is not None:
        header.append('#\tWeighted log-likelihood per effective sequence: {}'.format('%.17g' % float(weighted)))
    header += ['# The First column is the record number (1-based) of the query sequence and the',
               '# Second its exact log-probability log P(s) under the autoregressive model', _RULE]
    _write(path, header, ('{0:<7} {1}'.format(k + 1, '%.17g' % float(v)) for k, v in enumerate(logp)))


def write_samples(path, sequences, logp):
    """FASTA: one record '>sample_<k> log_probability=<log P>' (k from 1, %.17g) per sequence, the sequence on one line."""
    _write(path, [], ('>sample_{} log_probability={}\n{}'.format(k + 1, '%.17g' % float(v), s) for k, (s, v) in enumerate(zip(sequences, logp))))


def write_mutation_effects(path, dlogp, wildtype_letters, state_letters, metadata=None, wildtype_file=None):
    """One row per (site, state), site-major: site (1-based), wild-type letter, mutant letter, dlogP = log P(mutant) - log P(wt)."""
    header = [_RULE] + list(metadata or [])
    if wildtype_file:
        header.append('#\tWild-type sequence: {}'.format(wildtype_file))
    header += ['# The First column is the site (1-based), the Second the wild-type residue, the Third the',
               '# mutant residue and the Fourth dlogP = log P(mutant) - log P(wild type)', _RULE]
    L, q = dlogp.shape
    _write(path, header, ('{0:<7} {1} {2} {3}'.format(i + 1, wildtype_letters[i], state_letters[a], '%.17g' % float(dlogp[i, a]))
                          for i in range(L) for a in range(q)))


def execute_from_command_line(biomolecule, msa_file, the_command=None, seqid=None, lambda_h=None, lambda_J=None, max_iterations=None,
                              epsilon=None, order=None, output_dir=None, verbose=False, device=0, query_file=None, wildtype_file=None,
                              num_sequences=None, seed=None, apc=False, refseq_file=None, three_site=0,
                              three_site_no_gaps=False, pca=0, num_components=None):
    if verbose:
        logging.basicConfig(level=logging.INFO, format='%(levelname)s %(name)s: %(message)s')
    if the_command not in ARDCA_SUBCOMMANDS:
        raise ardca.ArDCAException('unknown sub-command {!r}'.format(the_command))
    kw = {k: v for k, v in dict(seqid=seqid, lambda_h=lambda_h, lambda_J=lambda_J, max_iterations=max_iterations, epsilon=epsilon,
                                order=order, device=device).items() if v is not None}
    instance = ardca.ArDCA(msa_file, biomolecule, **kw)
    if not output_dir:
        output_dir = 'ARDCA_output_' + os.path.splitext(os.path.basename(msa_file))[0]
    dca_utilities.create_directories(output_dir)
    path = lambda what, postfix: dca_utilities.get_dca_output_file_path(output_dir, msa_file, prefix='ARDCA_' + what + '_', postfix=postfix)
    bio = _lib.DCA_BIOMOLECULE_PROTEIN if instance.biomolecule == 'PROTEIN' else _lib.DCA_BIOMOLECULE_RNA
    letters = _potts.state_letters(bio)
    if the_command == 'fit':
        status = instance.fit()
        x, site_order = instance.get_fields_and_couplings()
        params, fit_file = path('params', '.npy'), path('fit', '.txt')
        np.save(params, x)
        write_fit(fit_file, status, site_order, metadata=ardca_param_metadata(instance))
        return params, fit_file
    meta = ardca_param_metadata(instance)
    if the_command == 'compare_sequences':
        return _compare.run_compare(instance, 'ARDCA', msa_file, output_dir, meta, query_file, ardca.ArDCAException,
                                    three_site=int(three_site or 0), three_site_include_gaps=not three_site_no_gaps, pca=int(pca or 0))
    if the_command == 'compute_pca':
        return _compare.run_pca(instance, 'ARDCA', msa_file, output_dir, meta, query_file=query_file, num_components=num_components,
                                seed=seed)
    if the_command == 'compute_log_probabilities':
        logp = instance.compute_sequence_log_probabilities(query_file)
        out = path('log_probabilities', '.txt')
        write_log_probabilities(out, logp, metadata=meta, query_file=query_file or msa_file)
        return out
    if the_command == 'compute_log_likelihood':
        ll = instance.compute_log_likelihood()
        logp = instance.compute_sequence_log_probabilities()
        out = path('log_likelihood', '.txt')
        write_log_probabilities(out, logp, metadata=meta, query_file=msa_file, weighted=ll)
        return out
    if the_command == 'sample_sequences':
        if num_sequences is None:
            raise ardca.ArDCAException('sample_sequences needs --num_sequences')
        seqs = instance.sample_sequences(num_sequences, seed=seed or 0)
        logp = instance.compute_sequence_log_probabilities(seqs) if seqs else []
        out = path('samples', '.fa')
        write_samples(out, seqs, logp)
        return out
    if the_command == 'compute_fn':
        # ARDCA_fn[_apc]_<base>.txt in the score-file format of plmdca compute_fn; --wildtype_file: the sequence whose double
        # mutants are scored (default: the first record of msa_file); --refseq_file: pairs on the reference's positions
        seqbackmapper = None
        if refseq_file:
            from .sequence_backmapper.sequence_backmapper import SequenceBackmapper
            seqbackmapper = SequenceBackmapper(msa_file=msa_file, refseq_file=refseq_file, biomolecule=instance.biomolecule)
        if apc:
            ranked = instance.compute_sorted_FN_APC(wildtype=wildtype_file, seqbackmapper=seqbackmapper)
            score_type = 'ARDCA epistatic score (Frobenius norm), average product corrected (APC)'
        else:
            ranked = instance.compute_sorted_FN(wildtype=wildtype_file, seqbackmapper=seqbackmapper)
            score_type = 'ARDCA epistatic score (Frobenius norm), non-APC (not average product corrected)'
        out = path('fn_apc' if apc else 'fn', '.txt')
        dca_utilities.write_sorted_dca_scores(out, ranked, metadata=meta, score_type=score_type)
        return out
    if the_command == 'compute_epistasis':
        # float64[L(L-1)/2, q, q] each, all file-site pairs i < j in pair order, first state index at site i
        eps_file, effects_file = path('epistasis', '.npy'), path('double_mutant_effects', '.npy')
        np.save(eps_file, instance.compute_epistasis(wildtype=wildtype_file))
        np.save(effects_file, instance.compute_double_mutant_effects(wildtype=wildtype_file))
        return eps_file, effects_file
    if not wildtype_file:
        raise ardca.ArDCAException('compute_mutation_effects needs --wildtype_file')
    w = _potts.wildtype_codes(wildtype_file, bio, instance.sequences_len, 0, ardca.ArDCAException)
    dlogp = instance.compute_single_mutant_effects(wildtype_file)
    out = path('mutation_effects', '.txt')
    write_mutation_effects(out, dlogp, [letters[c] for c in w], letters, metadata=meta, wildtype_file=wildtype_file)
    return out


def build_parser():
    parser = ArgumentParser(prog='ardca')
    subparsers = parser.add_subparsers(dest='subcommand_name')
    for name in ARDCA_SUBCOMMANDS:
        p = subparsers.add_parser(name)
        p.add_argument('biomolecule', help='protein or rna (case insensitive)')
        p.add_argument('msa_file', help='FASTA formatted multiple sequence alignment')
        p.add_argument('--seqid', type=float)
        p.add_argument('--lambda_h', type=float)
        p.add_argument('--lambda_J', type=float)
        p.add_argument('--max_iterations', type=int)
        p.add_argument('--epsilon', type=float, help='stop when |g| <= epsilon * max(1, |x|) (default 1e-5)')
        p.add_argument('--order', choices=('entropy', 'natural'), help='site order of the model (default: entropy)')
        p.add_argument('--verbose', action='store_true')
        if name == 'compute_log_probabilities':
            p.add_argument('--query_file', help='FASTA file of aligned query sequences (default: the records of msa_file)')
        if name == 'compare_sequences':
            p.add_argument('--query_file', required=True, help='FASTA file of aligned sequences to compare with the alignment; no fit is run')
            p.add_argument('--three_site', type=int, default=0, help='K > 0: also compare the alignment\'s K strongest three-site '
                           'connected correlations, found by a scan of all triples, with the set\'s')
            p.add_argument('--three_site_no_gaps', action='store_true', help='leave elements that name the gap state out of '
                           '--three_site')
            p.add_argument('--pca', type=int, default=0, help='K > 0: also the set\'s mean and variance along the alignment\'s K '
                           'first principal components')
        if name == 'compute_pca':
            _compare.add_pca_arguments(p)
        if name == 'compute_mutation_effects':
            p.add_argument('--wildtype_file', required=True, help='FASTA file with one aligned wild-type sequence')
        if name in ('compute_fn', 'compute_epistasis'):
            p.add_argument('--wildtype_file', help='FASTA file with one aligned sequence whose double mutants are scored '
                                                   '(default: the first record of msa_file)')
        if name == 'compute_fn':
            p.add_argument('--apc', action='store_true', help='average product correction of the scores')
            p.add_argument('--refseq_file', help='FASTA file of the reference sequence the site pairs are mapped onto')
        if name == 'sample_sequences':
            p.add_argument('--num_sequences', type=int, required=True, help='number of independent sequences to draw')
            p.add_argument('--seed', type=int, default=0, help='seed of the counter-based generator')
        p.add_argument('--output_dir')
        p.add_argument('--device', type=int, default=0, help='GPU index')
    return parser


def run_ardca(argv=None):
    parser = build_parser()
    argv = sys.argv[1:] if argv is None else argv
    args = vars(parser.parse_args(args=argv if argv else ['--help']))
    return execute_from_command_line(
        args.get('biomolecule'), args.get('msa_file'), the_command=args.get('subcommand_name'), seqid=args.get('seqid'),
        lambda_h=args.get('lambda_h'), lambda_J=args.get('lambda_J'), max_iterations=args.get('max_iterations'),
        epsilon=args.get('epsilon'), order=args.get('order'), output_dir=args.get('output_dir'), verbose=args.get('verbose'),
        device=args.get('device'), query_file=args.get('query_file'), wildtype_file=args.get('wildtype_file'),
        num_sequences=args.get('num_sequences'), seed=args.get('seed'), apc=bool(args.get('apc')),
        refseq_file=args.get('refseq_file'), three_site=args.get('three_site') or 0,
        three_site_no_gaps=bool(args.get('three_site_no_gaps')), pca=args.get('pca') or 0,
        num_components=args.get('num_components'))


if __name__ == '__main__':
    run_ardca()
