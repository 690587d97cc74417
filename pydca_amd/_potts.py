"""Query sequences of the energy methods of PlmDCA and MeanFieldDCA, encoded for the context (dca_encode_sequences)."""
import os

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


def state_letters(biomolecule):
    """Letter of every 0-based state (gap last), for the CLI's mutation-effect rows."""
    return list('ACDEFGHIKLMNPQRSTVWY-') if biomolecule == _lib.DCA_BIOMOLECULE_PROTEIN else list('ACGU-')



POTTS_SUBCOMMANDS = ('compute_energies', 'compute_mutation_effects')


def run_subcommand(instance, the_command, prefix, msa_file, output_dir, metadata, biomolecule, table, exc_type,
                   query_file=None, wildtype_file=None):
    """compute_energies / compute_mutation_effects of the plmdca and mfdca command lines -> the path of the file written:
    <output_dir>/<prefix>_energies_<alignment base>.txt or <prefix>_mutation_effects_<alignment base>.txt."""
    from .dca_utilities import dca_utilities
    dca_utilities.create_directories(output_dir)
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
