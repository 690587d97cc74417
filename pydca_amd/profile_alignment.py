"""Aligning raw sequences to the columns of a fitted alignment.

A profile is built from the alignment and its sequence weights (build_profile, pure numpy) and the sequences are aligned to it
on the GPU (dca_profile_align: the integer Gotoh recurrence, one wave64 lane per sequence).  The aligned strings have the
alignment's L columns, '-' where a column is deleted, and go straight into the query entries of PlmDCA, MeanFieldDCA and ArDCA
(energies, mutant scans, PLL, log P, distances, projections ...), which take aligned input only."""
import logging
import os

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

MODES = {'local': _lib.DCA_ALIGN_LOCAL, 'glocal': _lib.DCA_ALIGN_GLOCAL}
FORMATS = ('aligned', 'a2m')
MAX_QUERY_LENGTH = 32767
_WEIGHT_QUANTUM = float(1 << 30)


def build_profile(X, weights, q, pseudocount=0.2, deletion_floor=0.02, ins_open_bits=-6.0, ins_extend_bits=-1.0, scale=32):
    """The integer profile of an alignment -> dict(match int32[L, q], del_open int32[L], del_extend int32[L], ins_open int,
    ins_extend int).

    X: uint8[N, L], codes 0 .. q-1 with the gap q-1 (the coding of the library); weights: float[N], the sequence weights.
    The query alphabet is the same q codes; code q-1 of a QUERY means "unknown residue" and scores 0 in every column.

    Every count is a sum of weights quantised to multiples of 2^-30 (rint(w 2^30)), so that it is an exact integer in double
    precision and the tables do not depend on the order of the rows.  With W the sum of the quantised weights:
      f_i(a)    = sum_n w_n [X_ni = a] / W                                  a = 0 .. q-1 (q-1: the gap)
      r_i(a)    = f_i(a) / (1 - f_i(gap))                                   a < q-1; the residue frequencies of column i
      bg0(a)    = mean of r_i(a) over the columns that hold a residue       (uniform if there is none)
      bg(a)     = (1 - pseudocount) bg0(a) + pseudocount / (q - 1)          never 0
      p_i(a)    = (1 - pseudocount) r_i(a) + pseudocount bg(a)              an all-gap column: p_i = bg
      match[i][a]   = rint(scale log2(p_i(a) / bg(a)))                      a < q-1;  match[i][q-1] = 0
      del_open[i]   = rint(scale log2(clip(f_i(gap), deletion_floor, 1)))
      del_extend[i] = rint(scale log2(clip(P(gap at i | gap at i-1), deletion_floor, 1)))   from the weighted counts of the
                      adjacent columns (the floor where column i-1 has no gap);  del_extend[first] = del_open[first]
      ins_open, ins_extend = rint(scale ins_open_bits), rint(scale ins_extend_bits)
    rint rounds half to even (C's llrint).  scale is the number of score units per bit.  pseudocount, deletion_floor and the two
    insertion costs are design parameters for the user to set -- plain defaults, not values tuned on any benchmark."""
    X = np.asarray(X)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError('X must be a code array of shape (N, L)')
    q = int(q)
    if q < 3 or q > 32:
        raise ValueError('q {} is outside 3 .. 32'.format(q))
    if int(X.max()) >= q:
        raise ValueError('X holds the code {} >= q = {}'.format(int(X.max()), q))
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != X.shape[0]:
        raise ValueError('weights must hold one entry per row of X ({}), not {}'.format(X.shape[0], w.size))
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('the weights must be finite and >= 0')
    if not 0.0 < pseudocount <= 1.0:
        raise ValueError('pseudocount {} is outside (0, 1]'.format(pseudocount))
    if not 0.0 < deletion_floor <= 1.0:
        raise ValueError('deletion_floor {} is outside (0, 1]'.format(deletion_floor))
    if ins_open_bits > 0 or ins_extend_bits > 0:
        raise ValueError('ins_open_bits and ins_extend_bits must be <= 0')
    if not scale > 0:
        raise ValueError('scale must be > 0')
    N, L = X.shape
    wq = np.rint(w * _WEIGHT_QUANTUM)
    W = float(wq.sum())
    if W <= 0 or N > (1 << 22):
        raise ValueError('the weights must not all vanish (and N must be <= 2^22)')
    counts = np.empty((L, q), dtype=np.float64)
    for a in range(q):
        counts[:, a] = wq @ (X == a)
    gap = X == (q - 1)
    both = wq @ (gap[:, 1:] & gap[:, :-1]) if L > 1 else np.zeros(0)
    f = counts / W
    fgap = f[:, q - 1]
    has_res = counts[:, :q - 1].sum(axis=1) > 0
    r = np.zeros((L, q - 1))
    r[has_res] = counts[has_res, :q - 1] / counts[has_res, :q - 1].sum(axis=1, keepdims=True)
    uniform = np.full(q - 1, 1.0 / (q - 1))
    bg0 = r[has_res].mean(axis=0) if has_res.any() else uniform
    bg = (1.0 - pseudocount) * bg0 + pseudocount * uniform
    p = (1.0 - pseudocount) * r + pseudocount * bg
    p[~has_res] = bg
    match = np.zeros((L, q), dtype=np.int32)
    match[:, :q - 1] = np.rint(scale * np.log2(p / bg)).astype(np.int32)
    match[~has_res, :q - 1] = 0
    del_open = np.rint(scale * np.log2(np.clip(fgap, deletion_floor, 1.0))).astype(np.int32)
    cond = np.full(L, deletion_floor)
    if L > 1:
        prev = counts[:-1, q - 1]
        ok = prev > 0
        cond[1:][ok] = both[ok] / prev[ok]
    del_extend = np.rint(scale * np.log2(np.clip(cond, deletion_floor, 1.0))).astype(np.int32)
    del_extend[0] = del_open[0]
    return dict(match=match, del_open=np.minimum(del_open, 0), del_extend=np.minimum(del_extend, 0),
                ins_open=int(np.rint(scale * ins_open_bits)), ins_extend=int(np.rint(scale * ins_extend_bits)))


def letter_codes(biomolecule_int, q):
    """uint8[256]: the query code of every byte -- the library's residue table for the letters it knows, q-1 ("unknown", which
    scores 0 in every column) for everything else"""
    letters = ''.join(chr(c) for c in range(ord('A'), ord('Z') + 1))
    known = _lib.encode_sequences([letters], biomolecule_int, len(letters), 1)[0]       # the mf table: unknown -> gap = q-1
    table = np.full(256, q - 1, dtype=np.uint8)
    table[ord('A'):ord('Z') + 1] = known
    return table


def fasta_records(path):
    """(headers, sequences) of a FASTA file in file order: header up to the first blank, multi-line sequences joined, lengths
    free"""
    headers, seqs = [], []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith('>'):
                fields = line[1:].split()
                headers.append(fields[0] if fields else '')
                seqs.append([])
            elif line and seqs:
                seqs[-1].append(line)
    if not headers:
        raise ValueError('no records found in {}'.format(path))
    return headers, [''.join(s) for s in seqs]


def raw_records(sequences):
    """A FASTA path or a list of strings -> the residues: upper-cased, '-' and '.' stripped"""
    if sequences is None:
        raise ValueError('sequences are needed: a FASTA file or a list of strings')
    if isinstance(sequences, (str, bytes, os.PathLike)):
        if not os.path.isfile(os.fsdecode(sequences)):
            raise ValueError('{!r} is not a file; pass a list to align strings'.format(sequences))
        seqs = fasta_records(os.fsdecode(sequences))[1]
    else:
        seqs = [str(getattr(rec, 'seq', rec)) for rec in sequences]
    out = [s.upper().replace('-', '').replace('.', '') for s in seqs]
    for k, s in enumerate(out):
        if len(s) > MAX_QUERY_LENGTH:
            raise ValueError('record {} has {} residues; at most {} can be aligned'.format(k + 1, len(s), MAX_QUERY_LENGTH))
        if not s.isascii() or (s and not s.isalpha()):
            raise ValueError('record {} holds characters that are no letters'.format(k + 1))
    return out


def aligned_strings(raw, residue_at, fmt='aligned'):
    """residue_at int32[n, L] -> the strings.  'aligned': L characters, the input's letter in every matched column, '-' in a
    deleted one.  'a2m': the same with the unmatched residues added in lower case where they fall (those after a deleted
    column in front of the next matched one, the trailing ones at the end)."""
    out = []
    for s, res in zip(raw, np.asarray(residue_at)):
        if fmt == 'aligned':
            out.append(''.join(s[r] if r >= 0 else '-' for r in res))
            continue
        parts, nxt = [], 0
        for r in res:
            if r >= 0:
                parts.append(s[nxt:r].lower())
                parts.append(s[r])
                nxt = r + 1
            else:
                parts.append('-')
        parts.append(s[nxt:].lower())
        out.append(''.join(parts))
    return out


def check_mode_format(mode, fmt):
    if mode not in MODES:
        raise ValueError("mode {!r} is neither 'local' nor 'glocal'".format(mode))
    if fmt not in FORMATS:
        raise ValueError("format {!r} is neither 'aligned' nor 'a2m'".format(fmt))


def align_to_profile(ctx, profile, table, sequences, mode='glocal', format='aligned'):
    """-> dict(aligned: list of str, scores: int32[n], residue_at: int32[n, L], num_inserted: int32[n], the residues of each
    sequence that no column took -- overhangs included)"""
    check_mode_format(mode, format)
    raw = raw_records(sequences)
    codes = [table[np.frombuffer(s.encode('ascii'), dtype=np.uint8)] for s in raw]
    scores, res = ctx.profile_align(profile['match'], profile['del_open'], profile['del_extend'], profile['ins_open'],
                                    profile['ins_extend'], MODES[mode], codes, traceback=True)
    lens = np.array([len(s) for s in raw], dtype=np.int32)
    return dict(aligned=aligned_strings(raw, res, format), scores=scores, residue_at=res,
                num_inserted=(lens - (res >= 0).sum(axis=1)).astype(np.int32))


class ProfileAligner:
    """ProfileAligner(msa_file, 'protein' | 'rna', seqid=0.8, device=0, **profile_args): reads the alignment (every record, as
    the mfDCA reader encodes it), weighs its sequences at `seqid` on the GPU and builds the profile (build_profile takes
    profile_args).  .align(sequences) aligns raw sequences to its L columns."""

    def __init__(self, msa_file, biomolecule, seqid=0.8, device=0, **profile_args):
        from .msa_trimmer.msa_trimmer import read_fasta_records
        self.msa_file = msa_file
        self.biomolecule = biomolecule.strip().upper()
        if self.biomolecule not in ('PROTEIN', 'RNA'):
            raise ValueError('biomolecule {!r} is neither PROTEIN nor RNA'.format(biomolecule))
        if not 0.0 < float(seqid) <= 1.0:
            raise ValueError('seqid {} is outside (0, 1]'.format(seqid))
        self.q = 21 if self.biomolecule == 'PROTEIN' else 5
        self._bio = _lib.PROTEIN if self.q == 21 else _lib.RNA
        rows = [r.seq.upper() for r in read_fasta_records(msa_file)]
        self.X = _lib.encode_sequences(rows, self._bio, len(rows[0]), 1)
        self.num_sequences, self.sequences_len = self.X.shape
        self._ctx = _lib.Context(device, _lib.DCA_F64)
        try:
            self._ctx.set_msa(self.X, self.q)
            self.weights = self._ctx.compute_weights(float(seqid), _lib.DCA_F64)
            self.profile = build_profile(self.X, self.weights, self.q, **profile_args)
        except Exception:
            self.close()
            raise
        self._table = letter_codes(self._bio, self.q)

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def align(self, sequences, mode='glocal', format='aligned'):
        return align_to_profile(self._ctx, self.profile, self._table, sequences, mode, format)


class SequenceAlignment:
    """Mixin of PlmDCA, MeanFieldDCA and ArDCA beside _compare.SequenceComparison, whose hooks it uses: the profile comes from
    the context's alignment (in the library's coding, columns back in file order) and its weights."""

    def align_sequences(self, sequences, mode='glocal', format='aligned', **profile_args):
        """Raw sequences (a FASTA path or a list of strings, any lengths) aligned to the L columns of the model's alignment ->
        dict(aligned, scores, residue_at, num_inserted); m.compute_sequence_energies(m.align_sequences(raw)['aligned']) scores
        them.  profile_args: build_profile's.  The profile is kept until other profile_args are given."""
        self._compare_one_gpu('align_sequences')
        try:
            check_mode_format(mode, format)
            key = tuple(sorted(profile_args.items()))
            cached = getattr(self, '_alignment_profile', None)
            ctx = self._compare_context()
            bio, _L, q = self._compare_dims()
            if cached is None or cached[0] != key:
                X = ctx.msa()
                order = self._compare_order()
                if order is not None:
                    Xf = np.empty_like(X)
                    Xf[:, np.asarray(order)] = X          # position j of the context holds file site order[j]
                    X = Xf
                cached = (key, build_profile(X, ctx.weights(), q, **profile_args), letter_codes(bio, q))
                self._alignment_profile = cached
            return align_to_profile(ctx, cached[1], cached[2], sequences, mode, format)
        except (ValueError, TypeError) as exc:
            if isinstance(exc, self._compare_exc):
                raise
            raise self._compare_exc('align_sequences: {}'.format(exc))


# ---------------------------------------------------------------- the sub-command of `pydca`
ALIGN_SUBCOMMANDS = ['align_sequences']


def add_subparsers(subparsers):
    p = subparsers.add_parser('align_sequences', help='Aligns the raw sequences of a FASTA file to the columns of the MSA')
    p.add_argument('biomolecule')
    p.add_argument('msa_file')
    p.add_argument('sequences_file')
    p.add_argument('--mode', choices=sorted(MODES), default='glocal')
    p.add_argument('--a2m', action='store_true', help='adds the unmatched residues in lower case')
    p.add_argument('--seqid', type=float, default=0.8)
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--verbose', action='store_true')
    p.add_argument('--output_dir')


def execute(msa_file, biomolecule, sequences_file, mode='glocal', a2m=False, seqid=0.8, device=0, output_dir=None, aligner_class=None):
    """Writes Aligned_<raw>/Aligned_<raw>.fa and Aligned_<raw>_scores.txt -> the two paths.  aligner_class: a stand-in for
    ProfileAligner (tests)."""
    from .dca_utilities import dca_utilities
    check_mode_format(mode, 'a2m' if a2m else 'aligned')
    if not output_dir:
        base, _ext = os.path.splitext(os.path.basename(sequences_file))
        output_dir = 'Aligned_' + base
    headers, raw = fasta_records(sequences_file)
    aligner = (aligner_class or ProfileAligner)(msa_file, biomolecule, seqid=seqid, device=device)
    try:
        res = aligner.align(raw, mode=mode, format='a2m' if a2m else 'aligned')
    finally:
        if hasattr(aligner, 'close'):
            aligner.close()
    dca_utilities.create_directories(output_dir)
    files = [dca_utilities.get_dca_output_file_path(output_dir, sequences_file, prefix='Aligned_', postfix='.fa'),
             dca_utilities.get_dca_output_file_path(output_dir, sequences_file, prefix='Aligned_', postfix='_scores.txt')]
    with open(files[0], 'w') as fh:
        for h, s in zip(headers, res['aligned']):
            fh.write('>%s\n%s\n' % (h, s))
    with open(files[1], 'w') as fh:
        fh.write('# mode: %s\n# record\theader\tscore\tmatched columns\tunmatched residues\n' % mode)
        for k, h in enumerate(headers):
            fh.write('%d\t%s\t%d\t%d\t%d\n' % (k, h, res['scores'][k], int((res['residue_at'][k] >= 0).sum()), res['num_inserted'][k]))
    return files
