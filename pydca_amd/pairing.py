"""Pairing interaction partners across two alignments by the iterative pairing algorithm (IPA; Bitbol, Dwyer, Colwell, Wingreen,
PNAS 113:12180, 2016) on the GPU: every round is one mean-field fit on the concatenated alignment of the
pairs trusted so far, the inter-protein energies of all within-species pairs in one call (dca_mf_interaction_energies), one
assignment per species (dca_assign_partners) and a ranking of the assigned pairs by their energy gap."""
import logging
import os

import numpy as np

from . import _lib, _potts
from .fasta_reader import fasta_reader

logger = logging.getLogger(__name__)

PAIRING_TAG = 6     # Philox tag of the random start (tags 0 .. 5: the samplers, csrc/dca_internal.h)


class IterativePairingException(Exception):
    """Raised for inputs the pairing cannot use."""


def _records(source):
    """a FASTA path -> (names, sequences) in file order, duplicates kept; in-memory records -> (None or names, sequences)"""
    if isinstance(source, (str, bytes, os.PathLike)):
        path = os.fsdecode(source)
        names = []
        with open(path) as fh:
            names = [ln[1:].strip() for ln in fh if ln.startswith('>')]
        seqs = fasta_reader.get_alignment_from_fasta_file(path, same_length=False)
        if len(names) != len(seqs):
            names = ['record_{}'.format(k + 1) for k in range(len(seqs))]
        return names, seqs
    recs = list(source)
    names = [str(getattr(r, 'id', 'record_{}'.format(k + 1))) for k, r in enumerate(recs)]
    return names, [str(getattr(r, 'seq', r)) for r in recs]


def random_pairing(rows_a, rows_b, seed):
    """A one-to-one random pairing within every species, a function of the seed alone: Fisher-Yates over the species' B rows
    (position k = n - 1 down to 1 is swapped with position floor(U (k + 1))), U = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53 from
    dca_philox4x32_10 with key (seed lo, seed hi) and counter (species index, k, 0, PAIRING_TAG); the first min(nA, nB) A rows
    of the species take the shuffled B rows in order."""
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    pairs = []
    for g, (ra, rb) in enumerate(zip(rows_a, rows_b)):
        perm = [int(b) for b in rb]
        for k in range(len(perm) - 1, 0, -1):
            w = _lib.philox4x32_10((g & 0xffffffff, k, 0, PAIRING_TAG), key)
            u = ((int(w[0]) >> 5) * 67108864 + (int(w[1]) >> 6)) * 2.0 ** -53
            t = int(u * (k + 1))
            perm[k], perm[t] = perm[t], perm[k]
        pairs += [(int(a), b) for a, b in zip(ra, perm)]
    return pairs


class IterativePairing:
    """msa_a / msa_b: FASTA files or in-memory records (strings or objects with .seq) of the two proteins; species_a /
    species_b: one label (any hashable) per record.  Rows are never de-duplicated; a species present on one side only is left
    out and listed in .dropped_species.  training_pairs: (A row, B row) pairs known to be right (0-based record indices), or
    None: round 1 then trains on random_pairing(seed).  The rows of the training pairs are trained on in every round and are
    taken out of the testing set (they are never assigned, and are not among the returned pairs).  The iteration is mean-field
    only."""

    def __init__(self, msa_a, msa_b, species_a, species_b, biomolecule, training_pairs=None, n_increment=6, pseudocount=0.5, seqid=0.8,
                 gauge='zero_sum', seed=0, device=0):
        bio = str(biomolecule).strip().upper()
        if bio not in ('PROTEIN', 'RNA'):
            raise IterativePairingException('biomolecule must be protein or RNA, not {!r}'.format(biomolecule))
        self.biomolecule = _lib.DCA_BIOMOLECULE_PROTEIN if bio == 'PROTEIN' else _lib.DCA_BIOMOLECULE_RNA
        self.q = 21 if bio == 'PROTEIN' else 5
        if gauge not in _lib.GAUGES:
            raise IterativePairingException('gauge must be one of {}'.format(sorted(_lib.GAUGES)))
        if int(n_increment) < 1:
            raise IterativePairingException('n_increment must be at least 1')
        self.names_a, seqs_a = _records(msa_a)
        self.names_b, seqs_b = _records(msa_b)
        if not seqs_a or not seqs_b:
            raise IterativePairingException('an alignment is empty')
        self.LA, self.LB = len(seqs_a[0]), len(seqs_b[0])
        self.XA = _potts.query_codes(seqs_a, self.biomolecule, self.LA, 1, IterativePairingException)
        self.XB = _potts.query_codes(seqs_b, self.biomolecule, self.LB, 1, IterativePairingException)
        self.species, self.rows_a, self.rows_b, self.dropped_species = _potts.species_blocks(
            species_a, species_b, self.XA.shape[0], self.XB.shape[0], IterativePairingException)
        if species_a is None:
            raise IterativePairingException('the species labels are required')
        if self.dropped_species:
            logger.warning('\n\tSpecies on one side only are left out: {}'.format(self.dropped_species))
        if not self.species:
            raise IterativePairingException('no species is present on both sides')
        self.training_pairs = [] if training_pairs is None else [(int(a), int(b)) for a, b in training_pairs]
        for a, b in self.training_pairs:
            if not (0 <= a < self.XA.shape[0] and 0 <= b < self.XB.shape[0]):
                raise IterativePairingException('training pair ({}, {}) is out of range'.format(a, b))
        self.n_increment, self.pseudocount, self.seqid = int(n_increment), float(pseudocount), float(seqid)
        self.gauge, self.seed, self.device = gauge, int(seed), int(device)
        # as in the paper, the rows of the training pairs leave the testing set: they are trained on every round and never assigned
        used_a, used_b = {a for a, _ in self.training_pairs}, {b for _, b in self.training_pairs}
        self.rows_a = [np.array([r for r in ra if int(r) not in used_a], dtype=np.int64) for ra in self.rows_a]
        self.rows_b = [np.array([r for r in rb if int(r) not in used_b], dtype=np.int64) for rb in self.rows_b]
        self.GA, self.GB, self.offsets_a, self.offsets_b = _potts.grouped_rows(self.XA, self.XB, self.rows_a, self.rows_b)
        self.model_context = None
        self.pairs = self.gaps = self.energies = self.pair_species = self.history = None

    def _round(self, train):
        """one fit on the concatenated rows of `train` and the ranked assignment of all species under it"""
        if self.model_context is not None:
            self.model_context.close()
        ctx = _lib.Context(self.device, _lib.DCA_F64)
        ia, ib = [a for a, _ in train], [b for _, b in train]
        ctx.set_msa(np.concatenate([self.XA[ia], self.XB[ib]], axis=1), self.q)
        ctx.compute_weights(self.seqid, _lib.DCA_F64)
        ctx.mf_run(self.pseudocount, True)
        blocks = ctx.mf_interaction_energies(self.GA, self.GB, self.LA, self.offsets_a, self.offsets_b, gauge=self.gauge)
        self.model_context = ctx
        return _potts.rank_matches(blocks, self.rows_a, self.rows_b, self.species), ctx.meff()

    def run(self, max_rounds=None, true_pairs=None):
        """Round n trains on the training pairs plus the (n - 1) n_increment highest-gap pairs of round n - 1 (re-picked every
        round).  Stops after the round that trained on every pair assigned in the round before, or at max_rounds.  That is a
        deliberate reading of "the round in which every assigned pair was in the training set": the training set of a round is
        fixed before its assignment, so the round whose training set took all pairs of the previous assignment is the last one
        that can add anything, whether or not its own assignment moves a pair.
        -> dict: pairs int64[n, 2], gaps, energies, species (ranked by gap) and history (per round: training_size, meff,
        mean_gap (over the finite gaps), selected (the pairs trained on) and, with true_pairs, true_positive_fraction)."""
        truth = None if true_pairs is None else set((int(a), int(b)) for a, b in true_pairs)
        start = list(self.training_pairs) if self.training_pairs else random_pairing(self.rows_a, self.rows_b, self.seed)
        history, res, rnd, took_all = [], None, 0, False
        while True:
            rnd += 1
            if rnd == 1:
                train = start
            else:
                free = [(int(a), int(b)) for a, b in res['pairs']]
                extra = free[:(rnd - 1) * self.n_increment]
                took_all = len(extra) == len(free)
                train = list(self.training_pairs) + extra
            res, meff = self._round(train)
            finite = res['gaps'][np.isfinite(res['gaps'])]
            rec = dict(round=rnd, training_size=len(train), meff=float(meff), mean_gap=float(finite.mean()) if finite.size else 0.0,
                       selected=list(train))
            if truth is not None:
                rec['true_positive_fraction'] = sum((int(a), int(b)) in truth for a, b in res['pairs']) / max(len(res['pairs']), 1)
            history.append(rec)
            logger.info('\n\tround {}: trained on {} pairs, Meff {:.1f}, mean gap {:.4g}'.format(rnd, len(train), meff, rec['mean_gap']))
            if took_all or (max_rounds is not None and rnd >= max_rounds):
                break
        self.pairs, self.gaps, self.energies, self.pair_species, self.history = res['pairs'], res['gaps'], res['energies'], res['species'], history
        return dict(pairs=res['pairs'], gaps=res['gaps'], energies=res['energies'], species=res['species'], history=history)


# ---------------------------------------------------------------- the pair_partners sub-command of the mfdca command line
PAIR_SUBCOMMAND = 'pair_partners'


def add_pair_partners_parser(subparsers):
    p = subparsers.add_parser(PAIR_SUBCOMMAND)
    p.add_argument('biomolecule')
    p.add_argument('msa_file_a')
    p.add_argument('msa_file_b')
    p.add_argument('--species_a', required=True, help='file with one species label per record of msa_file_a, in file order')
    p.add_argument('--species_b', required=True, help='the same for msa_file_b')
    p.add_argument('--training_pairs', help='file of known pairs: one "A record B record" (1-based) per line')
    p.add_argument('--n_increment', type=int, default=6)
    p.add_argument('--max_rounds', type=int)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--seqid', type=float, default=0.8)
    p.add_argument('--pseudocount', type=float, default=0.5)
    p.add_argument('--gauge', choices=sorted(_lib.GAUGES), default='zero_sum')
    p.add_argument('--output_dir')
    p.add_argument('--device', type=int, default=0)
    p.add_argument('--verbose', action='store_true')
    return p


def run_pair_partners(args):
    """-> the paths of <output_dir>/MFDCA_partner_pairs_<A base>_<B base>.txt (A id, B id, species, gap in rank order) and
    MFDCA_partner_pairs_history_<A base>_<B base>.txt (one line per round)"""
    training = None
    if args.get('training_pairs'):
        with open(args['training_pairs']) as fh:
            training = [(int(t[0]) - 1, int(t[1]) - 1) for t in (ln.split() for ln in fh if ln.strip() and not ln.startswith('#'))]
    ip = IterativePairing(args['msa_file_a'], args['msa_file_b'], _potts.read_labels(args['species_a']), _potts.read_labels(args['species_b']),
                          args['biomolecule'], training_pairs=training, n_increment=args.get('n_increment') or 6,
                          pseudocount=args.get('pseudocount') or 0.5, seqid=args.get('seqid') or 0.8, gauge=args.get('gauge') or 'zero_sum',
                          seed=args.get('seed') or 0, device=args.get('device') or 0)
    res = ip.run(max_rounds=args.get('max_rounds'))
    base = '{}_{}'.format(os.path.splitext(os.path.basename(args['msa_file_a']))[0], os.path.splitext(os.path.basename(args['msa_file_b']))[0])
    out = args.get('output_dir') or 'MFDCA_output_' + base
    os.makedirs(out, exist_ok=True)
    pairs_path = os.path.join(out, 'MFDCA_partner_pairs_{}.txt'.format(base))
    with open(pairs_path, 'w') as fh:
        fh.write('# Partner pairs by the iterative pairing algorithm, ranked by gap\n')
        fh.write('# rounds {}, n_increment {}, seed {}, gauge {}\n'.format(len(res['history']), ip.n_increment, ip.seed, ip.gauge))
        if ip.dropped_species:
            fh.write('# Species on one side only (left out): {}\n'.format(', '.join(str(s) for s in ip.dropped_species)))
        fh.write('# A id\tB id\tspecies\tgap\n')
        for (a, b), s, g in zip(res['pairs'], res['species'], res['gaps']):
            fh.write('{}\t{}\t{}\t{!r}\n'.format(ip.names_a[a], ip.names_b[b], s, float(g)))
    hist_path = os.path.join(out, 'MFDCA_partner_pairs_history_{}.txt'.format(base))
    with open(hist_path, 'w') as fh:
        fh.write('# round\ttraining size\tMeff\tmean gap\n')
        for rec in res['history']:
            fh.write('{}\t{}\t{!r}\t{!r}\n'.format(rec['round'], rec['training_size'], rec['meff'], rec['mean_gap']))
    ip.model_context.close()
    return pairs_path, hist_path
