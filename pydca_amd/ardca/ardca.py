"""ArDCA -- the autoregressive Potts model (Trinquier et al., Nat. Commun. 2021) fitted and used on the GPU (ardca.hip).

P(s) = prod_l P(s_l | s_<l) over the sites in the model's order.  Every conditional is normalised, so log P(s) is exact and
one pass over the sites draws an exact, independent sample.  The library works in model order (the columns of the context's
alignment); this class permutes the file's columns into it and every method takes and returns sites in the FILE's order.
No pydca counterpart.
"""
import logging
import math
import os

import numpy as np

from .. import _compare, _lib, _potts, _ranking, profile_alignment
from ..fasta_reader import fasta_reader

logger = logging.getLogger(__name__)


class ArDCAException(Exception):
    """Raised for invalid arguments of ArDCA (host checks, before any device work)."""


def site_entropies(X, weights, q):
    """Entropy of the weighted single-site frequencies f_i(a) = sum_n w_n [X_ni = a] / sum_n w_n (no pseudocount, 0 log 0 = 0)
    -> float64[L]."""
    X = np.asarray(X)
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    f = np.stack([(w[:, None] * (X == a)).sum(axis=0) for a in range(q)], axis=1) / w.sum()
    logf = np.log(np.where(f > 0.0, f, 1.0))
    return -(f * logf).sum(axis=1)


def entropic_order(X, weights, q):
    """Sites by ascending entropy of the weighted frequencies, ties in ascending site number -> int64[L]."""
    return np.argsort(site_entropies(X, weights, q), kind='stable').astype(np.int64)


def explicit_order(order, L):
    """An explicit permutation of range(L) -> int64[L]; ArDCAException otherwise."""
    try:
        perm = np.asarray(order)
    except Exception:
        raise ArDCAException('order must be \'entropy\', \'natural\' or a permutation of range({})'.format(L))
    if perm.ndim != 1 or perm.size != L or not (np.issubdtype(perm.dtype, np.integer) or perm.size == 0):
        raise ArDCAException('order must be \'entropy\', \'natural\' or a permutation of range({}), not {!r}'.format(L, order))
    perm = perm.astype(np.int64)
    if not np.array_equal(np.sort(perm), np.arange(L)):
        raise ArDCAException('order is not a permutation of range({})'.format(L))
    return perm


def _number(name, v, low, integer=False):
    if isinstance(v, bool) or v is None:
        raise ArDCAException('{} must be a number, not {!r}'.format(name, v))
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ArDCAException('{} must be a number, not {!r}'.format(name, v))
    if not math.isfinite(f) or f < low or (integer and int(f) != f):
        raise ArDCAException('{} must be {} >= {}, not {!r}'.format(name, 'an integer' if integer else 'a finite number', low, v))
    return int(f) if integer else f


def checked_pairs(pairs, L):
    """pairs of compute_epistasis: a list of (i, j), i != j, 0-based file sites -> int64[P, 2]; ArDCAException otherwise."""
    try:
        arr = np.asarray(pairs)
    except Exception:
        raise ArDCAException('pairs must be a list of (i, j) site pairs, not {!r}'.format(pairs))
    if arr.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2 or arr.dtype == np.bool_ or not np.issubdtype(arr.dtype, np.integer):
        raise ArDCAException('pairs must be a list of (i, j) pairs of integer sites, not {!r}'.format(pairs))
    arr = arr.astype(np.int64)
    if arr.min() < 0 or arr.max() >= L:
        raise ArDCAException('a site of pairs lies outside 0 .. {}'.format(L - 1))
    same = np.nonzero(arr[:, 0] == arr[:, 1])[0]
    if same.size:
        raise ArDCAException('pair {} names site {} twice'.format(int(same[0]), int(arr[same[0], 0])))
    return arr


def model_pairs(site_order, pairs):
    """File-site pairs (i, j) -> (index of the model's pair block, transposed?): the block of the model positions of i and j in
    pair order, and whether the model places j before i (the block then has j's state first)."""
    L = len(site_order)
    inv = np.argsort(np.asarray(site_order, dtype=np.int64))
    pi, pj = inv[pairs[:, 0]], inv[pairs[:, 1]]
    k, l = np.minimum(pi, pj), np.maximum(pi, pj)
    return L * (L - 1) // 2 - (L - k) * (L - k - 1) // 2 + (l - k - 1), pi > pj


def file_pair_blocks(blocks_model, site_order, pairs):
    """blocks_model float64[pairs of the model, q, q] (pair order over model positions, first index the earlier position) ->
    float64[P, q, q] for the file-site pairs (i, j): first index the state of site i."""
    idx, transposed = model_pairs(site_order, pairs)
    out = np.array(blocks_model[idx], dtype=np.float64)
    out[transposed] = np.transpose(out[transposed], (0, 2, 1))
    return out


def file_pair_scores(scores_model, site_order):
    """A symmetric pair score in pair order over model positions -> the same in pair order over file sites."""
    L = len(site_order)
    iu, ju = np.triu_indices(L, k=1)
    idx, _t = model_pairs(site_order, np.stack([iu, ju], axis=1))
    return np.asarray(scores_model)[idx]


class ArDCA(_compare.SequenceComparison, profile_alignment.SequenceAlignment):
    """arDCA of a FASTA alignment: ArDCA(msa_file, 'protein' | 'rna', seqid=0.8, lambda_h=1e-6, lambda_J=1e-2,
    max_iterations=1000, epsilon=1e-5, order='entropy', device=0).  lambda_h, lambda_J weigh the L2 penalty against the
    weighted log-likelihood per effective sequence.  order: 'entropy' (ascending entropy of the weighted
    site frequencies), 'natural' (file order) or an explicit permutation of range(L) (model position j holds file site
    order[j])."""

    def __init__(self, msa_file, biomolecule, seqid=0.8, lambda_h=1e-6, lambda_J=1e-2, max_iterations=1000, epsilon=1e-5,
                 order='entropy', device=0):
        if not isinstance(biomolecule, str) or biomolecule.strip().upper() not in ('PROTEIN', 'RNA'):
            raise ArDCAException('biomolecule must be protein or rna, not {!r}'.format(biomolecule))
        self.__biomolecule = biomolecule.strip().upper()
        self.__biomolecule_int = _lib.DCA_BIOMOLECULE_PROTEIN if self.__biomolecule == 'PROTEIN' else _lib.DCA_BIOMOLECULE_RNA
        self.__q = 21 if self.__biomolecule == 'PROTEIN' else 5
        self.__seqid = _number('seqid', seqid, 0.0)
        if not 0.0 < self.__seqid <= 1.0:
            raise ArDCAException('seqid = {} lies outside (0, 1]'.format(seqid))
        self.__lambda_h = _number('lambda_h', lambda_h, 0.0)
        self.__lambda_J = _number('lambda_J', lambda_J, 0.0)
        self.__max_iterations = _number('max_iterations', max_iterations, 0, integer=True)
        self.__epsilon = _number('epsilon', epsilon, 0.0)
        self.__device = _number('device', device, 0, integer=True)
        if isinstance(order, str):
            if order not in ('entropy', 'natural'):
                raise ArDCAException('order must be \'entropy\', \'natural\' or a permutation, not {!r}'.format(order))
        self.__msa_file = os.fsdecode(msa_file)
        if not os.path.isfile(self.__msa_file):
            raise FileNotFoundError(self.__msa_file)
        self.__num_seqs, self.__L = _lib.fasta_shape(self.__msa_file)
        self.__order_arg = order if isinstance(order, str) else explicit_order(order, self.__L)
        self.__order = None if isinstance(order, str) and order == 'entropy' else (
            np.arange(self.__L, dtype=np.int64) if isinstance(order, str) else self.__order_arg)
        self.__ctx = None
        self.__fitted = False
        self.__weights = None
        self.last_status = None

    # ---- properties
    @property
    def biomolecule(self):
        return self.__biomolecule

    @property
    def sequence_identity(self):
        return self.__seqid

    @property
    def lambda_h(self):
        return self.__lambda_h

    @property
    def lambda_J(self):
        return self.__lambda_J

    @property
    def max_iterations(self):
        return self.__max_iterations

    @property
    def epsilon(self):
        return self.__epsilon

    @property
    def sequences_len(self):
        return self.__L

    @property
    def num_sequences(self):
        return self.__num_seqs

    @property
    def num_site_states(self):
        return self.__q

    @property
    def order(self):
        return self.__order_arg if isinstance(self.__order_arg, str) else 'explicit'

    @property
    def site_order(self):
        """The model's site order: model position j is file site site_order[j] (int64[L])."""
        if self.__order is None:
            self._context()
        return self.__order.copy()

    # ---- the context
    def _context(self):
        """Alignment (columns in model order), weights and configuration on the device; no fit."""
        if self.__ctx is not None:
            return self.__ctx
        X, _raw = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__L)
        ctx = _lib.Context(self.__device, _lib.DCA_F64)
        ctx.set_msa(X, self.__q)
        w = ctx.compute_weights(self.__seqid, _lib.DCA_F64)
        if self.__order is None:
            self.__order = entropic_order(X, w, self.__q)
        if not np.array_equal(self.__order, np.arange(self.__L)):
            ctx.set_msa(np.ascontiguousarray(X[:, self.__order]), self.__q)
            ctx.set_weights(w)
        ctx.ar_configure(self.__lambda_h, self.__lambda_J)
        self.__weights = w
        self.__ctx = ctx
        return ctx

    # ---- sequence sets against the alignment (_compare.SequenceComparison): the unfitted context serves; its columns are in
    # model order, so the queries are permuted the same way and distances and row indices come out as for the file's order
    _compare_exc = ArDCAException
    _compare_table = 0
    _compare_logger = logger

    def _compare_dims(self):
        return self.__biomolecule_int, self.__L, self.__q

    def _compare_devices(self):
        return None

    def _compare_context(self):
        return self._context()

    def _compare_order(self):
        self._context()
        return None if np.array_equal(self.__order, np.arange(self.__L)) else self.__order

    def _fitted_context(self):
        """The fitted model; fitted once here on first use."""
        ctx = self._context()
        if not self.__fitted:
            self.fit()
        return ctx

    def fit(self):
        """Fits the model from x = 0 by L-BFGS on the device -> dict(status, iterations, evaluations, fx, gnorm, seconds),
        also kept as last_status.  status: 'converged', 'max_iterations' or 'line_search_failed'."""
        ctx = self._context()
        ctx.ar_init_x()
        logger.info('\n\tarDCA fit: L-BFGS, at most {} iterations, epsilon {}'.format(self.__max_iterations, self.__epsilon))
        st = ctx.ar_fit(self.__max_iterations, self.__epsilon)
        names = {_lib.AR_CONVERGED: 'converged', _lib.AR_MAX_ITERATIONS: 'max_iterations',
                 _lib.AR_LINE_SEARCH_FAILED: 'line_search_failed'}
        st = dict(st, status=names.get(st['status'], st['status']), unique_sequences=int(ctx.N))
        self.__fitted = True
        self.last_status = st
        return dict(st)

    def get_fields_and_couplings(self):
        """-> (x, site_order): x float64 in the plm layout over the MODEL's sites (fields L*q, then the q x q blocks of the pairs
        k < l of model positions, element a*q + b = J_kl(a at k, b at l)), and the model's site order."""
        ctx = self._fitted_context()
        return ctx.ar_get_x(), self.site_order

    # ---- queries (file order in, file order out)
    def _query(self, sequences):
        src = self.__msa_file if sequences is None else sequences
        return _potts.query_codes(src, self.__biomolecule_int, self.__L, 0, ArDCAException)

    def _to_model(self, X):
        return np.ascontiguousarray(X[:, self.__order])

    def _log_probabilities(self, X, per_site=False, conditionals=False):
        ctx = self._fitted_context()
        res = ctx.ar_log_probabilities(self._to_model(X), per_site=per_site, conditionals=conditionals)
        if not per_site and not conditionals:
            return res
        inv = np.argsort(self.__order)
        return (res[0],) + tuple(a[:, inv] for a in res[1:])

    def compute_sequence_log_probabilities(self, sequences=None, per_site=False):
        """Exact log P(s) -> float64[n], or (float64[n], float64[n, L] of log P(s_i | the sites before i in the model's
        order), sites in file order) with per_site.  sequences: None (every record of the training file, in file order,
        duplicates kept), a FASTA path or a list of aligned strings."""
        per_site = _potts.pll_flag(per_site, ArDCAException)
        X = self._query(sequences)
        logger.info('\n\tarDCA log-probabilities of {} sequences'.format(X.shape[0]))
        return self._log_probabilities(X, per_site=per_site)

    def compute_conditional_log_probabilities(self, sequences):
        """log P(s_i = a | the sites before i in the model's order) for every site i (file order) and state a (gap last)
        -> float64[n, L, q], or float64[L, q] for a single aligned string."""
        single = _potts.single_query(sequences, ArDCAException)
        X = self._query([sequences] if single else sequences)
        _logp, cond = self._log_probabilities(X, conditionals=True)
        return cond[0] if single else cond

    def compute_log_likelihood(self):
        """sum_n W_n log P(s_n), W_n = w_n / sum w, over the de-duplicated training alignment and its weights -> float (exact:
        no log Z)."""
        ctx = self._fitted_context()
        X, _raw = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__L)
        logp = self._log_probabilities(X)
        w = self.__weights
        return float(np.dot(w, logp)) / float(w.sum())

    def sample_sequences(self, num_sequences, seed=0, return_codes=False):
        """num_sequences exact, independent samples by ancestral sampling (one pass over the sites in model order) from a
        counter-based generator of `seed` -> aligned strings (gap '-'), or uint8[n, L] codes (file order) with return_codes."""
        n = _number('num_sequences', num_sequences, 0, integer=True)
        seed = _number('seed', seed, 0, integer=True)
        ctx = self._fitted_context()
        logger.info('\n\tarDCA ancestral sampling of {} sequences'.format(n))
        model = ctx.ar_sample(n, seed=seed)
        codes = np.empty_like(model)
        codes[:, self.__order] = model
        if return_codes:
            return codes
        letters = _potts.state_letters(self.__biomolecule_int)
        return [''.join(letters[c] for c in row) for row in codes]

    def compute_single_mutant_effects(self, wildtype):
        """dlogP(i, a) = log P(wild type with site i set to a) - log P(wild type) for every site i (file order) and state a
        (gap last) -> float64[L, q]; 0 on the wild type's own states.  wildtype: an aligned string or a FASTA file with one
        record."""
        w = _potts.wildtype_codes(wildtype, self.__biomolecule_int, self.__L, 0, ArDCAException)
        L, q = self.__L, self.__q
        batch = np.repeat(w[None, :], L * q + 1, axis=0)
        idx = np.arange(L * q)
        batch[idx, idx // q] = (idx % q).astype(np.uint8)
        logp = self._log_probabilities(batch)
        return (logp[:L * q] - logp[L * q]).reshape(L, q)

    # ---- double mutants and contacts (ar_epistasis.hip)
    def _wildtype(self, wildtype):
        """-> uint8[L] codes in file order; None: the first record of the training file."""
        if wildtype is None:
            records = fasta_reader.get_alignment_from_fasta_file(self.__msa_file, same_length=False)
            if not records:
                raise ArDCAException('the training file {} holds no record'.format(self.__msa_file))
            wildtype = str(records[0])
        return _potts.wildtype_codes(wildtype, self.__biomolecule_int, self.__L, 0, ArDCAException)

    def _all_pairs(self):
        iu, ju = np.triu_indices(self.__L, k=1)
        return np.stack([iu, ju], axis=1).astype(np.int64)

    def _epistasis(self, wildtype, pairs, single):
        w = self._wildtype(wildtype)
        pairs = self._all_pairs() if pairs is None else checked_pairs(pairs, self.__L)
        ctx = self._fitted_context()
        logger.info('\n\tarDCA epistasis of the wild type, {} site pairs'.format(pairs.shape[0]))
        eps, d = ctx.ar_epistasis(w[self.__order], single=single)
        blocks = file_pair_blocks(eps, self.__order, pairs)
        return (blocks, pairs, d[np.argsort(self.__order)]) if single else (blocks, pairs, None)

    def compute_epistasis(self, wildtype=None, pairs=None):
        """eps_ij(a, b) = log P(wt with i -> a, j -> b) - log P(wt with i -> a) - log P(wt with j -> b) + log P(wt): the
        non-additive part of every double mutant of the wild type -> float64[P, q, q], a the state of site i (gap last); 0 where
        a or b is the wild type's own state.  pairs: a list of (i, j), i != j, 0-based file sites; None: all i < j in pair order.
        wildtype: an aligned string or a FASTA file with one record; None: the first record of the training file."""
        return self._epistasis(wildtype, pairs, False)[0]

    def compute_double_mutant_effects(self, wildtype=None, pairs=None):
        """log P(wt with i -> a, j -> b) - log P(wt) = d_i(a) + d_j(b) + eps_ij(a, b) -> float64[P, q, q]; arguments as
        compute_epistasis."""
        eps, pairs, d = self._epistasis(wildtype, pairs, True)
        return d[pairs[:, 0]][:, :, None] + d[pairs[:, 1]][:, None, :] + eps

    def get_mapped_site_pairs_dca_scores(self, sorted_dca_scores, seqbackmapper):
        """The ranked list on the reference sequence's positions, as PlmDCA.get_mapped_site_pairs_dca_scores."""
        mapped, _mapping = _ranking.mapped_site_pairs(sorted_dca_scores, seqbackmapper)
        logger.info('\n\tSite pairs mapped onto the reference sequence: {}'.format(len(mapped)))
        return mapped

    def _sorted_scores(self, wildtype, apc, seqbackmapper):
        w = self._wildtype(wildtype)
        ctx = self._fitted_context()
        scores = ctx.ar_epistatic_scores(w[self.__order], apc=apc)
        if np.array_equal(self.__order, np.arange(self.__L)):
            ranked = _ranking.ranked(scores, self.__L, ctx.scores_order())
        else:                                          # another site order: relabel, then rank the relabelled vector
            ranked = _ranking.ranked(file_pair_scores(scores, self.__order), self.__L)
        return ranked if seqbackmapper is None else self.get_mapped_site_pairs_dca_scores(ranked, seqbackmapper)

    def compute_sorted_FN(self, wildtype=None, seqbackmapper=None):
        """Contact scores [((i, j), score), ...], best first: the Frobenius norm of the double-centred epistasis block of every
        site pair without its gap row and column (the scoring of PlmDCA.compute_sorted_FN applied to eps).  Sites in file
        order, or reference positions with seqbackmapper."""
        logger.info('\n\tarDCA epistatic scores (Frobenius norm), ranked')
        return self._sorted_scores(wildtype, False, seqbackmapper)

    def compute_sorted_FN_APC(self, wildtype=None, seqbackmapper=None):
        """compute_sorted_FN with the average product correction."""
        logger.info('\n\tarDCA epistatic scores with the average product correction, ranked')
        return self._sorted_scores(wildtype, True, seqbackmapper)
