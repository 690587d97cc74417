"""PlmDCA -- same class surface as pydca/plmdca/plmdca.py for the `plmdca compute_fn`
path.  The reference crosses into native code once (plmdca.py:202-243, ctypes call of
plmdcaBackend); here that call goes to libdca_hip.so and the O(L^2 q^2) Python loops that
follow it in the reference (gap stripping :246-268, Frobenius norm :437-481, APC :484-524)
run as device kernels as well."""
import logging
import time

import numpy as np

from .. import _compare, _lib, _potts, _ranking, multi_gpu, profile_alignment

logger = logging.getLogger(__name__)


class PlmDCAException(Exception):
    """Exceptions related to PlmDCA computation."""


def _ranked(scores, L, ctx=None):
    """[((i, j), score), ...] sorted by score, descending; ties keep (i, j) order, as Python's
    stable sorted(..., reverse=True) does in the reference (meanfield_dca.py:940, plmdca.py:479).
    With ctx the order comes from the device (stable radix sort of the score vector the context
    just produced, dca_scores_order); without it from numpy."""
    return _ranking.ranked(scores, L, ctx.scores_order() if ctx is not None else None)


def _boltzmann_options(iterations, num_chains, sweeps_per_iteration, equilibration_sweeps, learning_rate, lambda_h, lambda_J,
                       pseudocount, init):
    """Checks the arguments of PlmDCA.fit_boltzmann (host only) -> dict of the checked values."""
    def count(name, v, low):
        if isinstance(v, bool) or int(v) != v or int(v) < low:
            raise PlmDCAException('{} must be an integer >= {}, not {!r}'.format(name, low, v))
        return int(v)

    def rate(name, v):
        v = float(v)
        if not (0.0 <= v < float('inf')):
            raise PlmDCAException('{} must be finite and >= 0, not {!r}'.format(name, v))
        return v
    opts = dict(iterations=count('iterations', iterations, 1), num_chains=count('num_chains', num_chains, 1),
                sweeps_per_iteration=count('sweeps_per_iteration', sweeps_per_iteration, 1),
                equilibration_sweeps=count('equilibration_sweeps', equilibration_sweeps, 0),
                learning_rate=rate('learning_rate', learning_rate), lambda_h=rate('lambda_h', lambda_h),
                lambda_J=rate('lambda_J', lambda_J), pseudocount=None, init=init)
    if pseudocount is not None:
        opts['pseudocount'] = float(pseudocount)
        if not (0.0 <= opts['pseudocount'] < 1.0):
            raise PlmDCAException('pseudocount must lie in [0, 1), not {!r}'.format(pseudocount))
    if init not in ('plm', 'zero'):
        raise PlmDCAException("init must be 'plm' or 'zero', not {!r}".format(init))
    return opts


def _decimation_options(target_density, drop_fraction, pearson_target, iterations_per_check, max_iterations_per_round,
                        warmup_iterations, gauge, num_chains, sweeps_per_iteration, equilibration_sweeps, learning_rate, lambda_h,
                        lambda_J, pseudocount, init):
    """Checks the arguments of PlmDCA.decimate_boltzmann (host only) -> dict of the checked values."""
    opts = _boltzmann_options(1, num_chains, sweeps_per_iteration, equilibration_sweeps, learning_rate, lambda_h, lambda_J,
                              pseudocount, init)
    del opts['iterations']

    def real(name, v, ok, what):
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise PlmDCAException('{} must be a number, not {!r}'.format(name, v))
        if isinstance(v, bool) or not ok(v):
            raise PlmDCAException('{} must lie in {}, not {!r}'.format(name, what, v))
        return v

    def count(name, v, low):
        if isinstance(v, bool) or int(v) != v or int(v) < low:
            raise PlmDCAException('{} must be an integer >= {}, not {!r}'.format(name, low, v))
        return int(v)
    opts.update(target_density=real('target_density', target_density, lambda v: 0.0 <= v <= 1.0, '[0, 1]'),
                drop_fraction=real('drop_fraction', drop_fraction, lambda v: 0.0 < v <= 1.0, '(0, 1]'),
                pearson_target=real('pearson_target', pearson_target, lambda v: -1.0 <= v <= 1.0, '[-1, 1]'),
                iterations_per_check=count('iterations_per_check', iterations_per_check, 1),
                max_iterations_per_round=count('max_iterations_per_round', max_iterations_per_round, 1),
                warmup_iterations=count('warmup_iterations', warmup_iterations, 1))
    if gauge not in ('zero_sum', 'keep'):
        raise PlmDCAException("gauge must be 'zero_sum' or 'keep', not {!r}".format(gauge))
    opts['gauge'] = gauge
    return opts


class PlmDCA(_potts.PottsModel, _compare.SequenceComparison, profile_alignment.SequenceAlignment):
    """plmdca.py:25-104.  Extra keyword arguments (not in the reference): device,
    precision (32: float storage as the reference; 64: float64 checking mode) and
    exact_gradient (opt-in mathematically exact pseudolikelihood gradient instead of the
    reference's carried-over probabilities)."""

    def __init__(self, msa_file, biomolecule, seqid=None, lambda_h=None, lambda_J=None, max_iterations=None,
                 num_threads=None, verbose=False, device=0, precision=32, exact_gradient=False, devices=None):
        self.__biomolecule = biomolecule.strip().upper()
        if self.__biomolecule not in ('PROTEIN', 'RNA'):
            logger.error('\n\tBiomolecule {!r} is neither PROTEIN nor RNA'.format(self.__biomolecule))
            raise PlmDCAException
        self.__msa_file = msa_file
        self.__biomolecule_int = 1 if self.__biomolecule == 'PROTEIN' else 2
        self.__num_site_states = 21 if self.__biomolecule == 'PROTEIN' else 5
        self.__num_seqs, self.__seqs_len = self._get_num_and_len_of_seqs()
        self.__seqid = 0.8 if seqid is None else seqid
        if self.__seqid <= 0 or self.__seqid > 1.0:
            logger.error('\n\tseqid = {} lies outside (0, 1]'.format(self.__seqid))
            raise PlmDCAException
        self.__lambda_h = 0.2 * (self.__seqs_len - 1) if lambda_h is None else lambda_h
        if self.__lambda_h < 0:
            logger.error('\n\tlambda_h = {} is negative; the field penalty must be >= 0'.format(self.__lambda_h))
            raise PlmDCAException
        self.__lambda_J = 0.2 * (self.__seqs_len - 1) if lambda_J is None else lambda_J
        if self.__lambda_J < 0:
            logger.error('\n\tlambda_J = {} is negative; the coupling penalty must be >= 0'.format(self.__lambda_J))
            raise PlmDCAException
        self.__max_iterations = max_iterations if max_iterations is not None else 100
        self.__num_threads = 1 if num_threads is None else num_threads   # accepted, unused: the work runs on the GPU
        self.__verbose = True if verbose else False
        # devices=[0, 1, ...]: one rank per GPU (pydca_amd/multi_gpu.py) -- the counterpart of the reference's num_threads, its
        # one parallel knob (plmdca_main.py:77-78,131); a single entry is the same as device=
        try:
            self.__devices = multi_gpu.parse_devices(devices)
        except ValueError as exc:
            logger.error('\n\t{}'.format(exc))
            raise PlmDCAException(str(exc))
        self.__device = int(device) if not self.__devices else self.__devices[0]
        self.__precision = _lib.DCA_F64 if int(precision) == 64 else _lib.DCA_F32
        self.__carry = _lib.CARRY_EXACT if exact_gradient else _lib.CARRY_CHUNKED
        self.__data_size = int((self.__seqs_len * (self.__seqs_len - 1) * (self.__num_site_states ** 2)) / 2
                               + self.__seqs_len * self.__num_site_states)
        self.__ctx = None
        self.__compare_ctx = None          # alignment and weights only (_compare_context), when no fit has run
        self.__fields_and_couplings_all = None
        self.last_status = None
        logger.info('Created plmDCA instance: biomolecule {}, L {}, sequences {}, seqid {}, lambda_h {}, lambda_J {}, '
                    'iterations {}'.format(self.__biomolecule, self.__seqs_len, self.__num_seqs, self.__seqid,
                                           self.__lambda_h, self.__lambda_J, self.__max_iterations))

    # ---- properties (plmdca.py:107-160)
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
    def sequences_len(self):
        return self.__seqs_len

    @property
    def num_sequences(self):
        return self.__num_seqs

    @property
    def effective_num_sequences(self):
        raise NotImplementedError

    def _get_num_and_len_of_seqs(self):
        """Raw number of records and alignment length (plmdca.py:163-180)."""
        from ..fasta_reader import fasta_reader
        try:
            n, L = _lib.fasta_shape(self.__msa_file)           # one native pass over the file (ms for 10^5 sequences)
            if n > 0:
                return n, L
        except _lib.DcaBackendError as exc:
            if exc.code != _lib.DCA_ERR_RESIDUE:               # non-ASCII bytes: text mode below
                raise FileNotFoundError(self.__msa_file) if exc.code == _lib.DCA_ERR_IO else exc
        msa_data = fasta_reader.get_alignment_from_fasta_file(self.__msa_file)
        return len(msa_data), len(msa_data[0])

    def map_index_couplings(self, i, j, a, b):
        """plmdca.py:183-199."""
        q = self.__num_site_states
        L = self.__seqs_len
        site = int(((L * (L - 1) / 2) - (L - i) * ((L - i) - 1) / 2 + j - i - 1) * q * q)
        return L * q + site + b + a * q

    # ---- the native call
    def _run_backend(self):
        """Read + de-duplicate (C++ reader semantics), weights, initial parameters and L-BFGS
        on the device; leaves the optimised parameters resident in the context."""
        t0 = time.perf_counter()
        X, _raw = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__seqs_len)
        t1 = time.perf_counter()
        if self.__ctx is not None:
            self.__ctx.close()
            self.__ctx = None
        if self.__devices and len(self.__devices) > 1:
            try:
                _x, st, selection, ctx = multi_gpu.run_plm(X, self.__num_site_states, self.__seqid, self.__lambda_h, self.__lambda_J,
                                                           self.__max_iterations, self.__precision, self.__carry, self.__devices,
                                                           verbose=self.__verbose)
            except multi_gpu.MultiGpuError as exc:
                logger.error('\n\tA GPU rank failed: {}'.format(exc))
                if exc.kind == 'FileNotFoundError':
                    raise FileNotFoundError(exc.message)
                raise PlmDCAException(str(exc))
            t3 = time.perf_counter()
            self.last_status = dict(st, multi_gpu=selection, stages_s=dict(reader=t1 - t0, setup_and_optimise=t3 - t1))
            self.__ctx = ctx
            return ctx
        ctx = _lib.Context(self.__device, self.__precision)
        ctx.set_msa(X, self.__num_site_states)
        # the reference's C++ compares in float (plmdca_numerics.cpp:642); the float64 checking
        # mode compares in double like the float64 oracle
        ctx.compute_weights(self.__seqid, self.__precision)
        ctx.plm_configure(self.__lambda_h, self.__lambda_J, self.__carry)
        ctx.plm_init_x()
        t2 = time.perf_counter()
        ctx.plm_lbfgs_begin(self.__max_iterations, self.__verbose)
        st = ctx.plm_lbfgs_iterate(self.__max_iterations if self.__max_iterations else 1 << 30)
        t3 = time.perf_counter()
        self.last_status = dict(status=st.status, iterations=st.iterations, evaluations=st.evaluations, fx=st.fx,
                                seconds=st.seconds, unique_sequences=int(X.shape[0]),
                                stages_s=dict(reader=t1 - t0, setup=t2 - t1, optimise=t3 - t2))
        self.__ctx = ctx
        return ctx

    def get_fields_and_couplings_from_backend(self):
        """plmdca.py:202-243 -> float32[L*q + L(L-1)/2*q*q] (one bulk copy instead of the
        reference's element-by-element Python loop)."""
        logger.info('\n\tOptimising fields and couplings (L-BFGS on the pseudolikelihood, device resident)')
        ctx = self._run_backend()
        fields_and_couplings = ctx.plm_get_x(np.float32)
        assert fields_and_couplings.size == self.__data_size
        return fields_and_couplings

    def get_couplings_no_gap_state(self, fields_and_couplings_all):
        """plmdca.py:246-268, vectorised: the a,b < q-1 sub-block of every pair."""
        L, q = self.__seqs_len, self.__num_site_states
        J = np.asarray(fields_and_couplings_all)[L * q:].reshape(L * (L - 1) // 2, q, q)
        return np.ascontiguousarray(J[:, :q - 1, :q - 1]).reshape(-1)

    def get_fields_no_gap_state(self, fields_and_couplings_all):
        """plmdca.py:271-292."""
        L, q = self.__seqs_len, self.__num_site_states
        h = np.asarray(fields_and_couplings_all)[:L * q].reshape(L, q)
        return list(h[:, :q - 1].reshape(-1))

    def get_fields_and_couplings_no_gap_state(self, fields_and_couplings_all):
        return (self.get_fields_no_gap_state(fields_and_couplings_all),
                self.get_couplings_no_gap_state(fields_and_couplings_all))

    def shift_couplings(self, couplings_ij):
        """plmdca.py:320-342 (zero-sum gauge of one block)."""
        qm1 = self.__num_site_states - 1
        couplings_ij = np.reshape(couplings_ij, (qm1, qm1))
        avx = np.reshape(np.mean(couplings_ij, axis=1), (qm1, 1))
        avy = np.reshape(np.mean(couplings_ij, axis=0), (1, qm1))
        return couplings_ij - avx - avy + np.mean(couplings_ij)

    # ---- scores
    def get_mapped_site_pairs_dca_scores(self, sorted_dca_scores, seqbackmapper):
        """Keeps the site pairs whose two MSA columns map to the reference sequence and renames
        them to reference positions (meanfield_dca.py:755-790, plmdca.py:527-562)."""
        sorted_scores_mapped, self.__refseq_mapping_dict = _ranking.mapped_site_pairs(sorted_dca_scores, seqbackmapper)
        logger.info('\n\tSite pairs mapped onto the reference sequence: {}'.format(len(sorted_scores_mapped)))
        return sorted_scores_mapped

    def _maybe_mapped(self, ranked, seqbackmapper):
        return ranked if seqbackmapper is None else self.get_mapped_site_pairs_dca_scores(ranked, seqbackmapper)

    def compute_sorted_FN(self, seqbackmapper=None):
        """plmdca.py:437-481."""
        ctx = self._run_backend()
        self.__fields_and_couplings_all = None
        logger.info('\n\tFrobenius-norm scores without the average product correction, ranked')
        return self._maybe_mapped(_ranked(ctx.plm_scores(False), self.__seqs_len, ctx), seqbackmapper)

    def compute_sorted_FN_APC(self, seqbackmapper=None):
        """plmdca.py:484-524."""
        ctx = self._run_backend()
        logger.info('\n\tAverage product correction of the Frobenius-norm scores')
        t0 = time.perf_counter()
        ranked = _ranked(ctx.plm_scores(True), self.__seqs_len, ctx)
        self.last_status['stages_s']['scores_and_ranking'] = time.perf_counter() - t0
        return self._maybe_mapped(ranked, seqbackmapper)

    def compute_params(self, seqbackmapper=None, ranked_by=None, linear_dist=None, num_site_pairs=None):
        """plmdca.py:345-434: fields of every site (gap state dropped) and the gauge-shifted couplings
        of the top site pairs of a ranking, float32 like the reference's backend array.  Unlike the
        reference the optimisation is run once here, not once per scoring call."""
        if ranked_by is None:
            ranked_by = 'fn_apc'
        if linear_dist is None:
            linear_dist = 4
        RANKING_METHODS = ('FN', 'FN_APC', 'DI', 'DI_APC')
        ranked_by = ranked_by.strip().upper()
        if ranked_by not in RANKING_METHODS:
            logger.error('\n\tUnknown ranking {!r}; available: {}'.format(ranked_by, RANKING_METHODS))
            raise PlmDCAException
        ctx = self._run_backend()
        L, q = self.__seqs_len, self.__num_site_states
        if ranked_by in ('FN', 'FN_APC'):
            scores = ctx.plm_scores(ranked_by == 'FN_APC')
        else:
            scores = ctx.plm_di_scores(self.get_reg_single_site_freqs(), ranked_by == 'DI_APC')
        dca_scores = self._maybe_mapped(_ranked(scores, L, ctx), seqbackmapper)
        self.__fields_and_couplings_all = ctx.plm_get_x(np.float32)
        f = self.__fields_and_couplings_all[:L * q].reshape(L, q)[:, :q - 1]
        if seqbackmapper is not None:
            # refseq position -> MSA column (the scores above are in refseq positions)
            mapping_dict = {value: key for key, value in self.__refseq_mapping_dict.items()}
        else:
            mapping_dict = {i: i for i in range(L)}
        if num_site_pairs is None:
            num_site_pairs = len(seqbackmapper.ref_sequence) if seqbackmapper is not None else len(mapping_dict.keys())
        logger.info('\n\tExtracting fields')
        fields_mapped = [(i, f[mapping_dict[i]]) for i in mapping_dict.keys()]
        logger.info('\n\tCouplings of the best {} site pairs with |i - j| > {} in the {} ranking'.format(
            num_site_pairs, linear_dist, ranked_by))
        pairs, names = [], []
        count_pairs = 0
        for pair, _score in dca_scores:
            if abs(pair[0] - pair[1]) > linear_dist:
                count_pairs += 1
                if count_pairs > num_site_pairs:
                    break
                i, j = mapping_dict[pair[0]], mapping_dict[pair[1]]
                if i > j:
                    logger.error('\n\tSite pair out of order: i < j is required')
                    raise PlmDCAException
                pairs.append((i, j))
                names.append(pair)
        if count_pairs < num_site_pairs:
            logger.warning('\n\tOnly {} ranked site pairs satisfy the distance filter; their couplings are returned.'.format(count_pairs))
        blocks = ctx.plm_pair_couplings(pairs, shift=True).astype(np.float32)
        couplings_ranked = [(pair, blocks[k].reshape(-1)) for k, pair in enumerate(names)]
        return tuple(fields_mapped), tuple(couplings_ranked)

    # ---- the fitted model as a sequence model (no reference counterpart)
    def _fitted_context(self):
        """The model this instance holds from an earlier compute_* call; fitted once here if there is none."""
        return self.__ctx if self.__ctx is not None else self._run_backend()

    _potts_exc = PlmDCAException
    _potts_table = 0
    _potts_logger = logger

    def _potts_dims(self):
        return self.__biomolecule_int, self.__seqs_len, self.__num_site_states

    def _potts_default_source(self):
        return self.__msa_file

    def _potts_devices(self):
        return self.__devices

    def _potts_training(self):
        ctx = self._fitted_context()
        X = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__seqs_len)[0]
        return X, ctx.weights(), ctx.meff()

    def _potts_call(self, name, *args, **kw):
        return getattr(self._fitted_context(), 'plm_' + name)(*args, **kw)

    # ---- sequence sets against the alignment (_compare.SequenceComparison): alignment and weights only, no fit
    _compare_exc = PlmDCAException
    _compare_table = 0
    _compare_logger = logger
    _compare_dims = _potts_dims
    _compare_devices = _potts_devices

    def _compare_order(self):
        return None

    def _compare_context(self):
        """The fitted context if there is one (its alignment and weights are what the comparison needs); otherwise a context
        of its own with the de-duplicated alignment and its weights, kept for later calls -- no optimisation is run."""
        if self.__ctx is not None:
            return self.__ctx
        if self.__compare_ctx is None:
            X, _raw = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__seqs_len)
            ctx = _lib.Context(self.__device, self.__precision)
            ctx.set_msa(X, self.__num_site_states)
            ctx.compute_weights(self.__seqid, self.__precision)
            self.__compare_ctx = ctx
        return self.__compare_ctx

    def _unfitted_context(self):
        """Alignment, weights and configuration as _run_backend sets them up, without the L-BFGS run."""
        X, _raw = _lib.read_msa(self.__msa_file, self.__biomolecule_int, self.__seqs_len)
        ctx = _lib.Context(self.__device, self.__precision)
        ctx.set_msa(X, self.__num_site_states)
        ctx.compute_weights(self.__seqid, self.__precision)
        ctx.plm_configure(self.__lambda_h, self.__lambda_J, self.__carry)
        return ctx

    def fit_boltzmann(self, iterations=500, num_chains=1000, sweeps_per_iteration=10, equilibration_sweeps=100,
                      learning_rate=0.05, lambda_h=1e-4, lambda_J=1e-4, pseudocount=None, seed=0, init='plm'):
        """Refines the model by Boltzmann machine learning (bmDCA): gradient ascent on the
        L2-regularised log-likelihood, the model's one- and two-site frequencies estimated from num_chains persistent
        Gibbs chains on the GPU (sweeps_per_iteration sweeps per iteration after equilibration_sweeps at the start).
        learning_rate is the step of fields and couplings, lambda_h / lambda_J their L2 weights; pseudocount
        regularises the data frequencies (None: 1 / Meff).  init='plm' starts from the model this instance holds (its
        pseudo-likelihood fit, fitted here if there is none; after an earlier fit_boltzmann, that refined model), 'zero'
        from all-zero parameters.  Afterwards compute_sequence_energies,
        compute_single_mutant_effects and sample_sequences use the refined model; compute_sorted_FN* / DI* and
        compute_params fit the pseudo-likelihood model again, as they always do.
        -> {'history': float64[iterations, 3] of (eps_h, eps_J, pearson), 'fields_and_couplings': x}"""
        if self.__devices and len(self.__devices) > 1:
            logger.error('\n\tBoltzmann learning runs on one GPU; devices={}'.format(self.__devices))
            raise PlmDCAException('fit_boltzmann runs on one GPU, not on devices {}'.format(self.__devices))
        opts = _boltzmann_options(iterations, num_chains, sweeps_per_iteration, equilibration_sweeps, learning_rate, lambda_h,
                                  lambda_J, pseudocount, init)
        if opts['init'] == 'plm':
            ctx = self._fitted_context()
        else:
            ctx = self.__ctx if self.__ctx is not None else self._unfitted_context()
        self.__ctx = ctx
        ctx.plm_lbfgs_end()                      # a pseudo-likelihood run stopped at its iteration cap stays open until now
        dt = np.float64 if self.__precision == _lib.DCA_F64 else np.float32
        if opts['init'] == 'zero':
            ctx.plm_set_x(np.zeros(ctx.num_params(), dtype=dt))
        lam = 1.0 / ctx.meff() if opts['pseudocount'] is None else opts['pseudocount']
        logger.info('\n\tBoltzmann learning: {} iterations, {} chains, {} sweeps per iteration, {} equilibration sweeps'.format(
            opts['iterations'], opts['num_chains'], opts['sweeps_per_iteration'], opts['equilibration_sweeps']))
        ctx.plm_bm_begin(opts['num_chains'], opts['sweeps_per_iteration'], opts['equilibration_sweeps'], seed=int(seed),
                         eta_h=opts['learning_rate'], eta_J=opts['learning_rate'], mu_h=opts['lambda_h'], mu_J=opts['lambda_J'],
                         pseudocount=lam)
        try:
            history = ctx.plm_bm_iterate(opts['iterations'])
        finally:
            ctx.plm_bm_end()
        if history.shape[0]:
            logger.info('\n\tLast iteration: eps_h {:.3g}, eps_J {:.3g}, pearson {:.4f}'.format(*history[-1]))
        return {'history': history, 'fields_and_couplings': ctx.plm_get_x(dt)}

    def decimate_boltzmann(self, target_density=0.02, drop_fraction=0.01, pearson_target=0.95, iterations_per_check=10,
                           max_iterations_per_round=500, warmup_iterations=500, gauge='zero_sum', num_chains=1000,
                           sweeps_per_iteration=10, equilibration_sweeps=100, learning_rate=0.05, lambda_h=1e-4, lambda_J=1e-4,
                           pseudocount=None, seed=0, init='plm'):
        """Sparse Boltzmann machine learning (Barrat-Charlaix, Muntoni, Weigt 2021): learns as
        fit_boltzmann does until the model's connected correlations reach pearson_target against the data's (checked every
        iterations_per_check iterations, at most warmup_iterations the first time and max_iterations_per_round later), then
        removes the fraction drop_fraction of the still-active coupling elements whose removal changes the model least
        (symmetrised Kullback-Leibler divergence), learns again, and repeats down to round(target_density * pairs * q^2) active
        elements; one more convergence round ends it.  gauge='zero_sum' moves the starting model to the zero-sum gauge
        first, in which a zero coupling means no interaction; 'keep' leaves it as it is.  The other arguments are
        fit_boltzmann's.  The instance holds the sparse model afterwards.
        -> {'history': float64[iterations, 3], 'rounds': float64[decimations, 6] of (iteration index, active before, removed,
        density after, threshold, pearson before), 'mask': bool[pairs, q, q], 'density', 'fields_and_couplings': x}"""
        if self.__devices and len(self.__devices) > 1:
            logger.error('\n\tBoltzmann learning runs on one GPU; devices={}'.format(self.__devices))
            raise PlmDCAException('decimate_boltzmann runs on one GPU, not on devices {}'.format(self.__devices))
        opts = _decimation_options(target_density, drop_fraction, pearson_target, iterations_per_check, max_iterations_per_round,
                                   warmup_iterations, gauge, num_chains, sweeps_per_iteration, equilibration_sweeps, learning_rate,
                                   lambda_h, lambda_J, pseudocount, init)
        if opts['init'] == 'plm':
            ctx = self._fitted_context()
        else:
            ctx = self.__ctx if self.__ctx is not None else self._unfitted_context()
        self.__ctx = ctx
        ctx.plm_lbfgs_end()
        dt = np.float64 if self.__precision == _lib.DCA_F64 else np.float32
        if opts['init'] == 'zero':
            ctx.plm_set_x(np.zeros(ctx.num_params(), dtype=dt))
        if opts['gauge'] == 'zero_sum':
            ctx.plm_zero_sum_gauge()
        lam = 1.0 / ctx.meff() if opts['pseudocount'] is None else opts['pseudocount']
        L, q = self.__seqs_len, self.__num_site_states
        total = L * (L - 1) // 2 * q * q
        target = max(int(round(opts['target_density'] * total)), 0)
        ctx.plm_bm_begin(opts['num_chains'], opts['sweeps_per_iteration'], opts['equilibration_sweeps'], seed=int(seed),
                         eta_h=opts['learning_rate'], eta_J=opts['learning_rate'], mu_h=opts['lambda_h'], mu_J=opts['lambda_J'],
                         pseudocount=lam)
        history, rounds = [], []
        done = [0]

        def converge(cap):
            ran = 0
            while ran < cap:
                block = ctx.plm_bm_iterate(min(opts['iterations_per_check'], cap - ran))
                history.append(block)
                ran += block.shape[0]
                done[0] += block.shape[0]
                if block[-1, 2] >= opts['pearson_target']:
                    break
            return float(history[-1][-1, 2])
        try:
            pearson = converge(opts['warmup_iterations'])
            active = total
            while active > target:
                remove = min(int(np.ceil(opts['drop_fraction'] * active)), active - target)
                info = ctx.plm_bm_decimate(remove)
                active = info['active_after']
                rounds.append((done[0], info['active_before'], info['removed'], active / float(total), info['threshold'], pearson))
                pearson = converge(opts['max_iterations_per_round'])
                logger.info('\n\tDecimation {}: {} active elements (density {:.4g}) after {} iterations, pearson {:.4f}'.format(
                    len(rounds), active, active / float(total), done[0], pearson))
            if rounds:
                logger.info('\n\t{} decimations to density {:.4g}, pearson {:.4f}'.format(len(rounds), active / float(total), pearson))
            mask = ctx.plm_bm_get_mask().astype(bool)
        finally:
            ctx.plm_bm_end()
        return {'history': np.concatenate(history), 'rounds': np.array(rounds, dtype=np.float64).reshape(-1, 6), 'mask': mask,
                'density': active / float(total) if total else 0.0, 'fields_and_couplings': ctx.plm_get_x(dt)}

    def compute_seqs_weight(self):
        """plmdca.py:565-591: weights of the PYTHON reader's alignment (float64 comparison,
        plmdca/msa_numerics.py:13-49), computed on the device; remembered with their sum like the
        reference remembers them."""
        from ..fasta_reader import fasta_reader
        from . import msa_numerics
        logger.info('\n\tSequence weights at identity threshold {}'.format(self.__seqid))
        aln = np.array(fasta_reader.get_alignment_int_form(self.__msa_file, biomolecule=self.__biomolecule))
        seqs_weight = msa_numerics.compute_sequences_weight(alignment_data=aln, sequence_identity=self.__seqid)
        self.__seqs_weight = seqs_weight
        self.__eff_num_seqs = np.sum(seqs_weight)
        logger.info('\n\tMeff (sum of the sequence weights): {}'.format(self.__eff_num_seqs))
        return seqs_weight

    def compute_two_site_model_fields(self, couplings):
        """plmdca.py:652-680: couplings is the gap-stripped 1-D array of get_couplings_no_gap_state;
        -> float64[L(L-1)/2, 2, q], one workgroup per site pair on the device."""
        from . import msa_numerics
        reg_fi = self.get_reg_single_site_freqs()
        logger.info('\n\tFitting the two-site model fields of every site pair')
        return msa_numerics.compute_two_site_model_fields(couplings=couplings, reg_fi=reg_fi, seqs_len=self.__seqs_len,
                                                          num_site_states=self.__num_site_states)

    def get_single_site_freqs(self):
        """plmdca.py:590-621: frequencies of the PYTHON reader's alignment (unknown letters -> gap,
        duplicates dropped, fasta_reader.py:122-163) with float64 weights, on the device."""
        from ..fasta_reader import fasta_reader
        aln = np.array(fasta_reader.get_alignment_int_form(self.__msa_file, biomolecule=self.__biomolecule))
        ctx = _lib.Context(self.__device, _lib.DCA_F64)
        try:
            ctx.set_msa((aln - 1).astype(np.uint8), self.__num_site_states)
            ctx.compute_weights(self.__seqid, _lib.DCA_F64)
            return ctx.mf_single_site_freqs()
        finally:
            ctx.close()

    def get_reg_single_site_freqs(self):
        """plmdca.py:624-648 (pseudocount fixed at 0.5 as in the reference)."""
        from ..meanfield_dca import msa_numerics
        return msa_numerics.get_reg_single_site_freqs(
            single_site_freqs=self.get_single_site_freqs(), seqs_len=self.__seqs_len,
            num_site_states=self.__num_site_states, pseudocount=0.5)

    def compute_direct_info_unsorted_DI(self, apc=False):
        """plmdca.py:683-720: DI in pair order from the optimised parameters left on the device."""
        ctx = self._run_backend()
        reg_fi = self.get_reg_single_site_freqs()
        logger.info('\n\tDirect information (DI) of every site pair, on the device')
        return ctx.plm_di_scores(reg_fi, apc)

    def compute_sorted_DI(self, seqbackmapper=None):
        """plmdca.py:723-750."""
        return self._maybe_mapped(_ranked(self.compute_direct_info_unsorted_DI(False), self.__seqs_len, self.__ctx), seqbackmapper)

    def compute_sorted_DI_APC(self, seqbackmapper=None):
        """plmdca.py:753-790."""
        logger.info('\n\tAverage product correction of the DI scores')
        return self._maybe_mapped(_ranked(self.compute_direct_info_unsorted_DI(True), self.__seqs_len, self.__ctx), seqbackmapper)
