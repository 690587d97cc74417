"""HopfieldPottsDCA -- the Hopfield-Potts model (Cocco, Monasson, Weigt, PLoS Comput Biol 2013): the
mean-field couplings restricted to the patterns of largest likelihood gain, the eigenvectors at both ends of the spectrum of the
Pearson correlation matrix.  The class is MeanFieldDCA with the fit swapped: everything that reads the fitted model (scores,
fields, parameters, energies, samplers, ascent, log Z) reads the Hopfield-Potts couplings the context holds after the fit."""
import logging

import numpy as np

from .. import _lib
from ..meanfield_dca.meanfield_dca import MeanFieldDCA, MeanFieldDCAException

logger = logging.getLogger(__name__)


class HopfieldPottsDCAException(MeanFieldDCAException):
    """Errors related to the Hopfield-Potts computation."""


class HopfieldPottsDCA(MeanFieldDCA):
    """Hopfield-Potts DCA.  num_patterns: the patterns of largest likelihood gain over the whole spectrum; or num_attractive and
    num_repulsive: that many of the largest and of the smallest eigenvalues (at most 64 of either end)."""

    def __init__(self, msa_file, biomolecule, pseudocount=None, seqid=None, num_patterns=None, num_attractive=None, num_repulsive=None,
                 tolerance=1e-10, max_iterations=1000, seed=0, device=0):
        super().__init__(msa_file, biomolecule, pseudocount=pseudocount, seqid=seqid, device=device)
        try:
            self.__selection = _lib.hopfield_arguments(num_patterns, num_attractive, num_repulsive, tolerance, max_iterations, seed,
                                                       self.sequences_len, self.num_site_states)
        except ValueError as exc:
            logger.error('\n\t{}'.format(exc))
            raise HopfieldPottsDCAException(str(exc))
        self.__fit = None
        self.__fit_pseudocount = None

    def __str__(self):
        return '<instance of HopfieldPottsDCA>'

    _potts_exc = HopfieldPottsDCAException
    _compare_exc = HopfieldPottsDCAException
    _potts_logger = logger
    _compare_logger = logger

    # ---- the fit
    def _fit_patterns(self):
        """The fit of the current pseudocount; run again when the pseudocount changed or the context holds another model."""
        ctx = self._compare_context()
        if (self.__fit is not None and self.__fit_pseudocount == self.pseudocount
                and ctx.mf_model_kind() == _lib.MF_MODEL_HOPFIELD):
            return self.__fit
        sel, p, a, r, tol, max_it, seed = self.__selection
        logger.info('\n\tHopfield-Potts patterns: whitening, both ends of the spectrum, selection, couplings')
        try:
            if sel == _lib.HOPFIELD_LIKELIHOOD:
                fit = ctx.mf_hopfield_fit(self.pseudocount, num_patterns=p, tol=tol, max_iterations=max_it, seed=seed)
            else:
                fit = ctx.mf_hopfield_fit(self.pseudocount, num_attractive=a, num_repulsive=r, tol=tol, max_iterations=max_it, seed=seed)
        except _lib.DcaBackendError as exc:
            if exc.code == _lib.DCA_ERR_NOT_SPD:
                logger.error('\n\tThe correlation matrix is not positive definite ({}): pseudocount {} is too small for this '
                             'alignment, raise it.'.format(exc, self.pseudocount))
                raise np.linalg.LinAlgError('Singular matrix')
            raise
        for end, name in ((0, 'attractive'), (1, 'repulsive')):
            if not fit['converged'][end]:
                logger.warning('\n\tThe {} end did not converge in {} iterations: largest residual {:.3e}'.format(
                    name, fit['iterations'][end], float(fit['residuals'].max())))
        self.__fit, self.__fit_pseudocount = fit, self.pseudocount
        return fit

    def compute_patterns(self):
        """-> dict: eigenvalues, gains, residuals float64[p], signs int32[p], patterns float64[p, L, q - 1], num_attractive,
        num_repulsive, iterations and converged per end (attractive, repulsive).  The attractive patterns come first, in
        descending order of the eigenvalue, then the repulsive ones in ascending order; the couplings are
        sum_mu signs[mu] patterns[mu] patterns[mu]^T off the diagonal blocks."""
        return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self._fit_patterns().items()}

    def project_on_patterns(self, sequences=None):
        """Overlaps x_mu(s) = sum_i patterns[mu, i, s_i] (a gap adds 0) -> float64[n, p].  sequences: None (every record of the
        training alignment), a FASTA path or a list of aligned strings."""
        fit = self._fit_patterns()
        X = self._query(sequences)
        return self._compare_context().hopfield_project(fit['patterns'], X)

    # ---- MeanFieldDCA's surface on the Hopfield-Potts couplings
    def _device_scores(self, apc):
        self._fit_patterns()
        return self._compare_context().mf_scores(apc)

    def get_couplings(self):
        """The Hopfield-Potts couplings as float64[L(q-1), L(q-1)]; the diagonal blocks are as the pattern sum gives them."""
        self._fit_patterns()
        return self._compare_context().mf_hopfield_couplings()

    def _with_couplings(self, call):
        self._fit_patterns()
        return call()
