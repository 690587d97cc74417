// C entry points over pydca_amd/csrc/pca_host.h for tests/test_pca_host.py (built with a host compiler, no HIP).
#include "pca_host.h"

extern "C" {

// M: n x n row-major, symmetric (symmetrised as the fit does); evals descending, eigenvector j in column j of U
int pca_driver_eigh(int n, const double* M, double* U, double* evals) { return pca_sym_eigh(n, M, U, evals); }

long pca_driver_fix_sign(long len, double* v) { return (long)pca_fix_sign((size_t)len, v); }

int pca_driver_is_null(double lambda, double lambda1, double tol) { return pca_is_null(lambda, lambda1, tol) ? 1 : 0; }

int pca_driver_orth_transform(int b, const double* G, double* T) { return pca_orth_transform(b, G, T); }

int pca_driver_max_block(void) { return kPcaMaxBlock; }

}
