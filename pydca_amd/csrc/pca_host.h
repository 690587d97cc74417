// The small dense pieces of the principal-component fit (pca.hip): the eigen-decomposition of the b x b
// Rayleigh-Ritz and Gram matrices (b <= 72), the order of the eigenpairs, the sign and null rules of the contract and the
// transform that orthonormalises a block through its Gram matrix.  Host code only, double, no HIP header: a host compiler
// builds it, and tests/test_pca_host.py holds it against numpy.linalg.eigh.  Every loop runs in a fixed order, so the same
// matrix gives the same bits on every host.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

constexpr int kPcaMaxBlock = 72;        // b = min(L q, k + 8), k <= 64
constexpr int kPcaJacobiSweeps = 60;

// Cyclic Jacobi of the symmetric n x n row-major A (both triangles are read and kept equal; A is destroyed).  Sweeps visit the
// pairs (p, q), p < q, row by row; a pair is rotated unless |a_pq| <= 2^-54 ||A||_F / n (the norm of the input), so what is left
// off the diagonal is below 2^-54 ||A||_F in norm.  evals[j] = the diagonal, U (n x n row-major) holds eigenvector j in COLUMN j.
// Returns the number of sweeps that rotated.
inline int pca_jacobi_eigh(int n, double* A, double* U, double* evals)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) U[(size_t)i * n + j] = i == j ? 1.0 : 0.0;
    double fro = 0.0;
    for (int e = 0; e < n * n; ++e) fro += A[e] * A[e];
    fro = std::sqrt(fro);
    const double thr = 0x1.0p-54 * fro / (double)(n > 0 ? n : 1);
    int sweeps = 0;
    for (; sweeps < kPcaJacobiSweeps; ++sweeps) {
        bool rotated = false;
        for (int p = 0; p + 1 < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[(size_t)p * n + q];
                if (!(std::fabs(apq) > thr)) continue;
                rotated = true;
                const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {               // columns p and q
                    const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
                    A[(size_t)k * n + p] = c * akp - s * akq;
                    A[(size_t)k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {               // rows p and q
                    const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
                    A[(size_t)p * n + k] = c * apk - s * aqk;
                    A[(size_t)q * n + k] = s * apk + c * aqk;
                }
                A[(size_t)p * n + q] = 0.0;
                A[(size_t)q * n + p] = 0.0;
                for (int k = 0; k < n; ++k) {
                    const double ukp = U[(size_t)k * n + p], ukq = U[(size_t)k * n + q];
                    U[(size_t)k * n + p] = c * ukp - s * ukq;
                    U[(size_t)k * n + q] = s * ukp + c * ukq;
                }
            }
        if (!rotated) break;
    }
    for (int j = 0; j < n; ++j) evals[j] = A[(size_t)j * n + j];
    return sweeps;
}

// eigenpairs in descending order of the eigenvalue, equal values in ascending order of the column they came from
inline void pca_sort_descending(int n, double* evals, double* U)
{
    std::vector<int> ord(n);
    for (int j = 0; j < n; ++j) ord[j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return evals[x] > evals[y]; });
    std::vector<double> e(evals, evals + n), u(U, U + (size_t)n * n);
    for (int j = 0; j < n; ++j) {
        evals[j] = e[ord[j]];
        for (int i = 0; i < n; ++i) U[(size_t)i * n + j] = u[(size_t)i * n + ord[j]];
    }
}

// symmetrise (the mean of the two triangles), decompose, sort: evals descending, eigenvector j in column j of U
inline int pca_sym_eigh(int n, const double* M, double* U, double* evals)
{
    std::vector<double> A((size_t)n * n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = 0.5 * (M[(size_t)i * n + j] + M[(size_t)j * n + i]);
    const int sweeps = pca_jacobi_eigh(n, A.data(), U, evals);
    pca_sort_descending(n, evals, U);
    return sweeps;
}

// the sign rule: the entry of largest magnitude becomes positive, ties go to the smallest index.  Returns the index of that
// entry (0 for an all-zero vector, which stays as it is).
inline size_t pca_fix_sign(size_t len, double* v)
{
    size_t at = 0;
    double big = -1.0;
    for (size_t e = 0; e < len; ++e) {
        const double a = std::fabs(v[e]);
        if (a > big) { big = a; at = e; }
    }
    if (len && v[at] < 0.0)
        for (size_t e = 0; e < len; ++e) v[e] = -v[e];
    return at;
}

// the null rule: a component whose eigenvalue does not exceed tol * lambda_1 is returned as zeros
inline bool pca_is_null(double lambda, double lambda1, double tol) { return !(lambda > tol * lambda1); }

// The transform T (b x b row-major) that orthonormalises a block Z with the Gram matrix G = Z^T Z: with s_j = G_jj^-1/2 (0 for
// a zero column) and S G S = U D U^T, column j of T is S U_j D_j^-1/2, so (Z T)^T (Z T) = I on the directions kept.  A
// direction with D_j below b 2^-52 D_max is dropped: its column of T is zero, and so is that column of Z T.  (No Cholesky
// factor: it breaks down on the rank-deficient blocks that fewer than b sequences produce.)  Returns the directions kept.
inline int pca_orth_transform(int b, const double* G, double* T)
{
    std::vector<double> s(b), A((size_t)b * b), U((size_t)b * b), D(b);
    for (int j = 0; j < b; ++j) {
        const double g = G[(size_t)j * b + j];
        s[j] = g > 0.0 && std::isfinite(1.0 / std::sqrt(g)) ? 1.0 / std::sqrt(g) : 0.0;
    }
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < b; ++j) A[(size_t)i * b + j] = 0.5 * (G[(size_t)i * b + j] + G[(size_t)j * b + i]) * s[i] * s[j];
    pca_jacobi_eigh(b, A.data(), U.data(), D.data());
    pca_sort_descending(b, D.data(), U.data());
    const double floor_ = (double)b * 0x1.0p-52 * D[0];
    int kept = 0;
    for (int j = 0; j < b; ++j) {
        const bool keep = D[0] > 0.0 && D[j] >= floor_ && D[j] > 0.0;
        const double r = keep ? 1.0 / std::sqrt(D[j]) : 0.0;
        for (int i = 0; i < b; ++i) T[(size_t)i * b + j] = keep ? s[i] * U[(size_t)i * b + j] * r : 0.0;
        kept += keep ? 1 : 0;
    }
    return kept;
}
