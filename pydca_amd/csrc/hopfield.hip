// Hopfield-Potts DCA (Cocco, Monasson, Weigt 2013): the patterns are the eigenpairs at both ends of the
// spectrum of Gamma = R^-1 C R^-T, C the mean-field correlation matrix and D = R R^T its block diagonal, and the couplings are
// J = sum over the selected patterns of (1 - 1 / lambda) u u^T with u = R^-T v.
//   hp_factor_kernel     one workgroup per site: Cholesky factor R_i of the (q-1) x (q-1) diagonal block in LDS; R_i^-1 is what it writes.
//   hp_whiten_kernel     one workgroup per site pair i <= j: Gamma_ij = R_i^-1 C_ij R_j^-T in place, the block and both factors
//                        staged in LDS, the mirror block written from the same values (Gamma is bit-symmetric).
//   hp_apply_kernel      Y = A V for a dense symmetric A (n x n, leading dimension ld) and a block V of b <= 72 columns on the
//                        f64 matrix cores (v_mfma_f64_16x16x4_f64).  A workgroup owns 64 rows and one slab of 1024 columns; its
//                        four waves take the slab's 16-column steps in turn and keep 4 x ceil(b / 16) accumulator tiles each, so
//                        an element of A is read once and a fragment of V serves four row tiles.  The waves' sums are added in
//                        wave order through LDS, the slabs' in ascending order by hp_sum_kernel.
//   hp_assemble_kernel   J = sum_mu s_mu xi_mu xi_mu^T on the matrix cores, 64 x 64 tiles; s_mu = +-1 multiplies one operand, so
//                        (r, c) and (c, r) add the same products in the same order and J is bit-symmetric.
// No floating atomics; the order of every sum is fixed by (n, b), (n, p) or q alone.  The b x b algebra of the subspace iteration
// is pca.hip's (Gram, sum, rotate kernels; tag "pca_small") and pca_host.h's.
#include "dca_internal.h"
#include "hopfield_plan.h"
#include "pca_host.h"

#include <algorithm>
#include <cmath>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

constexpr int kLdsStride = kHpMaxStates + 1;

__global__ __launch_bounds__(64)
void hp_factor_kernel(const double* __restrict__ C, int qm, int ld, double* __restrict__ Rinv, int* __restrict__ info)
{
    __shared__ double a[kHpMaxStates * kLdsStride], x[kHpMaxStates * kLdsStride];
    __shared__ int bad;
    const int i = blockIdx.x, t = threadIdx.x;
    for (int e = t; e < qm * qm; e += 64) {
        const int r = e / qm, c = e - r * qm;
        a[r * kLdsStride + c] = C[(size_t)(i * qm + r) * ld + (size_t)i * qm + c];
        x[r * kLdsStride + c] = 0.0;
    }
    if (t == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < qm; ++k) {                  // left-looking: column k of R from the columns before it, ascending
        if (t == k) {
            double s = a[k * kLdsStride + k];
            for (int c = 0; c < k; ++c) s -= a[k * kLdsStride + c] * a[k * kLdsStride + c];
            if (!(s > 0.0)) bad = k + 1;
            a[k * kLdsStride + k] = sqrt(s);
        }
        __syncthreads();
        if (bad) break;
        if (t > k && t < qm) {
            double s = a[t * kLdsStride + k];
            for (int c = 0; c < k; ++c) s -= a[t * kLdsStride + c] * a[k * kLdsStride + c];
            a[t * kLdsStride + k] = s / a[k * kLdsStride + k];
        }
        __syncthreads();
    }
    if (t == 0) info[i] = bad;
    if (bad) return;
    if (t < qm) {                                   // column t of R^-1 by forward substitution
        x[t * kLdsStride + t] = 1.0 / a[t * kLdsStride + t];
        for (int r = t + 1; r < qm; ++r) {
            double s = 0.0;
            for (int d = t; d < r; ++d) s += a[r * kLdsStride + d] * x[d * kLdsStride + t];
            x[r * kLdsStride + t] = -s / a[r * kLdsStride + r];
        }
    }
    __syncthreads();
    for (int e = t; e < qm * qm; e += 64) {
        const int r = e / qm, c = e - r * qm;
        Rinv[(size_t)i * qm * qm + e] = x[r * kLdsStride + c];
    }
}

// grid (L, L); blocks below the diagonal return.  In place: a workgroup reads C_ij only and writes Gamma_ij and Gamma_ji.
__global__ __launch_bounds__(256)
void hp_whiten_kernel(double* __restrict__ C, int qm, int ld, const double* __restrict__ Rinv)
{
    __shared__ double ri[kHpMaxStates * kLdsStride], rj[kHpMaxStates * kLdsStride], c[kHpMaxStates * kLdsStride],
        tmp[kHpMaxStates * kLdsStride];
    const int i = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
    if (j < i) return;
    for (int e = t; e < qm * qm; e += 256) {
        const int r = e / qm, s = e - r * qm;
        ri[r * kLdsStride + s] = Rinv[(size_t)i * qm * qm + e];
        rj[r * kLdsStride + s] = Rinv[(size_t)j * qm * qm + e];
        c[r * kLdsStride + s] = C[(size_t)(i * qm + r) * ld + (size_t)j * qm + s];
    }
    __syncthreads();
    for (int e = t; e < qm * qm; e += 256) {        // tmp = R_i^-1 C_ij, ascending over the inner index
        const int a = e / qm, b = e - a * qm;
        double s = 0.0;
        for (int d = 0; d <= a; ++d) s += ri[a * kLdsStride + d] * c[d * kLdsStride + b];
        tmp[a * kLdsStride + b] = s;
    }
    __syncthreads();
    for (int e = t; e < qm * qm; e += 256) {        // Gamma_ij = tmp R_j^-T
        const int a = e / qm, b = e - a * qm;
        if (i == j && b > a) continue;              // a diagonal block: the lower triangle, mirrored
        double s = 0.0;
        for (int d = 0; d <= b; ++d) s += tmp[a * kLdsStride + d] * rj[b * kLdsStride + d];
        C[(size_t)(i * qm + a) * ld + (size_t)j * qm + b] = s;
        if (i != j || a != b) C[(size_t)(j * qm + b) * ld + (size_t)i * qm + a] = s;
    }
}

// grid (row groups, slabs), 256 threads.  out: the slab's n x b block of partial sums (Y itself with one slab).
template <int NT>
__global__ __launch_bounds__(256)
void hp_apply_kernel(const double* __restrict__ A, int n, int ld, const double* __restrict__ V, int b, double* __restrict__ out)
{
    constexpr int RT = kHpApplyRowTiles;
    __shared__ double red[RT * NT * 4 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int row0 = blockIdx.x * kHpApplyRows, slab = blockIdx.y;
    const int kBeg = slab * kHpApplySlab, kEnd = min(n, kBeg + kHpApplySlab);
    const bool vec = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;     // kc is a multiple of 4: 16-byte loads
    double4_t acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    for (int k0 = kBeg + wave * kHpTile; k0 < kEnd; k0 += kHpTile * kHpApplyWaves) {
        // lane (lr, lg) holds A[row lr of the tile][kc .. kc + 3]: matrix-core step j multiplies the columns kc + j of the
        // four lane groups, a permutation of the 16 columns of the step that V's fragment follows
        const int kc = k0 + 4 * lg;
        double a[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = row0 + rt * kHpTile + lr;
            const double* ap = A + (size_t)r * ld + kc;
            if (r < n && kc + 3 < kEnd) {
                if (vec) {
                    const double2_t lo = *reinterpret_cast<const double2_t*>(ap), hi = *reinterpret_cast<const double2_t*>(ap + 2);
                    a[rt][0] = lo[0]; a[rt][1] = lo[1]; a[rt][2] = hi[0]; a[rt][3] = hi[1];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[rt][j] = ap[j];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[rt][j] = (r < n && kc + j < kEnd) ? ap[j] : 0.0;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = kc + j;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int col = t * kHpTile + lr;
                const double bv = (kk < kEnd && col < b) ? V[(size_t)kk * b + col] : 0.0;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt][j], bv, acc[rt][t], 0, 0, 0);
            }
        }
    }
    // the four waves' sums, added in wave order
    for (int w = 0; w < kHpApplyWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const int at = ((rt * NT + t) * 4 + reg) * 64 + lane;
                        red[at] = w == 0 ? acc[rt][t][reg] : red[at] + acc[rt][t][reg];
                    }
        }
        __syncthreads();
    }
    // result (row i, column j) of a tile sits in register i / 4 of lane (i % 4) * 16 + j
    double* dst = out + (size_t)slab * n * b;
    const int rowsHere = min(kHpApplyRows, n - row0);
    for (int e = threadIdx.x; e < rowsHere * b; e += 256) {
        const int row = e / b, col = e - row * b;
        const int rt = row / kHpTile, i = row % kHpTile, t = col / kHpTile, j = col % kHpTile;
        dst[(size_t)(row0 + row) * b + col] = red[((rt * NT + t) * 4 + i / 4) * 64 + (i % 4) * 16 + j];
    }
}

__global__ __launch_bounds__(256)
void hp_sum_kernel(const double* __restrict__ part, int slabs, size_t len, double* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int s = 0; s < slabs; ++s) acc += part[(size_t)s * len + e];
    out[e] = acc;
}

// grid (ceil(n / 64), ceil(n / 64)), 256 threads: wave w forms rows 16 w .. 16 w + 15 of the tile.  Xi: n x P4 row-major, P4 a
// multiple of 4 (zero columns past p); sgn: P4 values +-1.
__global__ __launch_bounds__(256)
void hp_assemble_kernel(const double* __restrict__ Xi, const double* __restrict__ sgn, int n, int P4, double* __restrict__ J, int ld)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lg = lane >> 4;
    const int r0 = blockIdx.y * kHpAsmTile + wave * kHpTile, c0 = blockIdx.x * kHpAsmTile;
    double4_t acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int ra = r0 + lr;
    for (int k0 = 0; k0 < P4; k0 += 4) {
        const int k = k0 + lg;
        const double a = ra < n ? Xi[(size_t)ra * P4 + k] * sgn[k] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cb = c0 + t * kHpTile + lr;
            const double bv = cb < n ? Xi[(size_t)cb * P4 + k] : 0.0;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = r0 + lg + 4 * reg, j = c0 + t * kHpTile + lr;
            if (i < n && j < n) J[(size_t)i * ld + j] = acc[t][reg];
        }
}

int upload(dca_ctx* ctx, const char* who, void* dst, const void* src, size_t bytes)
{
    HIP_TRY_AS(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}
int download(dca_ctx* ctx, const char* who, void* dst, const void* src, size_t bytes)
{
    HIP_TRY_AS(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}

#define HP_ALLOC(buf, count) HIP_TRY_AS_NOMEM((buf).alloc(std::max<size_t>(count, 1), false), who)

template <int NT>
void launch_apply(dca_ctx* ctx, const HpApplyPlan& p, const double* dA, int n, int ld, const double* dV, int b, double* dOut)
{
    hipLaunchKernelGGL(hp_apply_kernel<NT>, dim3(p.row_groups, p.slabs), dim3(256), 0, ctx->stream, dA, n, ld, dV, b, dOut);
}

}  // namespace

int dca_hp_factor(dca_ctx* ctx, const double* dC, int L, int qm, int ld, double* dRinv)
{
    static const char* who = "dca_mf_hopfield_fit";
    if (qm < 1 || qm >= kHpMaxStates) { dca_set_error("%s: q - 1 = %d is outside 1 .. %d", who, qm, kHpMaxStates - 1); return DCA_ERR_ARG; }
    DevBuf<int> dInfo;
    HP_ALLOC(dInfo, (size_t)L);
    {
        ScopedKernelClock kc(ctx, "hopfield_whiten");
        hipLaunchKernelGGL(hp_factor_kernel, dim3(L), dim3(64), 0, ctx->stream, dC, qm, ld, dRinv, dInfo.get());
    }
    HIP_TRY_AS(hipGetLastError(), who);
    std::vector<int> info(L);
    DCA_TRY(download(ctx, who, info.data(), dInfo, (size_t)L * sizeof(int)));
    for (int i = 0; i < L; ++i)
        if (info[i] != 0) {
            dca_set_error("%s: the diagonal block of site %d is not positive definite (pivot %d): raise the pseudocount", who, i, info[i]);
            return DCA_ERR_NOT_SPD;
        }
    return DCA_OK;
}

int dca_hp_whiten(dca_ctx* ctx, double* dC, int L, int qm, int ld, const double* dRinv)
{
    ScopedKernelClock kc(ctx, "hopfield_whiten");
    hipLaunchKernelGGL(hp_whiten_kernel, dim3(L, L), dim3(256), 0, ctx->stream, dC, qm, ld, dRinv);
    HIP_TRY_AS(hipGetLastError(), "dca_mf_hopfield_fit");
    return DCA_OK;
}

// dY (n x b) = dA (n x n, leading dimension ld) dV (n x b); dPart: hp_apply_plan(n, b).part_doubles doubles (unused with one slab)
int dca_hp_apply(dca_ctx* ctx, const double* dA, int n, int ld, const double* dV, int b, double* dY, double* dPart)
{
    static const char* who = "dca_dense_apply";
    if (n < 1 || b < 1 || b > kPcaMaxBlock || ld < n) { dca_set_error("%s: n %d, b %d (1 .. %d) or ld %d", who, n, b, kPcaMaxBlock, ld); return DCA_ERR_ARG; }
    const HpApplyPlan p = hp_apply_plan(n, b);
    double* dOut = p.slabs > 1 ? dPart : dY;
    ScopedKernelClock kc(ctx, "hopfield_apply");
    switch (p.col_tiles) {
    case 1: launch_apply<1>(ctx, p, dA, n, ld, dV, b, dOut); break;
    case 2: launch_apply<2>(ctx, p, dA, n, ld, dV, b, dOut); break;
    case 3: launch_apply<3>(ctx, p, dA, n, ld, dV, b, dOut); break;
    case 4: launch_apply<4>(ctx, p, dA, n, ld, dV, b, dOut); break;
    default: launch_apply<5>(ctx, p, dA, n, ld, dV, b, dOut); break;
    }
    if (p.slabs > 1) {
        const size_t len = (size_t)n * b;
        hipLaunchKernelGGL(hp_sum_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, ctx->stream, dPart, p.slabs, len, dY);
    }
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}

// The k largest eigenpairs of the dense symmetric dA by block subspace iteration with Rayleigh-Ritz on b = hp_block(n, k)
// vectors: the loop of dca_pca_fit with the operator applied by dca_hp_apply.  theta_out (b) descending, res_out (b) the
// residuals ||A v - theta v|| of the Ritz vectors, dV (n x b, allocated here) the Ritz vectors in columns.
int dca_hp_eigs(dca_ctx* ctx, const double* dA, int n, int ld, int k, double tol, int max_iterations, uint64_t seed, double* theta_out,
                double* res_out, DevBuf<double>* dV, int* iterations_out, int* converged_out)
{
    static const char* who = "dca_mf_hopfield_fit";
    const int b = hp_block(n, k);
    const HpApplyPlan plan = hp_apply_plan(n, b);
    DevBuf<double> dY, dR, dPart, dGpart, dSmall, dT1, dT2;
    const size_t bb = (size_t)b * b;
    HP_ALLOC(*dV, (size_t)n * b);
    HP_ALLOC(dY, (size_t)n * b);
    HP_ALLOC(dR, (size_t)n * b);
    HP_ALLOC(dPart, plan.part_doubles);
    HP_ALLOC(dGpart, (size_t)dca_pca_small_chunks(n) * bb);
    HP_ALLOC(dSmall, bb);
    HP_ALLOC(dT1, bb);
    HP_ALLOC(dT2, bb);
    std::vector<double> theta(b, 0.0), res(b, 0.0), U(bb), H(bb), T(bb);
    auto orthonormalise = [&]() -> int {
        for (int pass = 0; pass < 2; ++pass) {
            DCA_TRY(dca_pca_small_gram(ctx, who, *dV, b, *dV, b, n, false, dGpart, dSmall));
            DCA_TRY(download(ctx, who, H.data(), dSmall, bb * sizeof(double)));
            pca_orth_transform(b, H.data(), T.data());
            DCA_TRY(upload(ctx, who, dT1, T.data(), bb * sizeof(double)));
            DCA_TRY(dca_pca_small_rotate(ctx, who, *dV, dT1, nullptr, nullptr, n, b, dR));
            dV->swap(dR);
        }
        return DCA_OK;
    };
    DCA_TRY(dca_pca_small_init(ctx, who, *dV, n, b, seed));
    DCA_TRY(orthonormalise());
    int it = 0, converged = 0;
    for (;;) {
        ++it;
        DCA_TRY(dca_hp_apply(ctx, dA, n, ld, *dV, b, dY, dPart));                                     // Y = A V
        DCA_TRY(dca_pca_small_gram(ctx, who, *dV, b, dY, b, n, false, dGpart, dSmall));               // H = V^T Y
        DCA_TRY(download(ctx, who, H.data(), dSmall, bb * sizeof(double)));
        pca_sym_eigh(b, H.data(), U.data(), theta.data());
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) T[(size_t)i * b + j] = -(U[(size_t)i * b + j] * theta[j]);
        DCA_TRY(upload(ctx, who, dT1, U.data(), bb * sizeof(double)));
        DCA_TRY(upload(ctx, who, dT2, T.data(), bb * sizeof(double)));
        DCA_TRY(dca_pca_small_rotate(ctx, who, dY, dT1, *dV, dT2, n, b, dR));                         // R = Y U - V U Theta
        DCA_TRY(dca_pca_small_gram(ctx, who, dR, b, dR, b, n, true, dGpart, dSmall));
        DCA_TRY(download(ctx, who, res.data(), dSmall, (size_t)b * sizeof(double)));
        converged = 1;
        for (int m = 0; m < b; ++m) {
            res[m] = std::sqrt(res[m]);
            if (m < k && !(res[m] <= tol * theta[0])) converged = 0;
        }
        if (converged || it >= max_iterations) {
            DCA_TRY(dca_pca_small_rotate(ctx, who, *dV, dT1, nullptr, nullptr, n, b, dR));            // the Ritz vectors V U
            dV->swap(dR);
            break;
        }
        DCA_TRY(dca_pca_small_rotate(ctx, who, dY, dT1, nullptr, nullptr, n, b, dR));                 // the next block: orth(Y U)
        dV->swap(dR);
        DCA_TRY(orthonormalise());
    }
    for (int m = 0; m < b; ++m) { theta_out[m] = theta[m]; res_out[m] = res[m]; }
    *iterations_out = it;
    *converged_out = converged;
    return DCA_OK;
}

// res_out[m] = ||A v_m - lambda_m v_m|| for the b columns of dV (n x b): one application, one rotation, one diagonal Gram
int dca_hp_residuals(dca_ctx* ctx, const double* dA, int n, int ld, const double* dV, int b, const double* lambda, double* res_out)
{
    static const char* who = "dca_mf_hopfield_fit";
    const HpApplyPlan plan = hp_apply_plan(n, b);
    const size_t bb = (size_t)b * b;
    DevBuf<double> dY, dR, dPart, dGpart, dSmall, dT1, dT2;
    HP_ALLOC(dY, (size_t)n * b);
    HP_ALLOC(dR, (size_t)n * b);
    HP_ALLOC(dPart, plan.part_doubles);
    HP_ALLOC(dGpart, (size_t)dca_pca_small_chunks(n) * bb);
    HP_ALLOC(dSmall, bb);
    HP_ALLOC(dT1, bb);
    HP_ALLOC(dT2, bb);
    std::vector<double> I(bb, 0.0), T(bb, 0.0);
    for (int j = 0; j < b; ++j) { I[(size_t)j * b + j] = 1.0; T[(size_t)j * b + j] = -lambda[j]; }
    DCA_TRY(upload(ctx, who, dT1, I.data(), bb * sizeof(double)));
    DCA_TRY(upload(ctx, who, dT2, T.data(), bb * sizeof(double)));
    DCA_TRY(dca_hp_apply(ctx, dA, n, ld, dV, b, dY, dPart));
    DCA_TRY(dca_pca_small_rotate(ctx, who, dY, dT1, dV, dT2, n, b, dR));
    DCA_TRY(dca_pca_small_gram(ctx, who, dR, b, dR, b, n, true, dGpart, dSmall));
    DCA_TRY(download(ctx, who, res_out, dSmall, (size_t)b * sizeof(double)));
    for (int m = 0; m < b; ++m) res_out[m] = std::sqrt(res_out[m]);
    return DCA_OK;
}

// dJ (n x n, leading dimension ld) = sum_mu sign_mu xi_mu xi_mu^T; xi: host, p x n
int dca_hp_assemble(dca_ctx* ctx, const double* xi, const int32_t* sign, int p, int n, double* dJ, int ld)
{
    static const char* who = "dca_mf_hopfield_fit";
    const int P4 = (int)round_up((size_t)std::max(p, 1), 4);
    std::vector<double> X((size_t)n * P4, 0.0), s(P4, 1.0);
    for (int m = 0; m < p; ++m) {
        s[m] = sign[m] < 0 ? -1.0 : 1.0;
        for (int r = 0; r < n; ++r) X[(size_t)r * P4 + m] = xi[(size_t)m * n + r];
    }
    DevBuf<double> dX, dS;
    HP_ALLOC(dX, X.size());
    HP_ALLOC(dS, s.size());
    DCA_TRY(upload(ctx, who, dX, X.data(), X.size() * sizeof(double)));
    DCA_TRY(upload(ctx, who, dS, s.data(), s.size() * sizeof(double)));
    const int tiles = ceil_div(n, kHpAsmTile);
    {
        ScopedKernelClock kc(ctx, "hopfield_assemble");
        hipLaunchKernelGGL(hp_assemble_kernel, dim3(tiles, tiles), dim3(256), 0, ctx->stream, dX.get(), dS.get(), n, P4, dJ, ld);
    }
    HIP_TRY_AS(hipGetLastError(), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);       // dX and dS go out of scope
    return DCA_OK;
}

// the test hook dca_dense_apply: host A (n rows at stride ld), V (n x b) -> Y (n x b)
int dca_dense_apply_impl(dca_ctx* ctx, const double* A, int n, int ld, const double* V, int b, double* Y)
{
    static const char* who = "dca_dense_apply";
    const HpApplyPlan plan = hp_apply_plan(n, b);
    DevBuf<double> dA, dV, dY, dPart;
    HP_ALLOC(dA, (size_t)n * ld);
    HP_ALLOC(dV, (size_t)n * b);
    HP_ALLOC(dY, (size_t)n * b);
    HP_ALLOC(dPart, plan.part_doubles);
    DCA_TRY(upload(ctx, who, dA, A, (size_t)n * ld * sizeof(double)));
    DCA_TRY(upload(ctx, who, dV, V, (size_t)n * b * sizeof(double)));
    DCA_TRY(dca_hp_apply(ctx, dA, n, ld, dV, b, dY, dPart));
    return download(ctx, who, Y, dY, (size_t)n * b * sizeof(double));
}
