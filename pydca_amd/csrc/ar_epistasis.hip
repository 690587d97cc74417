// Double-mutant epistasis of the autoregressive model (dca_ar_epistasis, dca_ar_epistatic_scores), float64, model order.
//   eps_kl(a, b) = log P(w^{k->a, l->b}) - log P(w^{k->a}) - log P(w^{l->b}) + log P(w),  k < l, all q states
//   d_k(a)       = log P(w^{k->a}) - log P(w)
// for the wild type w, without forming one mutant sequence.  With cond_m the wild type's conditionals (ardca.hip's logits
// kernel, n = 1), p_m(c) = exp cond_m(c) and, for k < m,
//   U^k_m(a, c) = exp(J_km(a, c) - J_km(w_k, c)),  S_m(k, a) = sum_c p_m(c) U^k_m(a, c),  V^k_m(a, c) = sqrt(p_m(c)) U^k_m(a, c) / S_m(k, a)
// the sites before l cancel, the chosen-state logits after l cancel, and what is left is
//   d_k(a)       = (cond_k(a) - cond_k(w_k)) + sum_{m>k} [(J_km(a, w_m) - J_km(w_k, w_m)) - log S_m(k, a)]
//   eps_kl(a, b) = T - log prod_{m>l} r_m,   r_m = sum_c V^k_m(a, c) V^l_m(b, c)           [= S_m(k,a;l,b) / (S_m(k,a) S_m(l,b))]
//   T            = (J_kl(a, b) - J_kl(w_k, b)) - (J_kl(a, w_l) - J_kl(w_k, w_l))              [the site-l term: its normalisers cancel]
// DESIGN.md section 18 has the derivation.  Launches, all under the tag "ar_epistasis":
//   epi_prob_kernel    p_m(c) and sqrt(p_m(c)) = exp(cond_m(c) / 2)
//   epi_pairs_kernel   one workgroup per pair (k, m): U, S (ascending c), V into an m-major table (site m's rows (k, a), k < m, are
//                      contiguous: V[q^2 m (m - 1) / 2 + (k q + a) q + c]) and site m's term of d_k(a)
//   epi_single_kernel  d_k(a): those terms summed over ascending m
//   epi_main_kernel    for every later site m the product (k, a) x (l, b) over c is a tile of V_m V_m^T in the flattened index
//                      R = k q + a (p_m enters as sqrt(p_m) on both sides, so one table serves rows and columns and a tile's
//                      operands are two contiguous runs of it).  A workgroup owns 128 rows x 64 columns, streams m = l_min + 1 ..
//                      L - 1 through double-buffered LDS, keeps the running product of r_m of its 4 x 4 elements per thread in
//                      registers (a column joins once m > l), adds T and writes eps once.  Tiles go out heavy (low l) first.
// Order of every sum, fixed by (L, q): c ascending within S and r (fused multiply-adds, written as such), m ascending in the
// product.  Instead of one logarithm per (pair, state pair, m) the kernel multiplies the r_m and splits the exponent of the
// running product off into an integer every 4th step (so 4 consecutive r_m may span 2^+-1000 together before anything
// overflows); one logarithm at the end: eps = T - (log(mantissa product) + exponent sum * ln 2).  No atomics, no scratch.
// The product kernel's geometry (tile constants, epistasis_tiles, epi_mstart / epi_steps, epi_npre, epi_lds_bytes) is
// ar_epistasis_plan.h, host code that tests/ar_epistasis_plan_driver.cpp prints for the element audit.
#include "ar_epistasis_plan.h"
#include "site_conditionals.h"

#include <algorithm>
#include <cmath>

namespace {

__host__ __device__ __forceinline__ size_t v_offset(int m, int qq) { return (size_t)m * (m - 1) / 2 * qq; }

__global__ void epi_prob_kernel(const double* __restrict__ cond, int n, double* __restrict__ pm, double* __restrict__ spm)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    pm[t] = exp(cond[t]);
    spm[t] = exp(0.5 * cond[t]);
}

// grid (L - 1, L - 1): blockIdx.x = k, blockIdx.y = m - 1; the pairs k < m work
__global__ __launch_bounds__(256)
void epi_pairs_kernel(const double* __restrict__ x, const uint8_t* __restrict__ w, const double* __restrict__ pm,
                      const double* __restrict__ spm, int L, int q, double* __restrict__ V, double* __restrict__ term)
{
    __shared__ double U[32 * 32];
    __shared__ double S[32];
    const int k = blockIdx.x, m = blockIdx.y + 1;
    if (k >= m) return;
    const int qq = q * q, tid = threadIdx.x;
    const double* Jb = x + (size_t)L * q + pair_index(L, k, m) * (size_t)qq;
    const int wk = w[k];
    for (int e = tid; e < qq; e += 256) {
        const int a = e / q, c = e - a * q;
        U[e] = exp(Jb[e] - Jb[wk * q + c]);
    }
    __syncthreads();
    if (tid < q) {
        double s = 0.0;
        for (int c = 0; c < q; ++c) s = fma(pm[(size_t)m * q + c], U[tid * q + c], s);
        S[tid] = s;
        const int wm = w[m];
        term[(v_offset(m, 1) + k) * q + tid] = (Jb[tid * q + wm] - Jb[wk * q + wm]) - log(s);
    }
    __syncthreads();
    double* Vb = V + v_offset(m, qq) + (size_t)k * qq;
    for (int e = tid; e < qq; e += 256) {
        const int a = e / q, c = e - a * q;
        Vb[e] = (U[e] / S[a]) * spm[(size_t)m * q + c];
    }
}

__global__ void epi_single_kernel(const double* __restrict__ cond, const double* __restrict__ term, const uint8_t* __restrict__ w, int L,
                                  int q, double* __restrict__ d)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= L * q) return;
    const int k = t / q, a = t - k * q, wk = w[k];
    double s = 0.0;
    for (int m = k + 1; m < L; ++m) s += term[(v_offset(m, 1) + k) * q + a];
    d[t] = a == wk ? 0.0 : (cond[t] - cond[k * q + wk]) + s;
}

// tiles[blockIdx.x] = (row tile, column tile).  LDS: two buffers of (128 + 64) rows of q doubles, each a plain copy of two
// runs of V_m (q odd -- 5, 21 -- is an odd stride: the 16 columns tc of a half wave fall on 16 different bank pairs; an even q
// is served with bank conflicts; the 4 row groups of a wave read broadcast addresses).
// eps: the pair blocks in pair order, element a * q + b.
template <int QM>
__global__ __launch_bounds__(kEpiThreads)
void epi_main_kernel(const double* __restrict__ x, const uint8_t* __restrict__ w, const double* __restrict__ V,
                     const EpiTile* __restrict__ tiles, int L, int q, double* __restrict__ eps)
{
    constexpr int NPRE = epi_npre(QM);
    extern __shared__ __attribute__((aligned(16))) unsigned char epi_smem[];
    double* buf = reinterpret_cast<double*>(epi_smem);
    const int QP = q;
    const int bufVals = (kEpiTileR + kEpiTileC) * q;
    const int nA = kEpiTileR * q;
    const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
    const EpiTile tile = tiles[blockIdx.x];
    const int R0 = tile.x * kEpiTileR, C0 = tile.y * kEpiTileC;
    const int Lq = L * q, qq = q * q;
    const int mstart = epi_mstart(tile.y, q);
    const int steps = epi_steps(tile.y, L, q);

    int lcol[kEpiCols];                                  // site of column j; past the table: never joins
#pragma unroll
    for (int j = 0; j < kEpiCols; ++j) {
        const int C = C0 + tc + 16 * j;
        lcol[j] = C < Lq ? C / q : 0x7fffffff;
    }

    double pre[NPRE];
    auto load = [&](int m) {
        const double* Vm = V + v_offset(m, qq);
        const int lim = m * qq;                        // rows (k, a) with k < m exist
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + i * kEpiThreads;
            const int g = e < nA ? R0 * q + e : C0 * q + (e - nA);
            pre[i] = (e < bufVals && g < lim) ? Vm[g] : 0.0;
        }
    };
    auto store = [&](int t) {
        double* dst = buf + (t & 1) * bufVals;
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int e = tid + i * kEpiThreads;
            if (e < bufVals) dst[e] = pre[i];
        }
    };

    double prod[kEpiRows][kEpiCols];
    int esum[kEpiRows][kEpiCols];
#pragma unroll
    for (int i = 0; i < kEpiRows; ++i)
#pragma unroll
        for (int j = 0; j < kEpiCols; ++j) { prod[i][j] = 1.0; esum[i][j] = 0; }

    if (steps > 0) {
        load(mstart);
        store(0);
    }
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const int m = mstart + t;
        if (t + 1 < steps) load(m + 1);
        const double* A = buf + (t & 1) * bufVals + (tr * kEpiRows) * QP;
        const double* B = buf + (t & 1) * bufVals + (kEpiTileR + tc) * QP;
        double r[kEpiRows][kEpiCols];
#pragma unroll
        for (int i = 0; i < kEpiRows; ++i)
#pragma unroll
            for (int j = 0; j < kEpiCols; ++j) r[i][j] = 0.0;
#pragma unroll 1
        for (int c = 0; c < q; ++c) {
            double av[kEpiRows], bv[kEpiCols];
#pragma unroll
            for (int i = 0; i < kEpiRows; ++i) av[i] = A[i * QP + c];
#pragma unroll
            for (int j = 0; j < kEpiCols; ++j) bv[j] = B[16 * j * QP + c];
#pragma unroll
            for (int i = 0; i < kEpiRows; ++i)
#pragma unroll
                for (int j = 0; j < kEpiCols; ++j) r[i][j] = fma(av[i], bv[j], r[i][j]);
        }
#pragma unroll
        for (int j = 0; j < kEpiCols; ++j) {
            if (m > lcol[j]) {
#pragma unroll
                for (int i = 0; i < kEpiRows; ++i) prod[i][j] *= r[i][j];
            }
        }
        if ((t & (kEpiRescale - 1)) == kEpiRescale - 1) {
#pragma unroll
            for (int i = 0; i < kEpiRows; ++i)
#pragma unroll
                for (int j = 0; j < kEpiCols; ++j) {
                    const long long bits = __double_as_longlong(prod[i][j]);
                    esum[i][j] += (int)((bits >> 52) & 0x7ff) - 1023;
                    prod[i][j] = __longlong_as_double((bits & 0x800fffffffffffffLL) | 0x3ff0000000000000LL);
                }
        }
        if (t + 1 < steps) store(t + 1);
        __syncthreads();
    }

    const double* J = x + (size_t)Lq;
#pragma unroll
    for (int i = 0; i < kEpiRows; ++i) {
        const int R = R0 + tr * kEpiRows + i;
        if (R >= Lq) continue;
        const int k = R / q, a = R - k * q, wk = w[k];
#pragma unroll
        for (int j = 0; j < kEpiCols; ++j) {
            const int C = C0 + tc + 16 * j;
            if (C >= Lq) continue;
            const int l = lcol[j], b = C - l * q;
            if (k >= l) continue;
            const int wl = w[l];
            const size_t p = pair_index(L, k, l);
            const double* Jb = J + p * (size_t)qq;
            double v = 0.0;
            if (a != wk && b != wl) {
                const double T = (Jb[a * q + b] - Jb[wk * q + b]) - (Jb[a * q + wl] - Jb[wk * q + wl]);
                v = T - (log(prod[i][j]) + (double)esum[i][j] * 0.69314718055994530942);
            }
            eps[p * (size_t)qq + a * q + b] = v;
        }
    }
}

template <int QM>
hipError_t launch_main(dca_ctx* ctx, const double* x, const uint8_t* w, const double* V, const EpiTile* tiles, int ntiles,
                       int L, int q, double* eps)
{
    auto kern = epi_main_kernel<QM>;
    const size_t lds = epi_lds_bytes(q);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(ntiles), dim3(kEpiThreads), lds, ctx->stream, x, w, V, tiles, L, q, eps);
    return hipGetLastError();
}

struct EpiBuffers {
    DevBuf<uint8_t> dW;
    DevBuf<double> dCond, dPm, dSpm, dTerm, dV, dD, dVec;
    DevBuf<EpiTile> dTiles;
};

// B.dVec <- L q zeros, then eps in pair order (the plm layout scoring.hip reads); B.dD <- d.  Everything stays on the device.
int epistasis_device(dca_ctx* ctx, const double* dx, int L, int q, const uint8_t* wildtype, EpiBuffers& B)
{
    const size_t Lq = (size_t)L * q, pairs = (size_t)L * (L - 1) / 2, qq = (size_t)q * q;
    const std::vector<EpiTile> tiles = epistasis_tiles(L, q);
    if (B.dW.alloc((size_t)L, false) != hipSuccess || B.dCond.alloc(Lq, false) != hipSuccess || B.dPm.alloc(Lq, false) != hipSuccess ||
        B.dSpm.alloc(Lq, false) != hipSuccess || B.dD.alloc(Lq, false) != hipSuccess || B.dTerm.alloc(pairs * q, false) != hipSuccess ||
        B.dV.alloc(pairs * qq, false) != hipSuccess || B.dVec.alloc(Lq + pairs * qq, false) != hipSuccess ||
        B.dTiles.alloc(tiles.size(), false) != hipSuccess) {
        (void)hipGetLastError();
        dca_set_error("arDCA epistasis: out of device memory (%.0f MB for L = %d, q = %d)", (2.0 * pairs * qq + pairs * q) * 8e-6, L, q);
        return DCA_ERR_NOMEM;
    }
    DCA_TRY(dca_ar_engine_conditionals(ctx->ar, wildtype, B.dCond));
    HIP_TRY(hipMemcpyAsync(B.dW, wildtype, (size_t)L, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(B.dTiles, tiles.data(), tiles.size() * sizeof(EpiTile), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(B.dVec, 0, Lq * sizeof(double), ctx->stream));
    static const char* who = "arDCA epistasis";
    {
        ScopedKernelClock kc(ctx, "ar_epistasis");
        const unsigned lqBlocks = (unsigned)((Lq + 255) / 256);
        hipLaunchKernelGGL(epi_prob_kernel, dim3(lqBlocks), dim3(256), 0, ctx->stream, B.dCond.get(), (int)Lq, B.dPm.get(), B.dSpm.get());
        hipLaunchKernelGGL(epi_pairs_kernel, dim3(L - 1, L - 1), dim3(256), 0, ctx->stream, dx, B.dW.get(), B.dPm.get(), B.dSpm.get(), L, q,
                           B.dV.get(), B.dTerm.get());
        hipLaunchKernelGGL(epi_single_kernel, dim3(lqBlocks), dim3(256), 0, ctx->stream, B.dCond.get(), B.dTerm.get(), B.dW.get(), L, q,
                           B.dD.get());
        HIP_TRY_AS(hipGetLastError(), who);
        HIP_TRY_AS(with_qm(q, [&](auto qm) {
            return launch_main<decltype(qm)::value>(ctx, dx, B.dW, B.dV, B.dTiles, (int)tiles.size(), L, q, B.dVec + Lq);
        }), who);
    }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);     // the host copies of the wild type and the tiles are read until here
    return DCA_OK;
}

// the checks both entries share; on DCA_OK *dx, *L, *q describe the model
int epistasis_arguments(dca_ctx* ctx, const char* who, const uint8_t* wildtype, bool outputs, const double** dx, int* L, int* q)
{
    if (!ctx) { dca_set_error("null context"); return DCA_ERR_ARG; }
    if (!wildtype) { dca_set_error("%s: the wild type is NULL", who); return DCA_ERR_ARG; }
    if (!outputs) { dca_set_error("%s: no output requested", who); return DCA_ERR_ARG; }
    if (!dca_ar_engine_model(ctx->ar, dx, L, q)) { dca_set_error("dca_ar_configure first"); return DCA_ERR_STATE; }
    if (*L < 2) { dca_set_error("%s: the model has fewer than two sites", who); return DCA_ERR_ARG; }
    for (int k = 0; k < *L; ++k)
        if (wildtype[k] >= *q) { dca_set_error("%s: wild-type code %d >= q at site %d", who, (int)wildtype[k], k); return DCA_ERR_ARG; }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { dca_set_error("hipSetDevice: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
    return DCA_OK;
}

}  // namespace

// ---- C-ABI (include/dca_hip.h)
extern "C" {

int dca_ar_epistasis(dca_ctx* ctx, const uint8_t* wildtype, double* eps_out, double* single_out)
{
    const double* dx = nullptr;
    int L = 0, q = 0;
    DCA_TRY(epistasis_arguments(ctx, "dca_ar_epistasis", wildtype, eps_out || single_out, &dx, &L, &q));
    EpiBuffers B;
    DCA_TRY(epistasis_device(ctx, dx, L, q, wildtype, B));
    const size_t Lq = (size_t)L * q, n = (size_t)L * (L - 1) / 2 * q * q;
    if (eps_out) HIP_TRY(hipMemcpy(eps_out, B.dVec + Lq, n * sizeof(double), hipMemcpyDeviceToHost));
    if (single_out) HIP_TRY(hipMemcpy(single_out, B.dD, Lq * sizeof(double), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_ar_epistatic_scores(dca_ctx* ctx, const uint8_t* wildtype, int apc, double* scores_out)
{
    const double* dx = nullptr;
    int L = 0, q = 0;
    DCA_TRY(epistasis_arguments(ctx, "dca_ar_epistatic_scores", wildtype, scores_out != nullptr, &dx, &L, &q));
    EpiBuffers B;
    DCA_TRY(epistasis_device(ctx, dx, L, q, wildtype, B));
    const size_t npairs = (size_t)L * (L - 1) / 2;
    return dca_download_doubles(ctx, npairs, scores_out, "copy scores",
                                [&](double* dScores) { return dca_fn_scores(ctx, B.dVec, 0, DCA_F64, L, q, 0, apc, dScores); },
                                "dca_ar_epistatic_scores");
}

}  // extern "C"
