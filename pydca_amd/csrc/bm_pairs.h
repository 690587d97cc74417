// The Boltzmann-learning run and its pair kernel, shared by boltzmann.hip (statistics and update) and decimation.hip (the
// score mode): one workgroup per TB x TB tile of site pairs counts the chains' codes into an LDS histogram of uint32
// (ds_add_u32, exact) and then, per mode, writes g_ij, updates the couplings, or scores them from the histogram in LDS.
#pragma once
#include "dca_internal.h"

#include <cmath>

struct BmRun {
    int L = 0, q = 0, dtype = DCA_F32;
    int k = 1, E = 0;
    uint64_t seed = 0;
    double eta_h = 0, eta_J = 0, mu_h = 0, mu_J = 0;
    long long t = 0;                       // iterations since begin
    DcaChains ch;
    DevBuf<double> dFi, dFij, dGi, dEps, dSlab, dRec;
    int tb = 0, nb = 0, tiles = 0, recCap = 0;
    DevBuf<uint8_t> dMask;                 // pairs * q^2 bytes, 1 = active; absent until a mask is set or an element is removed
    long long active = 0;                  // active coupling elements (pairs * q^2 without a mask)
};

namespace {

// kBmThreads, kBmSums (slab: max |d|, sum Cd, sum Cm, sum Cd^2, sum Cm^2, sum Cd Cm) and bm_tile: potts_plan.h

enum { kBmCount = 0, kBmUpdate = 1, kBmScore = 2 };

// theta' = theta + eta * ((f - g) - mu * theta), every step in double, rounded once to S
template <typename S>
__device__ __forceinline__ void bm_update(S* p, double d, double eta, double mu)
{
    const double th = (double)*p;
    const double r = mu * th;
    const double s = d - r;
    *p = (S)(th + eta * s);
}

// The symmetrised Kullback-Leibler divergence between the model and the model with one coupling element J set to zero,
// p the element's frequency (include/dca_hip.h, dca_plm_bm_decimate): the operation order below, in double.  >= +0.
__host__ __device__ __forceinline__ double bm_decimation_score(double J, double p)
{
    if (p == 0.0 || p == 1.0 || J == 0.0) return 0.0;
    double D;
    if (J > 0.0) {
        const double e = expm1(-J);
        D = ((J * (-e)) * (p * (1.0 - p))) / (1.0 + p * e);
    } else {
        const double e = expm1(J);
        D = ((J * e) * (p * (1.0 - p))) / (1.0 + (1.0 - p) * e);
    }
    return D == 0.0 ? 0.0 : D;             // -0 becomes +0
}

// grid (nb, nb), nb = ceil(L / TB); the tiles (I, J) with I <= J hold the pairs i in block I, j in block J, i < j.
// kBmUpdate: couplings updated (a removed element, mask[off] == 0, is written +0; mask may be NULL) and slab[tile] written
// (tile = I nb - I (I - 1) / 2 + J - I); kBmCount: out = g_ij (pair order); kBmScore: out = the decimation score of every
// element from g_ij and x (-1 at a removed element), x untouched.
template <typename S, int TB, int MODE>
__global__ __launch_bounds__(kBmThreads)
void bm_pairs_kernel(const uint8_t* __restrict__ st, int nS, int n, int L, int q, int nb, const double* __restrict__ fi,
                     const double* __restrict__ fij, const double* __restrict__ gi, S* __restrict__ x, double eta, double mu,
                     double* __restrict__ slab, double* __restrict__ out, const uint8_t* __restrict__ mask)
{
    constexpr bool UPDATE = MODE == kBmUpdate;
    extern __shared__ __attribute__((aligned(16))) unsigned char bm_smem[];
    uint32_t* hist = reinterpret_cast<uint32_t*>(bm_smem);              // [TB * TB][q * q]
    __shared__ double red[kBmSums][kBmThreads];
    static_assert(sizeof(red) == kBmStaticLds, "potts_plan.h holds the static LDS of this kernel");
    const int I = blockIdx.y, J = blockIdx.x;
    if (J < I) return;
    const int t = threadIdx.x, qq = q * q, i0 = I * TB, j0 = J * TB;
    const int cells = TB * TB * qq;
    for (int e = t; e < cells; e += kBmThreads) hist[e] = 0u;
    __syncthreads();
    for (int c = t; c < n; c += kBmThreads) {
        int a[TB], b[TB];
#pragma unroll
        for (int u = 0; u < TB; ++u) {
            a[u] = i0 + u < L ? st[(size_t)(i0 + u) * nS + c] : 0;
            b[u] = j0 + u < L ? st[(size_t)(j0 + u) * nS + c] : 0;
        }
#pragma unroll
        for (int ii = 0; ii < TB; ++ii)
#pragma unroll
            for (int jj = 0; jj < TB; ++jj)
                if (i0 + ii < j0 + jj && j0 + jj < L) atomicAdd(&hist[(ii * TB + jj) * qq + a[ii] * q + b[jj]], 1u);
    }
    __syncthreads();
    double mx = 0.0, sd = 0.0, sm = 0.0, sdd = 0.0, smm = 0.0, sdm = 0.0;
    const size_t Lq = (size_t)L * q;
    for (int e = t; e < cells; e += kBmThreads) {
        const int p = e / qq, ab = e - p * qq;
        const int i = i0 + p / TB, j = j0 + p % TB;
        if (i >= j || j >= L) continue;
        const double g = (double)hist[e] / (double)n;
        const size_t off = pair_index(L, i, j) * qq + ab;
        if (MODE == kBmCount) { out[off] = g; continue; }
        if (MODE == kBmScore) {
            out[off] = mask && !mask[off] ? -1.0 : bm_decimation_score((double)x[Lq + off], g);
            continue;
        }
        const int a = ab / q, b = ab - a * q;
        const double f = fij[off];
        const double d = f - g;
        if (mask && !mask[off]) x[Lq + off] = (S)0;
        else bm_update(x + Lq + off, d, eta, mu);
        mx = fmax(mx, fabs(d));
        const double cd = f - fi[(size_t)i * q + a] * fi[(size_t)j * q + b];
        const double cm = g - gi[(size_t)i * q + a] * gi[(size_t)j * q + b];
        sd += cd; sm += cm; sdd += cd * cd; smm += cm * cm; sdm += cd * cm;
    }
    if (!UPDATE) return;
    red[0][t] = mx; red[1][t] = sd; red[2][t] = sm; red[3][t] = sdd; red[4][t] = smm; red[5][t] = sdm;
    __syncthreads();
    for (int s = kBmThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = fmax(red[0][t], red[0][t + s]);
#pragma unroll
            for (int k = 1; k < kBmSums; ++k) red[k][t] += red[k][t + s];
        }
        __syncthreads();
    }
    if (t < kBmSums) slab[((size_t)I * nb - (size_t)I * (I - 1) / 2 + (J - I)) * kBmSums + t] = red[t][0];
}

template <typename S, int TB, int MODE>
hipError_t launch_pairs_tb(dca_ctx* ctx, const BmRun* r, const DcaChains& ch, S* x, double* gi, double* out)
{
    auto kern = bm_pairs_kernel<S, TB, MODE>;
    const size_t lds = bm_lds(TB, r->q);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(r->nb, r->nb), dim3(kBmThreads), lds, ctx->stream, ch.dState.get(), ch.nS, ch.n, r->L, r->q, r->nb,
                       r->dFi.get(), r->dFij.get(), gi, x, r->eta_J, r->mu_J, r->dSlab.get(), out, r->dMask.get());
    return hipGetLastError();
}

// out: g_ij (kBmCount) or the scores (kBmScore); unused under kBmUpdate
template <typename S, int MODE>
hipError_t launch_pairs(dca_ctx* ctx, const BmRun* r, const DcaChains& ch, S* x, double* gi, double* out)
{
    switch (r->tb) {
    case 16: return launch_pairs_tb<S, 16, MODE>(ctx, r, ch, x, gi, out);
    case 4: return launch_pairs_tb<S, 4, MODE>(ctx, r, ch, x, gi, out);
    default: return launch_pairs_tb<S, 2, MODE>(ctx, r, ch, x, gi, out);
    }
}

}  // namespace
