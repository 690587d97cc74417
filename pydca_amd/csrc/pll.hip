// Site conditionals and pseudo-log-likelihoods of fixed query sequences under a fitted Potts model (E as in energy.hip):
//   u_i(a) = h_i(a) + sum_{j != i} J_ij(a, s_j)          (J read from the pair block (min(i,j), max(i,j)), as energy.hip reads it)
//   cond[i][a] = log-softmax of u_i,  site[i] = cond[i][s_i],  PLL(s) = sum_i site[i] (ascending i).
// The model arrives as a PottsSource (potts_source.h); the site kernel's loads are specialised per source kind (KIND).
//
// The kernel body, its geometry and the summation order (h_i first, then j ascending) are site_conditionals.h's; here are the
// policy that reads a Potts source, with each block staged transposed when j < i, T[b][a] = J_ij(a, b), and the host side of
// every site kernel (ardca.hip's too): the finish kernel, the pass size and the pass loop.  Queries go through in passes so that
// device scratch stays bounded whatever n is.
#include "site_conditionals.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

constexpr size_t kPPassBudget = 256ull << 20;      // device scratch of one pass

// site i of a Potts source: all j != i; the stored block of the pair (min(i,j), max(i,j)) holds J_ij(hi, lo) for j > i and
// J_ij(lo, hi) for j < i
template <typename S, int KIND, int QM>
struct PllPolicy {
    const S* src;
    const double* mfh;
    int L, q, ld, i;
    __device__ __forceinline__ int neighbours() const { return L; }
    __device__ __forceinline__ bool skip(int j) const { return j == i; }
    __device__ __forceinline__ S load(int j, int hi, int lo) const
    {
        const int lo_site = min(i, j), hi_site = max(i, j);
        if constexpr (KIND == 0) {
            return src[(size_t)L * q + pair_index(L, lo_site, hi_site) * (size_t)(q * q) + (size_t)(hi * q + lo)];
        } else {
            const int qm = q - 1;
            return (hi == qm || lo == qm) ? (S)0 : src[(size_t)(lo_site * qm + hi) * ld + (size_t)hi_site * qm + lo];
        }
    }
    __device__ __forceinline__ int lds_pos(int j, int hi, int lo) const { return j > i ? lo * QM + hi : hi * QM + lo; }
    __device__ __forceinline__ double field(int a) const { return potts_field(src, mfh, KIND, q, i, a); }
    __device__ __forceinline__ void epilogue(int, const double*, double, double, int) const {}
};

// grid (L, ceil(nq / 512)); LDS site_lds<S, QM>(q); the arguments as site_conditional_body takes them
template <typename S, int KIND, int QM>
__global__ __launch_bounds__(kSiteThreads)
void pll_site_kernel(const PottsView<S> pv, const uint8_t* __restrict__ QT, int nq, int NqS, double* __restrict__ site,
                     double* __restrict__ cond)
{
    const PllPolicy<S, KIND, QM> P{pv.src, pv.mfh, pv.L, pv.q, pv.ld, (int)blockIdx.x};
    site_conditional_body<S, QM>(P, blockIdx.x, blockIdx.y * kSiteSeqBlock, pv.L, pv.q, QT, nq, NqS, site, cond);
}

__global__ __launch_bounds__(256)
void site_finish_kernel(const double* __restrict__ site, int L, int nq, int NqS, double* __restrict__ sum, double* __restrict__ rows)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nq) return;
    double s = 0.0;
    for (int i = 0; i < L; ++i) {
        const double v = site[(size_t)i * NqS + n];
        s += v;
        if (rows) rows[(size_t)n * L + i] = v;
    }
    sum[n] = s;
}

template <typename S, int KIND, int QM>
hipError_t launch_site(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond)
{
    auto kern = pll_site_kernel<S, KIND, QM>;
    const size_t lds = site_lds<S, QM>(pv.q);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(pv.L, ceil_div(nq, kSiteSeqBlock)), dim3(kSiteThreads), lds, ctx->stream, pv, dQT, nq, NqS, dSite, dCond);
    return hipGetLastError();
}

template <typename S>
hipError_t dispatch_site(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond)
{
    return with_qm(pv.q, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        if constexpr (sizeof(S) == 8) {                       // the mf source is double
            if (pv.kind == 1) return launch_site<S, 1, QM>(ctx, pv, dQT, nq, NqS, dSite, dCond);
        }
        return launch_site<S, 0, QM>(ctx, pv, dQT, nq, NqS, dSite, dCond);
    });
}

}  // namespace

int site_pass_size(int n, size_t perSeq, size_t budget, const char* env, int granule)
{
    size_t cap = std::max((size_t)kSiteSeqBlock, budget / perSeq / kSiteSeqBlock * kSiteSeqBlock);
    const char* v = getenv(env);
    if (v && atol(v) > 0) cap = std::min(cap, std::max((size_t)granule, (size_t)atol(v) / granule * granule));
    return (int)std::min(cap, round_up((size_t)std::max(n, 1), granule));
}

hipError_t dca_site_finish(dca_ctx* ctx, const double* dSite, int L, int nq, int NqS, double* dSum, double* dRows)
{
    hipLaunchKernelGGL(site_finish_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, ctx->stream, dSite, L, nq, NqS, dSum, dRows);
    return hipGetLastError();
}

hipError_t dca_site_passes(dca_ctx* ctx, const SitePasses& sp, int L, int q, const uint8_t* X, int n, double* sum_out, double* site_out,
                           double* cond_out, const SiteLaunch& launch)
{
    const size_t perSeq = (size_t)L * (2 + sizeof(double)) + sizeof(double) + (site_out ? (size_t)L * sizeof(double) : 0) +
                          (cond_out ? (size_t)L * q * sizeof(double) : 0);
    const int cap = site_pass_size(n, perSeq, sp.budget, sp.env, sp.granule);
    const int NqS = (int)round_up((size_t)cap, kSiteSeqBlock);
    DevBuf<uint8_t> dRows, dQT;
    DevBuf<double> dSite, dSum, dSiteRows, dCond;
    HIP_PASS(dRows.alloc((size_t)cap * L, false));
    HIP_PASS(dQT.alloc((size_t)L * NqS, false));
    HIP_PASS(dSite.alloc((size_t)L * NqS, false));
    HIP_PASS(dSum.alloc((size_t)NqS, false));
    if (site_out) HIP_PASS(dSiteRows.alloc((size_t)cap * L, false));
    if (cond_out) HIP_PASS(dCond.alloc((size_t)cap * L * q, false));
    for (int first = 0; first < n; first += cap) {
        const int nq = std::min(cap, n - first);
        HIP_PASS(hipMemcpyAsync(dRows, X + (size_t)first * L, (size_t)nq * L, hipMemcpyHostToDevice, ctx->stream));
        HIP_PASS(dca_rows_to_sites(ctx, dRows, (size_t)L, nq, L, NqS, dQT));
        {
            ScopedKernelClock kc(ctx, sp.tag);
            HIP_PASS(launch(dQT, nq, NqS, dSite, dCond));
            HIP_PASS(dca_site_finish(ctx, dSite, L, nq, NqS, dSum, dSiteRows));
        }
        HIP_PASS(hipMemcpyAsync(sum_out + first, dSum, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (site_out)
            HIP_PASS(hipMemcpyAsync(site_out + (size_t)first * L, dSiteRows, (size_t)nq * L * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (cond_out)
            HIP_PASS(hipMemcpyAsync(cond_out + (size_t)first * L * q, dCond, (size_t)nq * L * q * sizeof(double), hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_PASS(hipStreamSynchronize(ctx->stream));
    }
    return hipSuccess;
}

int dca_potts_pseudo_likelihood(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, double* pll_out, double* site_out,
                                double* cond_out)
{
    if (n < 0 || (n > 0 && (!X || !pll_out))) { dca_set_error("pseudo-likelihood: bad arguments"); return DCA_ERR_ARG; }
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(X, (size_t)n * ps.L, ps.q, ""));
    const SitePasses sp{kPPassBudget, "DCA_PLL_PASS", kSiteSeqBlock, "pll"};
    const hipError_t e = with_source_type(ps, [&](auto pv) {
        return dca_site_passes(ctx, sp, ps.L, ps.q, X, n, pll_out, site_out, cond_out, [&](const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond) {
            return dispatch_site(ctx, pv, dQT, nq, NqS, dSite, dCond);
        });
    });
    if (e != hipSuccess) { dca_set_error("pseudo-likelihood: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
    return DCA_OK;
}
