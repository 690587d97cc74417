// Site conditionals and pseudo-log-likelihoods of fixed query sequences under a fitted Potts model (E as in energy.hip):
//   u_i(a) = h_i(a) + sum_{j != i} J_ij(a, s_j)          (J read from the pair block (min(i,j), max(i,j)), as energy.hip reads it)
//   m_i = max_b u_i(b),  Z_i = sum_b exp(u_i(b) - m_i) (ascending b),  cond[i][a] = (u_i(a) - m_i) - log Z_i,
//   site[i] = cond[i][s_i],  PLL(s) = sum_i site[i] (ascending i).
// The model arrives as a PottsSource (potts_source.h); the site kernel's loads are specialised per source kind (KIND).
//
// Summation order (depends on (L, q, dtype) only): every term widened to double; u_i(a) = h_i(a) first, then j ascending, one
// accumulator per (sequence, site, state) held by one lane.  No cross-lane or cross-workgroup sums, no atomics.
//
// Geometry: grid (site i, block of kPSeqBlock = 512 queries); a workgroup of 4 waves, each lane owns kPPerLane = 2 queries
// (tid and tid + 256 of the block) and keeps QM double accumulators for each.  Row i of J (L blocks of q x q) streams through
// LDS in double-buffered chunks of CJ blocks, each block stored transposed, T[b][a] = J_ij(a, b) with rows padded to QM values,
// so that a lane reads J_ij(., s_j) as QM contiguous values (ds_read_b128); the chunk's query codes (CJ x 512 bytes of the
// site-major copy) travel with it.  The next chunk's loads are in flight in registers while the current one is summed.
// Per-site values go to a site-major buffer; a finish kernel adds them per sequence in ascending i.  Queries go through in
// passes so that device scratch stays bounded whatever n is.
#include "dca_internal.h"

#include <cmath>
#include <cstdlib>

namespace {

constexpr int kPThreads = 256;                     // 4 waves
constexpr int kPPerLane = 2;                       // queries per lane
constexpr int kPSeqBlock = kPThreads * kPPerLane;  // queries per workgroup: one staging of row i serves 512 queries
constexpr int kPMaxCJ = 16;                        // blocks per chunk at most (bounds the code chunk to 8 KiB)
constexpr size_t kPChunkBudget = 16 * 1024;        // LDS per J chunk buffer (two of them)
constexpr size_t kPPassBudget = 256ull << 20;      // device scratch of one pass

// Blocks per chunk: a J chunk buffer holds CJ blocks of up to QM x QM values within kPChunkBudget (at most kPMaxCJ)
template <typename S, int QM>
constexpr int chunk_blocks() { return (int)(kPChunkBudget / (QM * QM * sizeof(S))) < kPMaxCJ ? (int)(kPChunkBudget / (QM * QM * sizeof(S))) : kPMaxCJ; }

// grid (L, ceil(nq / 512)).  LDS: two J chunk buffers (CJ blocks of q x QM values of S each), then two code buffers (CJ x 512
// bytes each).  KPB: block elements per thread (q * q <= 256 * KPB).  QT: site-major codes, NqS a multiple of 512 and
// >= gridDim.y * 512 (codes past nq are 0).  site: L x NqS doubles (site-major); cond: nq x L x q doubles or NULL.
template <typename S, int KIND, int QM>
__global__ __launch_bounds__(kPThreads)
void pll_site_kernel(const PottsView<S> pvIn, const uint8_t* __restrict__ QT, int nq, int NqS, double* __restrict__ site,
                     double* __restrict__ cond)
{
    PottsView<S> pv = pvIn;
    pv.kind = KIND;                                           // a compile-time constant from here on
    const S* src = pv.src;
    const int L = pv.L, q = pv.q, ld = pv.ld;
    constexpr int CJ = chunk_blocks<S, QM>();
    constexpr int KPB = (QM * QM + kPThreads - 1) / kPThreads;
    constexpr int codeBytes = CJ * kPSeqBlock;
    constexpr int CPT = (codeBytes / 16 + kPThreads - 1) / kPThreads;   // 16-byte code pieces per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char pll_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* bufJ = reinterpret_cast<S*>(pll_smem);
    uint8_t* bufC = pll_smem + ((size_t)2 * bufVals * sizeof(S) + 15) / 16 * 16;
    const int tid = threadIdx.x;
    const int i = blockIdx.x;
    const int seq0 = blockIdx.y * kPSeqBlock;
    const int qq = q * q;
    const int steps = (L + CJ - 1) / CJ;

    // this thread's block elements k = tid + kk * 256 < q * q: (hi, lo) = (k / q, k % q) of the stored block of the pair
    // (min(i,j), max(i,j)), i.e. J_ij(hi, lo) for j > i and J_ij(lo, hi) for j < i; the reads run along lo, contiguous in the source
    int kHi[KPB], kLo[KPB];
#pragma unroll
    for (int kk = 0; kk < KPB; ++kk) {
        const int k = tid + kk * kPThreads;
        kHi[kk] = k < qq ? k / q : -1;
        kLo[kk] = k < qq ? k - (k / q) * q : 0;
    }

    for (int e = tid; e < 2 * bufVals; e += kPThreads) bufJ[e] = (S)0;     // the row padding stays zero

    S val[CJ][KPB];
    static_assert(CPT <= 2, "at most two code pieces per thread");
    uint4 cv0 = {}, cv1 = {};                                 // the chunk's codes (kept out of an array: no stack)
    // registers <- chunk t: blocks j0 .. j0 + CJ - 1 of row i and their codes
    auto load = [&](int t) {
        const int j0 = t * CJ;
#pragma unroll
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= L || j == i) continue;
            const int lo_site = min(i, j), hi_site = max(i, j);
#pragma unroll
            for (int kk = 0; kk < KPB; ++kk) {
                if (kHi[kk] < 0) continue;
                if constexpr (KIND == 0) {
                    val[jj][kk] = src[(size_t)L * q + pair_index(L, lo_site, hi_site) * (size_t)qq + (size_t)(kHi[kk] * q + kLo[kk])];
                } else {
                    const int qm = q - 1;
                    val[jj][kk] = (kHi[kk] == qm || kLo[kk] == qm)
                                      ? (S)0 : src[(size_t)(lo_site * qm + kHi[kk]) * ld + (size_t)hi_site * qm + kLo[kk]];
                }
            }
        }
        // 16-byte piece e: row e / 32, bytes (e % 32) * 16 ..
        if (tid / 32 < CJ && j0 + tid / 32 < L) cv0 = *reinterpret_cast<const uint4*>(QT + (size_t)(j0 + tid / 32) * NqS + seq0 + (tid & 31) * 16);
        if constexpr (CPT > 1) {
            const int e = tid + kPThreads;
            if (e / 32 < CJ && j0 + e / 32 < L) cv1 = *reinterpret_cast<const uint4*>(QT + (size_t)(j0 + e / 32) * NqS + seq0 + (e & 31) * 16);
        }
    };
    auto store = [&](int t) {
        const int j0 = t * CJ;
        S* bj = bufJ + (t & 1) * bufVals;
        uint8_t* bc = bufC + (t & 1) * codeBytes;
#pragma unroll
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= L || j == i) continue;
#pragma unroll
            for (int kk = 0; kk < KPB; ++kk) {
                if (kHi[kk] < 0) continue;
                const int a = j > i ? kHi[kk] : kLo[kk], b = j > i ? kLo[kk] : kHi[kk];
                bj[jj * blk + b * QM + a] = val[jj][kk];
            }
        }
        if (tid / 32 < CJ && j0 + tid / 32 < L) *reinterpret_cast<uint4*>(bc + (tid / 32) * kPSeqBlock + (tid & 31) * 16) = cv0;
        if constexpr (CPT > 1) {
            const int e = tid + kPThreads;
            if (e / 32 < CJ && j0 + e / 32 < L) *reinterpret_cast<uint4*>(bc + (e / 32) * kPSeqBlock + (e & 31) * 16) = cv1;
        }
    };

    double u[kPPerLane][QM];
#pragma unroll
    for (int a = 0; a < QM; ++a) {
        const double h = a < q ? pv.field(i, a) : 0.0;
#pragma unroll
        for (int p = 0; p < kPPerLane; ++p) u[p][a] = h;
    }

    __syncthreads();
    load(0);
    store(0);
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const int j0 = t * CJ;
        if (t + 1 < steps) load(t + 1);
        const S* cur = bufJ + (t & 1) * bufVals;
        const uint8_t* cc = bufC + (t & 1) * codeBytes;
#pragma unroll 1
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= L) break;
            if (j == i) continue;
#pragma unroll
            for (int p = 0; p < kPPerLane; ++p) {
                const S* row = cur + jj * blk + (int)cc[jj * kPSeqBlock + p * kPThreads + tid] * QM;
                if constexpr (sizeof(S) == 4) {
#pragma unroll
                    for (int a = 0; a < QM; a += 4) {
                        const float4 v = *reinterpret_cast<const float4*>(row + a);
                        u[p][a] += (double)v.x; u[p][a + 1] += (double)v.y; u[p][a + 2] += (double)v.z; u[p][a + 3] += (double)v.w;
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < QM; a += 2) {
                        const double2 v = *reinterpret_cast<const double2*>(row + a);
                        u[p][a] += v.x; u[p][a + 1] += v.y;
                    }
                }
            }
        }
        if (t + 1 < steps) store(t + 1);
        __syncthreads();
    }

#pragma unroll
    for (int p = 0; p < kPPerLane; ++p) {
        const int n = seq0 + p * kPThreads + tid;
        if (n >= nq) continue;
        const int si = QT[(size_t)i * NqS + n];
        double m = u[p][0];
#pragma unroll
        for (int a = 1; a < QM; ++a) if (a < q) m = fmax(m, u[p][a]);
        double Z = 0.0, us = u[p][0];
#pragma unroll
        for (int a = 0; a < QM; ++a) {
            if (a < q) Z += exp(u[p][a] - m);
            if (a == si) us = u[p][a];
        }
        const double lz = log(Z);
        site[(size_t)i * NqS + n] = (us - m) - lz;
        if (cond) {
            double* out = cond + ((size_t)n * L + i) * q;
#pragma unroll
            for (int a = 0; a < QM; ++a) if (a < q) out[a] = (u[p][a] - m) - lz;
        }
    }
}

// PLL(n) = sum_i site[i][n] (ascending i); rows (nq x L) or NULL: the per-site values in the host layout
__global__ __launch_bounds__(256)
void pll_finish_kernel(const double* __restrict__ site, int L, int nq, int NqS, double* __restrict__ pll, double* __restrict__ rows)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nq) return;
    double s = 0.0;
    for (int i = 0; i < L; ++i) {
        const double v = site[(size_t)i * NqS + n];
        s += v;
        if (rows) rows[(size_t)n * L + i] = v;
    }
    pll[n] = s;
}

template <typename S, int QM>
size_t pll_lds(int q)
{
    constexpr int CJ = chunk_blocks<S, QM>();
    return round_up(2 * (size_t)CJ * q * QM * sizeof(S), 16) + 2 * (size_t)CJ * kPSeqBlock;
}

template <typename S, int KIND, int QM>
hipError_t launch_site(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond)
{
    auto kern = pll_site_kernel<S, KIND, QM>;
    const size_t lds = pll_lds<S, QM>(pv.q);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(pv.L, ceil_div(nq, kPSeqBlock)), dim3(kPThreads), lds, ctx->stream, pv, dQT, nq, NqS, dSite, dCond);
    return hipGetLastError();
}

template <typename S>
hipError_t dispatch_site(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond)
{
    const int QM = pv.q <= 8 ? 8 : pv.q <= 24 ? 24 : 32;
    if constexpr (sizeof(S) == 8) {                           // the mf source is double
        if (pv.kind == 1) switch (QM) {
        case 8: return launch_site<S, 1, 8>(ctx, pv, dQT, nq, NqS, dSite, dCond);
        case 24: return launch_site<S, 1, 24>(ctx, pv, dQT, nq, NqS, dSite, dCond);
        default: return launch_site<S, 1, 32>(ctx, pv, dQT, nq, NqS, dSite, dCond);
        }
    }
    switch (QM) {
    case 8: return launch_site<S, 0, 8>(ctx, pv, dQT, nq, NqS, dSite, dCond);
    case 24: return launch_site<S, 0, 24>(ctx, pv, dQT, nq, NqS, dSite, dCond);
    default: return launch_site<S, 0, 32>(ctx, pv, dQT, nq, NqS, dSite, dCond);
    }
}

// queries per pass: device scratch of a pass within kPPassBudget (DCA_PLL_PASS, a positive count, overrides it), a multiple of
// the workgroup's 512
int pll_pass_size(int n, int L, int q, bool want_site, bool want_cond)
{
    const size_t perSeq = (size_t)L * (2 + sizeof(double)) + sizeof(double) + (want_site ? (size_t)L * sizeof(double) : 0) +
                          (want_cond ? (size_t)L * q * sizeof(double) : 0);
    size_t cap = kPPassBudget / perSeq;
    const char* env = getenv("DCA_PLL_PASS");
    if (env && atol(env) > 0) cap = (size_t)atol(env);
    cap = std::max((size_t)kPSeqBlock, cap / kPSeqBlock * kPSeqBlock);
    return (int)std::min(cap, round_up((size_t)n, kPSeqBlock));
}

template <typename S>
int pll_t(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* X, int n, double* pll_out, double* site_out, double* cond_out)
{
    const int L = pv.L, q = pv.q;
    const int cap = pll_pass_size(n, L, q, site_out != nullptr, cond_out != nullptr);
    const int NqS = cap;                                      // a multiple of 512
    uint8_t *dRows = nullptr, *dQT = nullptr;
    double *dSite = nullptr, *dPll = nullptr, *dSiteRows = nullptr, *dCond = nullptr;
    hipError_t e = dca_dev_malloc(reinterpret_cast<void**>(&dRows), (size_t)cap * L, false);
    if (e == hipSuccess) e = dca_dev_malloc(reinterpret_cast<void**>(&dQT), (size_t)L * NqS, false);
    if (e == hipSuccess) e = dca_dev_malloc(reinterpret_cast<void**>(&dSite), (size_t)L * NqS * sizeof(double), false);
    if (e == hipSuccess) e = dca_dev_malloc(reinterpret_cast<void**>(&dPll), (size_t)NqS * sizeof(double), false);
    if (e == hipSuccess && site_out) e = dca_dev_malloc(reinterpret_cast<void**>(&dSiteRows), (size_t)cap * L * sizeof(double), false);
    if (e == hipSuccess && cond_out) e = dca_dev_malloc(reinterpret_cast<void**>(&dCond), (size_t)cap * L * q * sizeof(double), false);
    for (int first = 0; first < n && e == hipSuccess; first += cap) {
        const int nq = std::min(cap, n - first);
        e = hipMemcpyAsync(dRows, X + (size_t)first * L, (size_t)nq * L, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) break;
        e = dca_rows_to_sites(ctx, dRows, nq, L, NqS, dQT);
        if (e != hipSuccess) break;
        {
            ScopedKernelClock kc(ctx, "pll");
            e = dispatch_site<S>(ctx, pv, dQT, nq, NqS, dSite, dCond);
            if (e == hipSuccess)
                hipLaunchKernelGGL(pll_finish_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, ctx->stream, dSite, L, nq, NqS, dPll, dSiteRows);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pll_out + first, dPll, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && site_out)
            e = hipMemcpyAsync(site_out + (size_t)first * L, dSiteRows, (size_t)nq * L * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && cond_out)
            e = hipMemcpyAsync(cond_out + (size_t)first * L * q, dCond, (size_t)nq * L * q * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    dca_dev_free(dRows); dca_dev_free(dQT); dca_dev_free(dSite); dca_dev_free(dPll); dca_dev_free(dSiteRows); dca_dev_free(dCond);
    if (e != hipSuccess) { dca_set_error("pseudo-likelihood: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
    return DCA_OK;
}

}  // namespace

int dca_potts_pseudo_likelihood(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, double* pll_out, double* site_out,
                                double* cond_out)
{
    if (n < 0 || (n > 0 && (!X || !pll_out))) { dca_set_error("pseudo-likelihood: bad arguments"); return DCA_ERR_ARG; }
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(X, (size_t)n * ps.L, ps.q, ""));
    return with_source_type(ps, [&](auto pv) { return pll_t(ctx, pv, X, n, pll_out, site_out, cond_out); });
}
