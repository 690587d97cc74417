// Log-softmax site conditionals of query sequences, shared by pll.hip (Potts pseudo-likelihood) and ardca.hip (arDCA):
//   u(a) = h(a) + sum over the neighbour sites j of J_j(a, s_j),  m = max_b u(b),  Z = sum_b exp(u(b) - m) (ascending b),
//   cond[a] = (u(a) - m) - log Z,  site = cond[s_i];  per sequence, the site values are added in ascending site order.
// A policy says which neighbours a site has and where their blocks lie; everything else is here once.
//
// Summation order (depends on the shape and the policy only): every term widened to double, no contraction; u(a) = h(a)
// first, then the neighbours ascending, one accumulator per (sequence, site, state) held by one lane.  No cross-lane or
// cross-workgroup sums, no atomics: a sequence's outputs have the same bits in any batch, position, pass split or repeat.
//
// Geometry: a workgroup of 4 waves serves one site and a block of kSiteSeqBlock = 512 queries; each lane owns kSitePerLane = 2
// queries (tid and tid + 256 of the block) and keeps QM double accumulators for each (QM = qm_of(q)).  The site's neighbour
// blocks (q x q) stream through LDS in double-buffered chunks of CJ blocks, each staged so that row s_j holds J_j(., s_j) padded
// to QM values: a lane reads it as QM contiguous values (ds_read_b128).  The chunk's query codes (CJ x 512 bytes of the
// site-major copy) travel with it.  The next chunk's loads are in flight in registers while the current one is summed.
#pragma once
#include "potts_rows.h"      // add_row (and dca_internal.h)

#include <functional>
#include <type_traits>

// kSiteThreads, kSitePerLane, kSiteSeqBlock, kSiteMaxCJ, kSiteChunkBudget, qm_of, chunk_blocks and site_lds: potts_plan.h

// f(std::integral_constant<int, qm_of(q)>): a run-time q to a QM template argument (decltype(qm)::value)
template <typename F>
auto with_qm(int q, F&& f)
{
    switch (qm_of(q)) {
    case 8: return f(std::integral_constant<int, 8>());
    case 24: return f(std::integral_constant<int, 24>());
    default: return f(std::integral_constant<int, 32>());
    }
}

// The body of a site kernel (kSiteThreads threads): site i, the queries seq0 .. seq0 + 511 of QT (site-major codes, NqS a
// multiple of 512 and > seq0 + 511; codes past nq are 0).  site: L x NqS doubles (site-major); cond: nq x L x q doubles (host
// layout) or NULL.  The policy P supplies what differs between the models:
//   int neighbours()             the sites j = 0 .. neighbours() - 1 are walked in ascending order,
//   bool skip(j)                 ... except these
//   S load(j, hi, lo)            element hi * q + lo of the stored block of the pair (i, j); the reads run along lo
//   int lds_pos(j, hi, lo)       where it goes in the staged block: b * QM + a for the term J_j(a, b = s_j)
//   double field(a)              h_i(a)
//   void epilogue(n, u, m, lz, si)   after query n's site value is written (u: its QM accumulators, si its code at site i)
template <typename S, int QM, typename Policy>
__device__ __forceinline__ void site_conditional_body(const Policy& P, int i, int seq0, int L, int q, const uint8_t* __restrict__ QT,
                                                      int nq, int NqS, double* __restrict__ site, double* __restrict__ cond)
{
    constexpr int CJ = chunk_blocks<S, QM>();
    constexpr int KPB = site_kpb<QM>();                                      // block elements per thread (q * q <= 256 * KPB)
    constexpr int codeBytes = CJ * kSiteSeqBlock;
    constexpr int CPT = site_cpt<S, QM>();                                    // 16-byte code pieces per thread
    static_assert(CPT <= 2, "at most two code pieces per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char site_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* bufJ = reinterpret_cast<S*>(site_smem);
    uint8_t* bufC = site_smem + ((size_t)2 * bufVals * sizeof(S) + 15) / 16 * 16;
    const int tid = threadIdx.x;
    const int qq = q * q;
    const int nb = P.neighbours();
    const int steps = (nb + CJ - 1) / CJ;

    // this thread's block elements k = tid + kk * 256 < q * q: (hi, lo) = (k / q, k % q) of the stored block
    int kHi[KPB], kLo[KPB];
#pragma unroll
    for (int kk = 0; kk < KPB; ++kk) {
        const int k = tid + kk * kSiteThreads;
        kHi[kk] = k < qq ? k / q : -1;
        kLo[kk] = k < qq ? k - (k / q) * q : 0;
    }

    for (int e = tid; e < 2 * bufVals; e += kSiteThreads) bufJ[e] = (S)0;  // the row padding stays zero

    S val[CJ][KPB];
    uint4 cv0 = {}, cv1 = {};                                 // the chunk's codes (kept out of an array: no stack)
    // registers <- chunk t: the blocks of the neighbours j0 .. j0 + CJ - 1 and their codes
    auto load = [&](int t) {
        const int j0 = t * CJ;
#pragma unroll
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= nb || P.skip(j)) continue;
#pragma unroll
            for (int kk = 0; kk < KPB; ++kk)
                if (kHi[kk] >= 0) val[jj][kk] = P.load(j, kHi[kk], kLo[kk]);
        }
        // 16-byte piece e: row e / 32, bytes (e % 32) * 16 ..
        if (tid / 32 < CJ && j0 + tid / 32 < nb) cv0 = *reinterpret_cast<const uint4*>(QT + (size_t)(j0 + tid / 32) * NqS + seq0 + (tid & 31) * 16);
        if constexpr (CPT > 1) {
            const int e = tid + kSiteThreads;
            if (e / 32 < CJ && j0 + e / 32 < nb) cv1 = *reinterpret_cast<const uint4*>(QT + (size_t)(j0 + e / 32) * NqS + seq0 + (e & 31) * 16);
        }
    };
    auto store = [&](int t) {
        const int j0 = t * CJ;
        S* bj = bufJ + (t & 1) * bufVals;
        uint8_t* bc = bufC + (t & 1) * codeBytes;
#pragma unroll
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= nb || P.skip(j)) continue;
#pragma unroll
            for (int kk = 0; kk < KPB; ++kk)
                if (kHi[kk] >= 0) bj[jj * blk + P.lds_pos(j, kHi[kk], kLo[kk])] = val[jj][kk];
        }
        if (tid / 32 < CJ && j0 + tid / 32 < nb) *reinterpret_cast<uint4*>(bc + (tid / 32) * kSiteSeqBlock + (tid & 31) * 16) = cv0;
        if constexpr (CPT > 1) {
            const int e = tid + kSiteThreads;
            if (e / 32 < CJ && j0 + e / 32 < nb) *reinterpret_cast<uint4*>(bc + (e / 32) * kSiteSeqBlock + (e & 31) * 16) = cv1;
        }
    };

    double u[kSitePerLane][QM];
#pragma unroll
    for (int a = 0; a < QM; ++a) {
        const double h = a < q ? P.field(a) : 0.0;
#pragma unroll
        for (int p = 0; p < kSitePerLane; ++p) u[p][a] = h;
    }

    __syncthreads();
    if (steps > 0) {
        load(0);
        store(0);
    }
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const int j0 = t * CJ;
        if (t + 1 < steps) load(t + 1);
        const S* cur = bufJ + (t & 1) * bufVals;
        const uint8_t* cc = bufC + (t & 1) * codeBytes;
#pragma unroll 1
        for (int jj = 0; jj < CJ; ++jj) {
            const int j = j0 + jj;
            if (j >= nb) break;
            if (P.skip(j)) continue;
#pragma unroll
            for (int p = 0; p < kSitePerLane; ++p)
                add_row<S, QM>(u[p], cur + jj * blk + (int)cc[jj * kSiteSeqBlock + p * kSiteThreads + tid] * QM);
        }
        if (t + 1 < steps) store(t + 1);
        __syncthreads();
    }

#pragma unroll
    for (int p = 0; p < kSitePerLane; ++p) {
        const int n = seq0 + p * kSiteThreads + tid;
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
        P.epilogue(n, u[p], m, lz, si);
        if (cond) {
            double* out = cond + ((size_t)n * L + i) * q;
#pragma unroll
            for (int a = 0; a < QM; ++a) if (a < q) out[a] = (u[p][a] - m) - lz;
        }
    }
}

// ---- pll.hip: the host side of a site kernel
// queries per pass: the device scratch of a pass (perSeq bytes per query) within `budget`, in whole workgroups; the environment
// variable `env` (a positive count, rounded down to the granule) caps it; never more than n rounded up to the granule
int site_pass_size(int n, size_t perSeq, size_t budget, const char* env, int granule);

// sum[n] = sum_i site[i][n] (ascending i); rows (nq x L) or NULL: the site values in the host layout
hipError_t dca_site_finish(dca_ctx* ctx, const double* dSite, int L, int nq, int NqS, double* dSum, double* dRows);

// The site values of host rows X (n x L codes < q), pass by pass: upload, site-major copy, launch(dQT, nq, NqS, dSite, dCond)
// and the finish kernel under the clock `tag`, copies back.  sum_out: n; site_out (n x L) and cond_out (n x L x q) may be NULL.
struct SitePasses { size_t budget; const char* env; int granule; const char* tag; };
using SiteLaunch = std::function<hipError_t(const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond)>;
hipError_t dca_site_passes(dca_ctx* ctx, const SitePasses& sp, int L, int q, const uint8_t* X, int n, double* sum_out, double* site_out,
                           double* cond_out, const SiteLaunch& launch);
