// Greedy ascent of the Potts energy to a local maximum, with clamped sites (dca_plm_ascend, dca_mf_ascend; DESIGN.md
// section 24): every chain repeatedly applies the single mutation of a free site with the largest gain until none exceeds
// min_gain.  The model arrives as a PottsSource and is read in place through the free functions of potts_source.h.
//
// Two kernels:
//   ascent_table_kernel   once per call and block of chains, lane = chain (cond_fields_kernel's style; the chunk staging is potts_rows.h's): the local-field table
//                         U_i(a) = h_i(a) + sum over j != i, ascending, of J_ij(a, s_j), a sequential double sum (h first, then j
//                         ascending: site_conditionals.h's order), for every free site i = f_kappa and state a, written as
//                         tab[(c * F + kappa) * q + a].  The blocks of row i stream through LDS in double-buffered chunks.
//   ascent_kernel         one launch runs all steps of all chains of the block; one workgroup = one chain, a persistent loop.
//                         The table sits in LDS (copied once from tab) or stays in tab; thread t owns the free positions
//                         k = t (mod 256) with their rows of the table and their codes.  One pass per step: the owner adds
//                         J_{j i*}(b, a*) - J_{j i*}(b, old) (the difference first) to its rows after the previous move, then
//                         scans g = U_k(a) - U_k(s_k); the candidates meet in a wave shuffle tree and one LDS exchange under the
//                         total order (g descending, position ascending, state ascending), which is associative: any tree
//                         names the same winner.  J is read in place: a row of block (i*, j) for j > i*, a column of block
//                         (j, i*) for j < i*.  No atomics, no communication between workgroups, no host round trip.
// The tables (and the path records) of one block of chains stay within kAscScratchBudget: blocks run one after another
// (DCA_ASCENT_PASS caps them).  A chain's bits depend on nothing but its own row, so neither the split nor the table's place shows.
#include "site_conditionals.h"
#include "ascent_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

// The table pass.  grid (F, ceil(nb / 256)); thread = chain c of the block.  LDS: two chunk buffers (CJ blocks of q x QM values
// of S each).  state: site-major codes st[j * nS + c].  R: chunk elements per thread.
template <typename S, int QM, int R>
__global__ __launch_bounds__(kAscInitChains)
void ascent_table_kernel(const S* __restrict__ src, int kind, const double* __restrict__ mfh, int L, int q, int ld, int CJ,
                         const int* __restrict__ freeS, int F, const uint8_t* __restrict__ state, int nb, int nS, double* __restrict__ tab)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char asc_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* buf0 = reinterpret_cast<S*>(asc_smem);
    const int tid = threadIdx.x;
    const int kappa = blockIdx.x, i = freeS[kappa];
    const int c = blockIdx.y * kAscInitChains + tid;
    const bool live = c < nb;
    const int qq = q * q;
    const uint32_t mqq = 0xffffffffu / (uint32_t)qq + 1, mq = 0xffffffffu / (uint32_t)q + 1;
    const int steps = (L + CJ - 1) / CJ;
    const int chunkVals = CJ * qq;

    for (int e = tid; e < 2 * bufVals; e += kAscInitChains) buf0[e] = (S)0;      // the row padding stays zero

    double u[QM];
#pragma unroll
    for (int a = 0; a < QM; ++a) u[a] = a < q ? potts_field(src, mfh, kind, q, i, a) : 0.0;

    S val[R];
    int dst[R];
    __syncthreads();
    row_chunk_load<S, QM, R, kAscInitChains>(src, kind, L, q, ld, AllSites(nullptr, L), i, i, 0, chunkVals, mqq, mq, val, dst);
    row_chunk_store<S, R>(buf0, val, dst);
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const int j0 = t * CJ;
        if (t + 1 < steps) row_chunk_load<S, QM, R, kAscInitChains>(src, kind, L, q, ld, AllSites(nullptr, L), i, i, j0 + CJ, chunkVals, mqq, mq, val, dst);
        const S* cur = buf0 + (t & 1) * bufVals;
        if (live) {
#pragma unroll 1
            for (int jj = 0; jj < CJ; ++jj) {
                const int j = j0 + jj;
                if (j >= L) break;
                if (j == i) continue;
                const S* row = cur + jj * blk + (int)state[(size_t)j * nS + c] * QM;
                // add_row's text, inline: through the helper this kernel alone compiled to other instructions
                if constexpr (sizeof(S) == 4) {
#pragma unroll
                    for (int a = 0; a < QM; a += 4) {
                        const float4 v = *reinterpret_cast<const float4*>(row + a);
                        u[a] += (double)v.x; u[a + 1] += (double)v.y; u[a + 2] += (double)v.z; u[a + 3] += (double)v.w;
                    }
                } else {
#pragma unroll
                    for (int a = 0; a < QM; a += 2) {
                        const double2 v = *reinterpret_cast<const double2*>(row + a);
                        u[a] += v.x; u[a + 1] += v.y;
                    }
                }
            }
        }
        if (t + 1 < steps) row_chunk_store<S, R>(buf0 + ((t + 1) & 1) * bufVals, val, dst);
        __syncthreads();
    }
    if (live) {
        double* out = tab + ((size_t)c * F + kappa) * q;
#pragma unroll
        for (int a = 0; a < QM; ++a)
            if (a < q) out[a] = u[a];
    }
}

// a candidate move: the gain, the free position and (new state) | (current state) << 8
struct AscCand { double g; int k, code; };

// the total order: g descending, then position ascending, then new state ascending
__device__ __forceinline__ bool asc_better(const AscCand& x, const AscCand& y)
{
    if (x.g != y.g) return x.g > y.g;
    if (x.k != y.k) return x.k < y.k;
    return (x.code & 255) < (y.code & 255);
}

// The ascent.  grid: nb workgroups, workgroup c = chain c of the block.  Dynamic LDS: with TLDS the table (F x q doubles), then
// the site list (F ints) and the free sites' codes (F bytes).  rows: nb x L codes, read at the free sites and written back there.
// path (nb x max_steps x 2) and path_gain (nb x max_steps) may be NULL; the caller has filled them with -1 and 0.
template <typename S, bool TLDS>
__global__ __launch_bounds__(kAscThreads)
void ascent_kernel(const S* __restrict__ src, int kind, int L, int q, int ld, const int* __restrict__ freeS, int F, double* __restrict__ tab,
                   uint8_t* __restrict__ rows, int max_steps, double min_gain, int* __restrict__ steps_out, uint8_t* __restrict__ conv_out,
                   double* __restrict__ gain_out, int* __restrict__ path, double* __restrict__ path_gain)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char asc_smem[];
    __shared__ double redG[2][kAscThreads / 64];
    __shared__ int redK[2][kAscThreads / 64], redC[2][kAscThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x;
    const size_t tabVals = (size_t)F * q;
    double* U = TLDS ? reinterpret_cast<double*>(asc_smem) : tab + (size_t)c * tabVals;
    int* listL = reinterpret_cast<int*>(asc_smem + (TLDS ? tabVals * sizeof(double) : 0));
    uint8_t* sL = reinterpret_cast<uint8_t*>(listL + F);
    uint8_t* row = rows + (size_t)c * L;

    if (TLDS) {
        const double* g0 = tab + (size_t)c * tabVals;
        for (size_t e = tid; e < tabVals; e += kAscThreads) U[e] = g0[e];
    }
    for (int k = tid; k < F; k += kAscThreads) {
        const int j = freeS[k];
        listL[k] = j;
        sL[k] = row[j];
    }
    __syncthreads();

    int t = 0, conv = 0;
    int mk = -1, mi = 0, ma = 0, mo = 0;                       // the move applied last: position, site, new and old state
    double gain = 0.0;
    for (;;) {
        AscCand best{-INFINITY, INT_MAX, 0};
        for (int k = tid; k < F; k += kAscThreads) {          // ascending k, strict >: the smallest (k, a) among a thread's ties
            const int j = listL[k], sj = sL[k];
            double* Uk = U + (size_t)k * q;
            if (mk >= 0 && k != mk) {
                if (j > mi) {                                   // row a* and row old of block (i*, j)
                    for (int b = 0; b < q; ++b)
                        Uk[b] += potts_coupling(src, kind, L, q, ld, mi, j, ma, b) - potts_coupling(src, kind, L, q, ld, mi, j, mo, b);
                } else {                                        // column a* and column old of block (j, i*)
                    for (int b = 0; b < q; ++b)
                        Uk[b] += potts_coupling(src, kind, L, q, ld, j, mi, b, ma) - potts_coupling(src, kind, L, q, ld, j, mi, b, mo);
                }
            }
            const double us = Uk[sj];
            for (int a = 0; a < q; ++a) {
                const double g = Uk[a] - us;
                if (a != sj && g > best.g) best = AscCand{g, k, a | (sj << 8)};
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            AscCand o;
            o.g = __shfl_down(best.g, off);
            o.k = __shfl_down(best.k, off);
            o.code = __shfl_down(best.code, off);
            if (asc_better(o, best)) best = o;
        }
        const int slot = t & 1;
        if (lane == 0) { redG[slot][wave] = best.g; redK[slot][wave] = best.k; redC[slot][wave] = best.code; }
        __syncthreads();
        best = AscCand{redG[slot][0], redK[slot][0], redC[slot][0]};
#pragma unroll
        for (int w = 1; w < kAscThreads / 64; ++w) {
            const AscCand o{redG[slot][w], redK[slot][w], redC[slot][w]};
            if (asc_better(o, best)) best = o;
        }
        if (!(best.g > min_gain)) { conv = 1; break; }
        if (t >= max_steps) break;
        mk = best.k; mi = listL[mk]; ma = best.code & 255; mo = best.code >> 8;
        if (tid == (mk & (kAscThreads - 1))) sL[mk] = (uint8_t)ma;      // the owner of position mk; nobody else reads its code
        if (tid == 0 && path) {
            path[((size_t)c * max_steps + t) * 2] = mi;
            path[((size_t)c * max_steps + t) * 2 + 1] = ma;
            path_gain[(size_t)c * max_steps + t] = best.g;
        }
        gain += best.g;
        ++t;
    }
    for (int k = tid; k < F; k += kAscThreads) row[listL[k]] = sL[k];
    if (tid == 0) {
        steps_out[c] = t;
        conv_out[c] = (uint8_t)conv;
        gain_out[c] = gain;
    }
}

// what the launches of one block of chains take besides the model
struct AscArgs {
    const int* dFree; int F; const uint8_t* dState; int nb, nS; double* dTab; uint8_t* dRows; int max_steps; double min_gain;
    int* dSteps; uint8_t* dConv; double* dGain; int* dPath; double* dPathGain;
};

template <typename S>
hipError_t run_block(dca_ctx* ctx, const AscentPlan& p, const PottsView<S>& pv, const AscArgs& a)
{
    HIP_PASS(with_qm(pv.q, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        constexpr int R = asc_init_regs(sizeof(S));
        ScopedKernelClock kc(ctx, "ascent_init");
        auto kern = ascent_table_kernel<S, QM, R>;
        HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.ldsInit));
        hipLaunchKernelGGL(kern, dim3(a.F, ceil_div(a.nb, kAscInitChains)), dim3(kAscInitChains), p.ldsInit, ctx->stream, pv.src, pv.kind,
                           pv.mfh, pv.L, pv.q, pv.ld, p.CJ, a.dFree, a.F, a.dState, a.nb, a.nS, a.dTab);
        return hipGetLastError();
    }));
    ScopedKernelClock kc(ctx, "ascent");
    auto kern = p.tableInLds ? ascent_kernel<S, true> : ascent_kernel<S, false>;
    HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.ldsAscent));
    hipLaunchKernelGGL(kern, dim3(a.nb), dim3(kAscThreads), p.ldsAscent, ctx->stream, pv.src, pv.kind, pv.L, pv.q, pv.ld, a.dFree, a.F,
                       a.dTab, a.dRows, a.max_steps, a.min_gain, a.dSteps, a.dConv, a.dGain, a.dPath, a.dPathGain);
    return hipGetLastError();
}

long env_long(const char* name, long unset)
{
    const char* v = getenv(name);
    return v && *v ? atol(v) : unset;
}

}  // namespace

int dca_potts_ascend(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, const int32_t* free_sites, int num_free, int max_steps,
                     double min_gain, uint8_t* out, int32_t* steps_out, uint8_t* converged_out, double* gain_out, int32_t* path_out,
                     double* path_gain_out)
{
    static const char* who = "ascend";
    const int L = ps.L, q = ps.q, F = num_free;
    if (n < 0 || max_steps < 0 || !(min_gain >= 0.0) || std::isinf(min_gain) || (n > 0 && (!X || !out || !steps_out || !converged_out))) {
        dca_set_error("%s: bad arguments (n %d, max_steps %d, min_gain %g, X %s, out %s, steps_out %s, converged_out %s, path_out %s, "
                      "path_gain_out %s)", who, n, max_steps, min_gain, X ? "given" : "NULL", out ? "given" : "NULL",
                      steps_out ? "given" : "NULL", converged_out ? "given" : "NULL", path_out ? "given" : "NULL",
                      path_gain_out ? "given" : "NULL");
        return DCA_ERR_ARG;
    }
    DCA_TRY(dca_check_free_sites(free_sites, F, L, who));
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(X, (size_t)n * L, q, "ascend: X "));

    const bool paths = path_out || path_gain_out;
    for (size_t e = 0, m = (size_t)n * max_steps; e < m; ++e) {
        if (path_out) path_out[2 * e] = path_out[2 * e + 1] = -1;
        if (path_gain_out) path_gain_out[e] = 0.0;
    }
    if (F == 0) {                                               // nothing may move: every chain rests where it is
        if (out != X) std::copy(X, X + (size_t)n * L, out);
        for (int k = 0; k < n; ++k) { steps_out[k] = 0; converged_out[k] = 1; if (gain_out) gain_out[k] = 0.0; }
        return DCA_OK;
    }

    const long ldsEnv = env_long("DCA_ASCENT_LDS", -1);
    const size_t ldsCap = ldsEnv < 0 ? kAscLdsTotal : std::min((size_t)ldsEnv, kAscLdsTotal);
    const AscentPlan p = ascent_plan(F, q, ps.dtype == DCA_F32 ? 4 : 8, ldsCap, paths, max_steps);
    const int cap = ascent_pass_chains(n, p.perChain, env_long("DCA_ASCENT_PASS", 0));
    const int nS = (int)round_up((size_t)cap, 64);
    const size_t pathVals = paths ? (size_t)cap * max_steps : 0;

    DevBuf<int> dFree, dSteps, dPath;
    DevBuf<uint8_t> dRows, dState, dConv;
    DevBuf<double> dTab, dGain, dPathGain;
    HIP_TRY_AS_NOMEM(dFree.alloc((size_t)F, false), who);
    HIP_TRY_AS_NOMEM(dRows.alloc((size_t)cap * L, false), who);
    HIP_TRY_AS_NOMEM(dState.alloc((size_t)L * nS, false), who);
    HIP_TRY_AS_NOMEM(dTab.alloc((size_t)cap * F * q, false), who);
    HIP_TRY_AS_NOMEM(dSteps.alloc((size_t)cap, false), who);
    HIP_TRY_AS_NOMEM(dConv.alloc((size_t)cap, false), who);
    HIP_TRY_AS_NOMEM(dGain.alloc((size_t)cap, false), who);
    if (pathVals) {
        HIP_TRY_AS_NOMEM(dPath.alloc(2 * pathVals, false), who);
        HIP_TRY_AS_NOMEM(dPathGain.alloc(pathVals, false), who);
    }
    HIP_TRY_AS(hipMemcpyAsync(dFree, free_sites, (size_t)F * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);

    for (int first = 0; first < n; first += cap) {
        const int nb = std::min(cap, n - first);
        HIP_TRY_AS(hipMemcpyAsync(dRows, X + (size_t)first * L, (size_t)nb * L, hipMemcpyHostToDevice, ctx->stream), who);
        HIP_TRY_AS(dca_rows_to_sites(ctx, dRows, (size_t)L, nb, L, nS, dState), who);
        const AscArgs a{dFree.get(), F, dState.get(), nb, nS, dTab.get(), dRows.get(), max_steps, min_gain,
                        dSteps.get(), dConv.get(), dGain.get(), dPath.get(), dPathGain.get()};
        HIP_TRY_AS(with_source_type(ps, [&](auto pv) { return run_block(ctx, p, pv, a); }), who);
        HIP_TRY_AS(hipMemcpyAsync(out + (size_t)first * L, dRows, (size_t)nb * L, hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipMemcpyAsync(steps_out + first, dSteps, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipMemcpyAsync(converged_out + first, dConv, (size_t)nb, hipMemcpyDeviceToHost, ctx->stream), who);
        if (gain_out) HIP_TRY_AS(hipMemcpyAsync(gain_out + first, dGain, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
        if (pathVals) {                                         // the applied steps only: the rest keeps the host's -1 / 0
            int maxT = 0;
            for (int k = 0; k < nb; ++k) maxT = std::max(maxT, (int)steps_out[first + k]);
            int32_t* po = path_out ? path_out + (size_t)first * max_steps * 2 : nullptr;
            double* pg = path_gain_out ? path_gain_out + (size_t)first * max_steps : nullptr;
            if (maxT > 0 && po)
                HIP_TRY_AS(hipMemcpy2D(po, (size_t)max_steps * 2 * sizeof(int), dPath, (size_t)max_steps * 2 * sizeof(int),
                                       (size_t)maxT * 2 * sizeof(int), nb, hipMemcpyDeviceToHost), who);
            if (maxT > 0 && pg)
                HIP_TRY_AS(hipMemcpy2D(pg, (size_t)max_steps * sizeof(double), dPathGain, (size_t)max_steps * sizeof(double),
                                       (size_t)maxT * sizeof(double), nb, hipMemcpyDeviceToHost), who);
            for (int k = 0; k < nb; ++k)
                for (int t = steps_out[first + k]; t < maxT; ++t) {
                    if (po) po[((size_t)k * max_steps + t) * 2] = po[((size_t)k * max_steps + t) * 2 + 1] = -1;
                    if (pg) pg[(size_t)k * max_steps + t] = 0.0;
                }
        }
    }
    return DCA_OK;
}
