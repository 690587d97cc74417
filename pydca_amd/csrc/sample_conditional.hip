// Conditional Gibbs sampling of a fitted Potts model: sample.hip's systematic scan over a list of F free sites
// f_0 < ... < f_{F-1}, every other site clamped to the chain's own row of `initial` (dca_plm_sample_conditional,
// dca_mf_sample_conditional).  The model arrives as a PottsSource and is read through the free
// functions of potts_source.h.
//
// Two kernels, both with lane = chain:
//   cond_fields_kernel   once per call and block of chains: c_i(a) = h_i(a) + sum over the clamped j, ascending, of
//                        J_ij(a, s_j), a sequential double sum (site_conditionals.h's order: h first, then j ascending), for
//                        every free site i = f_kappa and state a, written as fld[(kappa * q + a) * nS + c].  With no clamped
//                        site it is the widened h.
//   cond_sweep_kernel    one launch per sweep (the staging and the row add: potts_rows.h): gibbs_sweep_kernel's geometry (64 chains per workgroup, 4 waves, wave w sums
//                        the positions k = w (mod 4), double-buffered chunks of CJ transposed blocks through LDS, the partials
//                        meet in LDS in ascending w, wave 0 draws) with the chunk loop over the free POSITIONS k: the block
//                        read is the one of the site j = f_k, in place, and wave 0 starts from fld instead of the field.  So
//                          u(a) = (((c_i(a) + S_0(a)) + S_1(a)) + S_2(a)) + S_3(a),  S_w(a) = sum over k = w (mod 4), k != kappa,
//                        ascending k (S_0's terms join c_i(a) one by one, S_1 .. S_3 start from 0), the draw rule is sample.hip's
//                        and the Philox counter is (chain, sweep, i, 0) with the SITE index i.  With F = L this is
//                        gibbs_sweep_kernel operation for operation.  A sweep reads the F x F sub-table of J and the codes of
//                        the free sites only (in LDS when F <= kSResidentL, else in the site-major state buffer).
// The field buffer (F x q doubles per chain) stays within kCFieldBudget: blocks of chains (multiples of 64; the environment
// variable DCA_COND_PASS caps them) run one after another.  A chain's bits depend on nothing but its own row, so the split
// does not show.  No atomics, no communication between workgroups.
#include "site_conditionals.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

// tag-1 start of the free sites: s_i = floor(U * q), counter (chain, 0, i, 1) with the site index i; chains past n keep code 0
__global__ void cond_random_start_kernel(int n, int q, int nS, const int* __restrict__ freeS, int F, uint64_t seed, uint64_t first_chain,
                                         uint8_t* __restrict__ st)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)F * nS) return;
    const int k = (int)(t / nS), c = (int)(t % nS);
    const int i = freeS[k];
    if (c < n) st[(size_t)i * nS + c] = (uint8_t)(int)(philox_uniform(seed, first_chain + c, 0, i, 1) * q);
}

// The field pass.  grid (F, ceil(nS / 256)); thread = chain c of the block (all nS of them: the padding chains are swept too).
// LDS: two chunk buffers (CJ blocks of q x QM values of S each).  state: site-major codes st[j * nS + c]; clamped: the nC
// sites outside freeS, ascending.  R: chunk elements per thread.
template <typename S, int QM, int R>
__global__ __launch_bounds__(kCFieldChains)
void cond_fields_kernel(const S* __restrict__ src, int kind, const double* __restrict__ mfh, int L, int q, int ld, int CJ,
                        const int* __restrict__ freeS, const int* __restrict__ clamped, int nC, const uint8_t* __restrict__ state,
                        int nS, double* __restrict__ fld)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cond_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* buf0 = reinterpret_cast<S*>(cond_smem);
    const int tid = threadIdx.x;
    const int kappa = blockIdx.x, i = freeS[kappa];
    const int c = blockIdx.y * kCFieldChains + tid;
    const bool live = c < nS;
    const int qq = q * q;
    const uint32_t mqq = 0xffffffffu / (uint32_t)qq + 1, mq = 0xffffffffu / (uint32_t)q + 1;
    const int steps = (nC + CJ - 1) / CJ;
    const int chunkVals = CJ * qq;

    for (int e = tid; e < 2 * bufVals; e += kCFieldChains) buf0[e] = (S)0;      // the row padding stays zero

    double u[QM];
#pragma unroll
    for (int a = 0; a < QM; ++a) u[a] = a < q ? potts_field(src, mfh, kind, q, i, a) : 0.0;

    S val[R];
    int dst[R];
    __syncthreads();
    if (steps > 0) {
        row_chunk_load<S, QM, R, kCFieldChains>(src, kind, L, q, ld, ListedSites(clamped, nC), -1, i, 0, chunkVals, mqq, mq, val, dst);
        row_chunk_store<S, R>(buf0, val, dst);
    }
    __syncthreads();

    for (int t = 0; t < steps; ++t) {
        const int k0 = t * CJ;
        if (t + 1 < steps) row_chunk_load<S, QM, R, kCFieldChains>(src, kind, L, q, ld, ListedSites(clamped, nC), -1, i, k0 + CJ, chunkVals, mqq, mq, val, dst);
        const S* cur = buf0 + (t & 1) * bufVals;
        if (live) {
#pragma unroll 1
            for (int jj = 0; jj < CJ; ++jj) {
                if (k0 + jj >= nC) break;
                const int j = clamped[k0 + jj];
                add_row<S, QM>(u, cur + jj * blk + (int)state[(size_t)j * nS + c] * QM);
            }
        }
        if (t + 1 < steps) row_chunk_store<S, R>(buf0 + ((t + 1) & 1) * bufVals, val, dst);
        __syncthreads();
    }
    if (live) {
#pragma unroll
        for (int a = 0; a < QM; ++a)
            if (a < q) fld[((size_t)kappa * q + a) * nS + c] = u[a];
    }
}

// One sweep over the free sites.  grid: nS / 64 workgroups.  LDS as gibbs_sweep_kernel's at F sites: two chunk buffers, the
// partial buffer (QM x 64 doubles), and with RES the free sites' codes (F x 64 bytes, position-major) and the site list (F ints:
// the chunk loads look every element's site up, and from global memory that lookup is a second dependent load per element).
template <typename S, int QM, bool RES, int R>
__global__ __launch_bounds__(kSThreads)
void cond_sweep_kernel(const S* __restrict__ src, int kind, int L, int q, int ld, int CJ, const int* __restrict__ freeS, int F,
                       const double* __restrict__ fld, uint8_t* __restrict__ state, int nS, uint64_t seed, uint64_t first_chain,
                       uint64_t sweep, double beta)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cond_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* buf0 = reinterpret_cast<S*>(cond_smem);
    double* P = reinterpret_cast<double*>(cond_smem + ((size_t)2 * bufVals * sizeof(S) + 15) / 16 * 16);
    uint8_t* stL = reinterpret_cast<uint8_t*>(P + QM * kSChains);
    int* listL = reinterpret_cast<int*>(stL + (size_t)F * kSChains);
    const int* sites = RES ? listL : freeS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * kSChains;
    const uint64_t chain = first_chain + (uint64_t)(c0 + lane);
    const int qq = q * q;
    const uint32_t mqq = 0xffffffffu / (uint32_t)qq + 1, mq = 0xffffffffu / (uint32_t)q + 1;
    const int nch = (F + CJ - 1) / CJ;
    const int steps = F * nch;
    const int chunkVals = CJ * qq;

    for (int e = tid; e < 2 * bufVals; e += kSThreads) buf0[e] = (S)0;      // the row padding stays zero
    if (RES) {
        for (int e = tid; e < F * kSChains; e += kSThreads) stL[e] = state[(size_t)freeS[e >> 6] * nS + c0 + (e & 63)];
        for (int e = tid; e < F; e += kSThreads) listL[e] = freeS[e];
    }

    S val[R];
    int dst[R];
    // registers <- the chunk of step t (position t / nch, blocks of the positions k0 .. k0 + CJ - 1)
    auto load = [&](int t) {
        const int kappa = t / nch, k0 = (t - kappa * nch) * CJ;
        row_chunk_load<S, QM, R, kSThreads>(src, kind, L, q, ld, ListedSites(sites, F), kappa, sites[kappa], k0, chunkVals, mqq, mq, val, dst);
    };
    auto code = [&](int k) -> int { return RES ? stL[k * kSChains + lane] : state[(size_t)sites[k] * nS + c0 + lane]; };

    __syncthreads();
    load(0);
    row_chunk_store<S, R>(buf0, val, dst);
    __syncthreads();

    double u[QM];
    for (int t = 0; t < steps; ++t) {
        const int kappa = t / nch, ch = t - kappa * nch, k0 = ch * CJ;
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < QM; ++a) u[a] = (wave == 0 && a < q) ? fld[((size_t)kappa * q + a) * nS + c0 + lane] : 0.0;
        }
        if (t + 1 < steps) load(t + 1);
        const S* cur = buf0 + (t & 1) * bufVals;
        for (int jj = wave; jj < CJ; jj += 4) {
            const int k = k0 + jj;
            if (k >= F) break;
            if (k == kappa) continue;
            add_row<S, QM>(u, cur + jj * blk + code(k) * QM);
        }
        if (t + 1 < steps) row_chunk_store<S, R>(buf0 + ((t + 1) & 1) * bufVals, val, dst);
        if (ch == nch - 1) {                                  // position kappa complete: S_1, S_2, S_3 join wave 0's c + S_0 in order
            for (int w = 1; w < 4; ++w) {
                if (wave == w)
#pragma unroll
                    for (int a = 0; a < QM; ++a) P[a * kSChains + lane] = u[a];
                __syncthreads();
                if (wave == 0)
#pragma unroll
                    for (int a = 0; a < QM; ++a) u[a] += P[a * kSChains + lane];
                __syncthreads();
            }
            if (wave == 0) {
                const int i = sites[kappa];
                double m = u[0];
#pragma unroll
                for (int a = 1; a < QM; ++a) if (a < q) m = fmax(m, u[a]);
                double T = 0.0;
#pragma unroll
                for (int a = 0; a < QM; ++a) {
                    u[a] = a < q ? exp(beta * (u[a] - m)) : 0.0;
                    T += u[a];
                }
                const double r = philox_uniform(seed, chain, sweep, i, 0) * T;
                int pick = -1, last = 0;
                double cum = 0.0;
#pragma unroll
                for (int a = 0; a < QM; ++a) {
                    if (a < q) {
                        cum += u[a];
                        if (pick < 0 && cum > r) pick = a;
                        if (u[a] > 0.0) last = a;
                    }
                }
                if (pick < 0) pick = last;
                if (RES) stL[kappa * kSChains + lane] = (uint8_t)pick;
                else state[(size_t)i * nS + c0 + lane] = (uint8_t)pick;
            }
        }
        __syncthreads();
    }
    if (RES)
        for (int e = tid; e < F * kSChains; e += kSThreads) state[(size_t)freeS[e >> 6] * nS + c0 + (e & 63)] = stL[e];
}

// what the launches of one block of chains take besides the model
struct CondArgs {
    const int* dFree; int F; const int* dClamped; int nC; double* dFld; uint8_t* dState; int nS;
    uint64_t seed, first_chain, sweep; double beta;
};

template <typename S, int QM>
hipError_t launch_fields(dca_ctx* ctx, const CondSampleGeom& g, const PottsView<S>& pv, const CondArgs& a)
{
    constexpr int R = cond_field_regs(sizeof(S));
    auto kern = cond_fields_kernel<S, QM, R>;
    HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.ldsFields));
    hipLaunchKernelGGL(kern, dim3(a.F, ceil_div(a.nS, kCFieldChains)), dim3(kCFieldChains), g.ldsFields, ctx->stream, pv.src, pv.kind,
                       pv.mfh, pv.L, pv.q, pv.ld, g.CJF, a.dFree, a.dClamped, a.nC, (const uint8_t*)a.dState, a.nS, a.dFld);
    return hipGetLastError();
}

template <typename S, int QM, bool RES>
hipError_t launch_cond_sweep(dca_ctx* ctx, const CondSampleGeom& g, const PottsView<S>& pv, const CondArgs& a)
{
    constexpr int R = sample_regs(sizeof(S));
    auto kern = cond_sweep_kernel<S, QM, RES, R>;
    HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    hipLaunchKernelGGL(kern, dim3(a.nS / kSChains), dim3(kSThreads), g.lds, ctx->stream, pv.src, pv.kind, pv.L, pv.q, pv.ld, g.CJ,
                       a.dFree, a.F, (const double*)a.dFld, a.dState, a.nS, a.seed, a.first_chain, a.sweep, a.beta);
    return hipGetLastError();
}

// the field pass (under "cond_fields") and `sweeps` sweep launches (each under "sample_cond") of one block of chains
template <typename S>
hipError_t run_block(dca_ctx* ctx, const CondSampleGeom& g, const PottsView<S>& pv, CondArgs a, int sweeps)
{
    return with_qm(pv.q, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        {
            ScopedKernelClock kc(ctx, "cond_fields");
            HIP_PASS((launch_fields<S, QM>(ctx, g, pv, a)));
        }
        for (int t = 0; t < sweeps; ++t, ++a.sweep) {               // one launch per sweep
            ScopedKernelClock kc(ctx, "sample_cond");
            if (g.res) HIP_PASS((launch_cond_sweep<S, QM, true>(ctx, g, pv, a)));
            else HIP_PASS((launch_cond_sweep<S, QM, false>(ctx, g, pv, a)));
        }
        return hipSuccess;
    });
}

}  // namespace

int dca_check_free_sites(const int32_t* free_sites, int F, int L, const char* who)
{
    if (F < 0 || F > L || (F > 0 && !free_sites)) {
        dca_set_error("%s: num_free %d outside [0, %d], or free_sites NULL", who, F, L);
        return DCA_ERR_ARG;
    }
    for (int k = 0; k < F; ++k) {
        if (free_sites[k] < 0 || free_sites[k] >= L || (k > 0 && free_sites[k] <= free_sites[k - 1])) {
            dca_set_error("%s: free_sites[%d] = %d is outside [0, %d) or not above its predecessor", who, k, (int)free_sites[k], L);
            return DCA_ERR_ARG;
        }
    }
    return DCA_OK;
}

int dca_potts_sample_conditional(dca_ctx* ctx, const PottsSource& ps, int n, int sweeps, uint64_t seed, uint64_t first_chain,
                                 uint64_t first_sweep, double beta, const int32_t* free_sites, int num_free, const uint8_t* initial,
                                 int random_start, uint8_t* out)
{
    static const char* who = "sample_conditional";
    const int L = ps.L, q = ps.q, F = num_free;
    if (n < 0 || sweeps < 0 || !(beta >= 0.0) || std::isinf(beta) || (n > 0 && (!initial || !out))) {
        dca_set_error("%s: bad arguments (n %d, sweeps %d, beta %g, initial %s, out %s)", who, n, sweeps, beta, initial ? "given" : "NULL",
                      out ? "given" : "NULL");
        return DCA_ERR_ARG;
    }
    DCA_TRY(dca_check_free_sites(free_sites, F, L, who));
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(initial, (size_t)n * L, q, "sample_conditional: initial "));

    // the free sites, then the clamped ones, both ascending
    std::vector<int> lists((size_t)L);
    std::vector<char> isFree((size_t)L, 0);
    for (int k = 0; k < F; ++k) { lists[k] = free_sites[k]; isFree[free_sites[k]] = 1; }
    for (int j = 0, k = F; j < L; ++j)
        if (!isFree[j]) lists[k++] = j;
    const bool run = F > 0 && sweeps > 0;

    const int cap = site_pass_size(n, std::max<size_t>(1, (size_t)F * q * sizeof(double)), kCFieldBudget, "DCA_COND_PASS", kSChains);
    const int nS = (int)round_up((size_t)cap, kSChains);
    const CondSampleGeom g = cond_sample_geometry(std::max(F, 1), q, ps.dtype == DCA_F32 ? 4 : 8);
    DevBuf<int> dLists;
    DevBuf<uint8_t> dRows, dState;
    DevBuf<double> dFld;
    HIP_TRY_AS_NOMEM(dLists.alloc((size_t)L, false), who);
    HIP_TRY_AS_NOMEM(dRows.alloc((size_t)cap * L, false), who);
    HIP_TRY_AS_NOMEM(dState.alloc((size_t)L * nS, false), who);
    if (run) HIP_TRY_AS_NOMEM(dFld.alloc((size_t)F * q * nS, false), who);
    HIP_TRY_AS(hipMemcpyAsync(dLists, lists.data(), (size_t)L * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);

    for (int first = 0; first < n; first += cap) {
        const int nb = std::min(cap, n - first);
        HIP_TRY_AS(hipMemcpyAsync(dRows, initial + (size_t)first * L, (size_t)nb * L, hipMemcpyHostToDevice, ctx->stream), who);
        HIP_TRY_AS(dca_rows_to_sites(ctx, dRows, (size_t)L, nb, L, nS, dState), who);
        if (random_start && F > 0) {
            const size_t total = (size_t)F * nS;
            hipLaunchKernelGGL(cond_random_start_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, nb, q, nS,
                               (const int*)dLists.get(), F, seed, first_chain + (uint64_t)first, dState.get());
            HIP_TRY_AS(hipGetLastError(), who);
        }
        if (run) {
            const CondArgs a{dLists.get(), F, dLists.get() + F, L - F, dFld.get(), dState.get(), nS,
                             seed, first_chain + (uint64_t)first, first_sweep, beta};
            HIP_TRY_AS(with_source_type(ps, [&](auto pv) { return run_block(ctx, g, pv, a, sweeps); }), who);
        }
        HIP_TRY_AS(dca_sites_to_rows(ctx, dState, nb, L, nS, dRows), who);
        HIP_TRY_AS(hipMemcpyAsync(out + (size_t)first * L, dRows, (size_t)nb * L, hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    }
    return DCA_OK;
}
