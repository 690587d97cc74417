// Systematic-scan Gibbs sampling of a fitted Potts model, P(s) ~ exp(beta * E(s)), E as in energy.hip:
//   one sweep visits sites i = 0 .. L-1 in order; at site i chain c forms
//     u_i(a) = h_i(a) + sum_{j != i} J(a, s_j)        (J read from the pair block (min(i,j), max(i,j)), as energy.hip reads it)
//   for every state a < q (gap included) and draws s_i from p_a = exp(beta * (u_i(a) - max_b u_i(b))).
// The model arrives as a PottsSource and is read through PottsView (potts_source.h).
//
// Summation order (depends on (L, q, dtype) only): every term widened to double;
//   u(a) = (((h_i(a) + S_0(a)) + S_1(a)) + S_2(a)) + S_3(a),  S_w(a) = sum over j = w (mod 4), j != i, ascending j.
// Draw rule (restated by the tests): T = sum_a p_a ascending; r = U * T; s_i = the smallest a with p_0 + ... + p_a > r
// (ascending sums), or the largest a with p_a > 0 if rounding leaves none.  U = Philox4x32-10 of
//   key = (seed lo, seed hi), counter = (chain, sweep, site, tag) (each word the value mod 2^32), tag 0: Gibbs draw,
//   tag 1: initial state (sweep word 0, s_i = floor(U * q)); U = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53.  (Tag 2 is the AIS
//   start draw, ais.hip; tag 5 the exchange decision, tempered.hip.)  The kSweepInterp instantiations draw from the AIS
//   interpolation c(a) = h0_i(a) + bk (u(a) - h0_i(a)) instead of beta * u(a); the kSweepTempered ones (tempered.hip) are the
//   plain sweep with chain c's own beta_c, read from a device array, in the place of beta; the others compile to the plain sweep.
//
// Geometry: one workgroup of 4 waves holds 64 chains (lane = chain) in lockstep over the sites.  Wave w sums the j = w
// (mod 4) terms; the partials meet in LDS in ascending w and wave 0 draws.  Row i of J (L blocks of q x q) streams through
// LDS in double-buffered chunks of CJ blocks (CJ a multiple of 4), each block stored transposed, T[b][a] = J(a, b) with rows
// padded to QM values, so that a lane reads J(., s_j) as QM contiguous values; the next chunk's loads are in flight in
// registers while the current one is summed.  Chain codes live in LDS (64 x L bytes) when L <= kSResidentL, otherwise in
// the global site-major state buffer.  One launch is one sweep; no atomics, no inter-workgroup communication.  The state
// buffer lives in a DcaChains (dca_internal.h): dca_potts_sample makes one per call, a Boltzmann-learning run (boltzmann.hip)
// keeps its own on the device for the whole run.
#include "site_conditionals.h"

#include <cmath>

namespace {

// kSThreads, kSChains, kSResidentL, kSChunkBudget and sample_geometry: potts_plan.h

// rows (n x L) <-> site-major state (st[s * nS + c], nS a multiple of 64; chains past n start at code 0)
__global__ void rows_to_sites_kernel(const uint8_t* __restrict__ rows, size_t ld, int n, int L, int nS, uint8_t* __restrict__ st)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)L * nS) return;
    const int s = (int)(t / nS), c = (int)(t % nS);
    st[t] = c < n ? rows[(size_t)c * ld + s] : 0;
}

__global__ void sites_to_rows_kernel(const uint8_t* __restrict__ st, int n, int L, int nS, uint8_t* __restrict__ rows)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)n * L) return;
    const int c = (int)(t / L), s = (int)(t % L);
    rows[t] = st[(size_t)s * nS + c];
}

// initial state of tag 1: s_i = floor(U * q) (sweep word 0)
__global__ void initial_state_kernel(int n, int L, int q, int nS, uint64_t seed, uint64_t first_chain, uint8_t* __restrict__ st)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)L * nS) return;
    const int s = (int)(t / nS), c = (int)(t % nS);
    st[t] = c < n ? (uint8_t)(int)(philox_uniform(seed, first_chain + c, 0, s, 1) * q) : 0;
}

// One sweep.  grid: nS / 64 workgroups.  LDS: two chunk buffers (CJ blocks of q x QM values of S each), the partial
// buffer (QM x 64 doubles), and with RES the chain codes (L x 64 bytes, site-major).  R: chunk elements per thread.
// MODE kSweepInterp (annealed importance sampling, ais.hip): wave 0 draws from c(a) = h0_i(a) + bk * (u(a) - h0_i(a)),
// p_a = exp(c(a) - max_b c(b)), with aux = h0, the L x q base fields (device); beta is not used.  MODE kSweepTempered (replica
// exchange, tempered.hip): p_a = exp(beta_c * (u(a) - m)) with beta_c = aux[c], one value per chain of the state buffer (nS
// doubles, device); beta and bk are not used.  MODE kSweepPlain reads neither aux nor bk.
constexpr int kSweepPlain = 0, kSweepInterp = 1, kSweepTempered = 2;

template <typename S, int QM, bool RES, int R, int MODE>
__global__ __launch_bounds__(kSThreads)
void gibbs_sweep_kernel(const S* __restrict__ src, int kind, const double* __restrict__ mfh, int L, int q, int ld, int CJ,
                        uint8_t* __restrict__ state, int nS, uint64_t seed, uint64_t first_chain, uint64_t sweep, double beta,
                        const double* __restrict__ aux, double bk)
{
    constexpr bool INTERP = MODE == kSweepInterp;
    extern __shared__ __attribute__((aligned(16))) unsigned char sample_smem[];
    const int blk = q * QM;                                   // values of one staged block
    const int bufVals = CJ * blk;
    S* buf0 = reinterpret_cast<S*>(sample_smem);
    double* P = reinterpret_cast<double*>(sample_smem + ((size_t)2 * bufVals * sizeof(S) + 15) / 16 * 16);
    uint8_t* stL = reinterpret_cast<uint8_t*>(P + QM * kSChains);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * kSChains;
    const uint64_t chain = first_chain + (uint64_t)(c0 + lane);
    const int qq = q * q;
    const uint32_t mqq = 0xffffffffu / (uint32_t)qq + 1, mq = 0xffffffffu / (uint32_t)q + 1;
    const int nch = (L + CJ - 1) / CJ;
    const int steps = L * nch;
    const int chunkVals = CJ * qq;
    double betaC = beta;
    if constexpr (MODE == kSweepTempered) betaC = aux[c0 + lane];

    for (int e = tid; e < 2 * bufVals; e += kSThreads) buf0[e] = (S)0;      // the row padding stays zero
    if (RES)
        for (int e = tid; e < L * kSChains; e += kSThreads) stL[e] = state[(size_t)(e >> 6) * nS + c0 + (e & 63)];

    S val[R];
    int dst[R];
    // registers <- the chunk of step t (site t / nch, blocks j0 .. j0 + CJ - 1)
    auto load = [&](int t) {
        const int i = t / nch, j0 = (t - i * nch) * CJ;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int e = tid + r * kSThreads;
            dst[r] = -1;
            if (e >= chunkVals) continue;
            const int jj = fast_div(e, mqq), k = e - jj * qq;
            const int j = j0 + jj;
            if (j >= L || j == i) continue;
            const int hi = fast_div(k, mq), lo = k - hi * q;
            const int a = j > i ? hi : lo, b = j > i ? lo : hi;          // source order: (a, b) rows for j > i, (b, a) for j < i
            val[r] = (S)(j > i ? potts_coupling(src, kind, L, q, ld, i, j, a, b) : potts_coupling(src, kind, L, q, ld, j, i, b, a));
            dst[r] = jj * blk + b * QM + a;
        }
    };
    auto store = [&](S* buf) {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (dst[r] >= 0) buf[dst[r]] = val[r];
    };
    auto code = [&](int j) -> int { return RES ? stL[j * kSChains + lane] : state[(size_t)j * nS + c0 + lane]; };

    __syncthreads();
    load(0);
    store(buf0);
    __syncthreads();

    double u[QM];
    for (int t = 0; t < steps; ++t) {
        const int i = t / nch, ch = t - i * nch, j0 = ch * CJ;
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < QM; ++a) u[a] = (wave == 0 && a < q) ? potts_field(src, mfh, kind, q, i, a) : 0.0;
        }
        if (t + 1 < steps) load(t + 1);
        const S* cur = buf0 + (t & 1) * bufVals;
        for (int jj = wave; jj < CJ; jj += 4) {
            const int j = j0 + jj;
            if (j >= L) break;
            if (j == i) continue;
            const S* row = cur + jj * blk + code(j) * QM;
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
        if (t + 1 < steps) store(buf0 + ((t + 1) & 1) * bufVals);
        if (ch == nch - 1) {                                  // site i complete: S_1, S_2, S_3 join wave 0's h + S_0 in order
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
                if constexpr (INTERP) {
#pragma unroll
                    for (int a = 0; a < QM; ++a)
                        if (a < q) {
                            const double b0 = aux[(size_t)i * q + a];
                            u[a] = b0 + bk * (u[a] - b0);
                        }
                }
                double m = u[0];
#pragma unroll
                for (int a = 1; a < QM; ++a) if (a < q) m = fmax(m, u[a]);
                double T = 0.0;
#pragma unroll
                for (int a = 0; a < QM; ++a) {
                    if constexpr (INTERP) u[a] = a < q ? exp(u[a] - m) : 0.0;
                    else u[a] = a < q ? exp(betaC * (u[a] - m)) : 0.0;
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
                if (RES) stL[i * kSChains + lane] = (uint8_t)pick;
                else state[(size_t)i * nS + c0 + lane] = (uint8_t)pick;
            }
        }
        __syncthreads();
    }
    if (RES)
        for (int e = tid; e < L * kSChains; e += kSThreads) state[(size_t)(e >> 6) * nS + c0 + (e & 63)] = stL[e];
}

// what one sweep launch takes besides the model
// (h0: the interpolated sweep; betas: the tempered one; neither: the plain one)
struct SweepArgs { uint8_t* dState; int nS; uint64_t seed, first_chain, sweep; double beta; const double* h0; double bk; const double* betas; };

template <typename S, int QM, bool RES, int MODE>
hipError_t launch_sweep(dca_ctx* ctx, const SampleGeom& sg, const PottsView<S>& pv, const SweepArgs& a)
{
    constexpr int R = sample_regs(sizeof(S));
    auto kern = gibbs_sweep_kernel<S, QM, RES, R, MODE>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(a.nS / kSChains), dim3(kSThreads), sg.lds, ctx->stream, pv.src, pv.kind, pv.mfh, pv.L, pv.q, pv.ld,
                       sg.CJ, a.dState, a.nS, a.seed, a.first_chain, a.sweep, a.beta, MODE == kSweepTempered ? a.betas : a.h0, a.bk);
    return hipGetLastError();
}

template <typename S, int QM, int MODE>
hipError_t dispatch_res(dca_ctx* ctx, const SampleGeom& sg, const PottsView<S>& pv, const SweepArgs& a)
{
    if (sg.res) return launch_sweep<S, QM, true, MODE>(ctx, sg, pv, a);
    return launch_sweep<S, QM, false, MODE>(ctx, sg, pv, a);
}

template <typename S, int MODE>
hipError_t dispatch_qm(dca_ctx* ctx, const SampleGeom& sg, const PottsView<S>& pv, const SweepArgs& a)
{
    return with_qm(pv.q, [&](auto qm) { return dispatch_res<S, decltype(qm)::value, MODE>(ctx, sg, pv, a); });
}

// betas: the tempered sweep; else h0: the interpolated one; neither: the plain sweep under beta (MODE above)
template <typename S>
hipError_t dispatch_sweep(dca_ctx* ctx, const SampleGeom& sg, const PottsView<S>& pv, const SweepArgs& a)
{
    if (a.betas) return dispatch_qm<S, kSweepTempered>(ctx, sg, pv, a);
    if (a.h0) return dispatch_qm<S, kSweepInterp>(ctx, sg, pv, a);
    return dispatch_qm<S, kSweepPlain>(ctx, sg, pv, a);
}

}  // namespace

hipError_t dca_rows_to_sites(dca_ctx* ctx, const uint8_t* dRows, size_t ld, int n, int L, int nS, uint8_t* dSites)
{
    const size_t total = (size_t)L * nS;
    hipLaunchKernelGGL(rows_to_sites_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dRows, ld, n, L, nS, dSites);
    return hipGetLastError();
}

hipError_t dca_sites_to_rows(dca_ctx* ctx, const uint8_t* dSites, int n, int L, int nS, uint8_t* dRows)
{
    const size_t total = (size_t)n * L;
    hipLaunchKernelGGL(sites_to_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dSites, n, L, nS, dRows);
    return hipGetLastError();
}

// ---- device-resident chains (dca_internal.h): the sampler's state between calls
int dca_chains_start(dca_ctx* ctx, DcaChains* ch, int n, int L, int q, uint64_t seed, uint64_t first_chain, const uint8_t* initial,
                     int stride)
{
    *ch = DcaChains();
    ch->n = n; ch->L = L;
    ch->nS = (int)round_up((size_t)n, (size_t)stride);
    const size_t sites = (size_t)L * ch->nS;
    DevBuf<uint8_t> dRows;
    HIP_TRY_AS(ch->dState.alloc(sites, false), "sample");
    if (initial) {
        HIP_TRY_AS(dRows.alloc((size_t)n * L, false), "sample");
        HIP_TRY_AS(hipMemcpyAsync(dRows, initial, (size_t)n * L, hipMemcpyHostToDevice, ctx->stream), "sample");
        HIP_TRY_AS(dca_rows_to_sites(ctx, dRows, (size_t)L, n, L, ch->nS, ch->dState), "sample");
    } else {
        hipLaunchKernelGGL(initial_state_kernel, dim3((unsigned)((sites + 255) / 256)), dim3(256), 0, ctx->stream, n, L, q, ch->nS, seed,
                           first_chain, ch->dState.get());
    }
    HIP_TRY_AS(hipGetLastError(), "sample");
    return DCA_OK;
}

int dca_chains_sweeps(dca_ctx* ctx, const DcaChains& ch, const PottsSource& ps, int sweeps, uint64_t seed, uint64_t first_chain,
                      uint64_t first_sweep, double beta, const double* dBase, double bk, const double* dBetas)
{
    const hipError_t e = with_source_type(ps, [&](auto pv) {
        const SampleGeom sg = sample_geometry(pv.L, pv.q, sizeof(*pv.src));
        hipError_t e = hipSuccess;
        for (int t = 0; t < sweeps && e == hipSuccess; ++t) {       // one launch per sweep
            ScopedKernelClock kc(ctx, "sample");
            e = dispatch_sweep(ctx, sg, pv, SweepArgs{ch.dState, ch.nS, seed, first_chain, first_sweep + (uint64_t)t, beta, dBase, bk, dBetas});
        }
        return e;
    });
    if (e != hipSuccess) { dca_set_error("sample: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
    return DCA_OK;
}

int dca_chains_read(dca_ctx* ctx, const DcaChains& ch, uint8_t* out)
{
    const size_t total = (size_t)ch.n * ch.L;
    DevBuf<uint8_t> dRows;
    HIP_TRY_AS(dRows.alloc(total, false), "sample");
    HIP_TRY_AS(dca_sites_to_rows(ctx, ch.dState, ch.n, ch.L, ch.nS, dRows), "sample");
    HIP_TRY_AS(hipMemcpyAsync(out, dRows, total, hipMemcpyDeviceToHost, ctx->stream), "sample");
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), "sample");
    return DCA_OK;
}

int dca_potts_sample(dca_ctx* ctx, const PottsSource& ps, int n, int sweeps, uint64_t seed, uint64_t first_chain, uint64_t first_sweep,
                     double beta, const uint8_t* initial, uint8_t* out)
{
    if (n < 0 || sweeps < 0 || !(beta >= 0.0) || std::isinf(beta) || (n > 0 && !out)) {
        dca_set_error("sample: bad arguments (n %d, sweeps %d, beta %g)", n, sweeps, beta);
        return DCA_ERR_ARG;
    }
    if (n == 0) return DCA_OK;
    if (initial) DCA_TRY(dca_check_codes(initial, (size_t)n * ps.L, ps.q, "sample: initial "));
    DcaChains ch;
    DCA_TRY(dca_chains_start(ctx, &ch, n, ps.L, ps.q, seed, first_chain, initial));
    DCA_TRY(dca_chains_sweeps(ctx, ch, ps, sweeps, seed, first_chain, first_sweep, beta));
    return dca_chains_read(ctx, ch, out);
}

int dca_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    if (!ctr || !key || !out) { dca_set_error("philox: bad arguments"); return DCA_ERR_ARG; }
    philox4x32_10(ctr, key, out);
    return DCA_OK;
}
