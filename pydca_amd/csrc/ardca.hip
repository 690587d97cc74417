// Autoregressive Potts model (arDCA): fit, exact log-probabilities and ancestral sampling, all in float64.
//   P(s) = prod_l P(s_l | s_<l),  P(s_l = b | s_<l) = exp u_l(b) / sum_c exp u_l(c),  u_l(b) = h_l(b) + sum_{k<l} J_kl(s_k, b)
// with x in the plm layout (dca_plm_num_params): fields L*q first, then the q x q blocks of the pairs (k < l) in pair order,
// element a*q + b = J_kl(a at the earlier site k, b at the later site l).  Sites are in model order (the alignment's columns).
//
// Objective (include/dca_hip.h): f(x) = -sum_n W_n sum_l log P(s_nl | s_n,<l) + lambda_h sum h^2 + lambda_J sum J^2, W_n = w_n / sum w.
// One evaluation runs the sequences through in passes (bounded device scratch); per pass:
//   dca_rows_to_sites site-major copy of the pass's codes, QT[l * NpS + n]
//   ar_logits_kernel  ("ar_logits") u_l, log-softmax, the site values log P(s_nl | .) and the residual R_nl(b) = W_n (P_nl(b) - [s_nl = b]):
//                     site_conditionals.h's body (which states the summation order: h_l first, then k ascending) with the policy below
//   dca_site_finish   log P(s_n) = sum_l site (ascending l); ar_wsum_kernel: F_pass = sum_n W_n log P(s_n) (fixed tree)
//   ar_field_kernel / ar_grad_kernel ("ar_grad")  G_h[l][b] = sum_n R_nl(b), G_kl[a][b] = sum_n [s_nk = a] R_nl(b), ascending n
// and the pass results are added in ascending pass order; then g += 2 lambda x and fx = -(sum of F_pass) + lambda_h |h|^2 + lambda_J |J|^2.
// No atomics anywhere: every element is summed in an order fixed by (N, L, q, pass size), so repeated calls give the same bits.
//
// Optimiser: L-BFGS (m = 5) on device vectors with the More-Thuente line search (strong Wolfe conditions) that plmDCA runs
// too: more_thuente.h, with up to 20 evaluations per search here; the elementwise vector kernels are vec_kernels.h's.  Only
// scalars cross to the host.
//
// Sampler ("ar_sample"): chain c visits sites 0 .. L-1 once and draws s_l with sample.hip's rule at beta = 1 from
// U = Philox(seed; chain, 0, site, 3).  DESIGN.md section 16 has the geometry and the measured numbers.
#include "site_conditionals.h"
#include "ar_plan.h"
#include "more_thuente.h"
#include "vec_kernels.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

namespace {

constexpr size_t kAPassBudget = 1ull << 30;        // device scratch of one pass
constexpr int kSSlices = 4;                        // sampler: lanes per chain (k = w mod 4)
constexpr int kSChainsPerWave = 64 / kSSlices;
constexpr int kDotBlocks = 256;

// site l of the autoregressive model: the earlier sites k < l; the block of the pair (k, l) holds J_kl(a, b) as the term needs
// it, so nothing is transposed.  With R (L x NpS x q) and W (the pass's normalised weights) the epilogue writes the residual
// R_nl(b) = W_n (P_nl(b) - [s_nl = b]).
template <int QM>
struct ArPolicy {
    const double* x;
    int L, q, l, NpS;
    const double* W;
    double* R;
    __device__ __forceinline__ int neighbours() const { return l; }
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ double load(int k, int a, int b) const { return x[(size_t)L * q + pair_index(L, k, l) * (size_t)(q * q) + (a * q + b)]; }
    __device__ __forceinline__ int lds_pos(int, int a, int b) const { return a * QM + b; }
    __device__ __forceinline__ double field(int b) const { return x[(size_t)l * q + b]; }
    __device__ __forceinline__ void epilogue(int n, const double* u, double m, double lz, int sl) const
    {
        if (!R) return;
        const double w = W[n];
        double* r = R + ((size_t)l * NpS + n) * q;
#pragma unroll
        for (int b = 0; b < QM; ++b)
            if (b < q) r[b] = w * (exp((u[b] - m) - lz) - (b == sl ? 1.0 : 0.0));
    }
};

// grid (ceil(nq / 512), L): blockIdx.y = L - 1 - l, so the sites with the most terms are dispatched first.  LDS
// site_lds<double, QM>(q).  QT, site and cond as site_conditional_body takes them; R and W as the policy does.
template <int QM>
__global__ __launch_bounds__(kSiteThreads)
void ar_logits_kernel(const double* __restrict__ x, int L, int q, const uint8_t* __restrict__ QT, int nq, int NpS,
                      const double* __restrict__ W, double* __restrict__ site, double* __restrict__ R, double* __restrict__ cond)
{
    const int l = L - 1 - (int)blockIdx.y;
    const ArPolicy<QM> P{x, L, q, l, NpS, W, R};
    site_conditional_body<double, QM>(P, l, blockIdx.x * kSiteSeqBlock, L, q, QT, nq, NpS, site, cond);
}

// out[0] = sum_n W_n logp_n: thread t sums n = t, t + 256, ... ascending, then a fixed tree over the 256 partials
__global__ __launch_bounds__(256)
void ar_wsum_kernel(const double* __restrict__ logp, const double* __restrict__ W, int nq, double* __restrict__ out)
{
    __shared__ double part[256];
    double s = 0.0;
    for (int n = threadIdx.x; n < nq; n += 256) s += W[n] * logp[n];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = part[0];
}

// field gradient of one pass: g[l * q + b] (+)= sum_n R_nl(b), ascending n
__global__ __launch_bounds__(256)
void ar_field_kernel(const double* __restrict__ R, int L, int q, int nq, int NpS, double* __restrict__ g, int accumulate)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= L * q) return;
    const int l = t / q, b = t - l * q;
    const double* r = R + (size_t)l * NpS * q + b;
    double s = 0.0;
    for (int n = 0; n < nq; ++n) s += r[(size_t)n * q];
    g[t] = accumulate ? g[t] + s : s;
}

// coupling gradient of one pass.  grid (ceil((L - 1) / KC), L - 1): blockIdx.y = L - 1 - l (heavy sites first), blockIdx.x the
// chunk of KC earlier sites k.  Thread e < kc * q owns the column b = e % q of the block of k = k0 + e / q: G[kk][a][b] in LDS,
// which it alone updates, for every a.  Tiles of 64 sequences (their residual rows R_nl(.) and the chunk's codes s_nk) are
// staged in LDS; within a tile n ascends, so every element is summed over n in ascending order.  LDS: KC q^2 + 64 q doubles,
// then KC x 64 code bytes.
__global__ __launch_bounds__(kGMaxThreads)
void ar_grad_kernel(const uint8_t* __restrict__ QT, const double* __restrict__ R, int L, int q, int nq, int NpS, int KC,
                    double* __restrict__ g, int accumulate)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ar_gsmem[];
    const int l = L - 1 - (int)blockIdx.y;
    const int k0 = blockIdx.x * KC;
    if (k0 >= l) return;
    const int kc = min(KC, l - k0);
    const int qq = q * q;
    double* G = reinterpret_cast<double*>(ar_gsmem);
    double* Rt = G + (size_t)KC * qq;
    uint8_t* Ct = reinterpret_cast<uint8_t*>(Rt + kGTile * q);
    const int tid = threadIdx.x;
    const bool own = tid < kc * q;
    const int kk = own ? tid / q : 0, b = own ? tid - (tid / q) * q : 0;
    double* Gc = G + (size_t)kk * qq + b;
    if (own)
        for (int a = 0; a < q; ++a) Gc[a * q] = 0.0;
    const double* Rl = R + (size_t)l * NpS * q;
    for (int n0 = 0; n0 < nq; n0 += kGTile) {
        const int tn = min(kGTile, nq - n0);
        __syncthreads();
        for (int e = tid; e < tn * q; e += blockDim.x) Rt[e] = Rl[(size_t)n0 * q + e];
        for (int e = tid; e < kc * kGTile; e += blockDim.x) Ct[e] = QT[(size_t)(k0 + e / kGTile) * NpS + n0 + (e % kGTile)];
        __syncthreads();
        if (own) {
            const uint8_t* cs = Ct + kk * kGTile;
            for (int j = 0; j < tn; ++j) Gc[(int)cs[j] * q] += Rt[j * q + b];
        }
    }
    if (!own) return;
    double* dst = g + (size_t)L * q + pair_index(L, k0 + kk, l) * (size_t)qq + b;
    for (int a = 0; a < q; ++a) dst[(size_t)a * q] = accumulate ? dst[(size_t)a * q] + Gc[a * q] : Gc[a * q];
}

// g[i] += 2 lambda x[i]  (lambda_h on the L q fields, lambda_J on the couplings)
__global__ void ar_reg_kernel(double* __restrict__ g, const double* __restrict__ x, size_t P, size_t Lq, double lh2, double lJ2)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= P) return;
    g[i] = g[i] + (i < Lq ? lh2 : lJ2) * x[i];
}

// part[block] = sum of a[i] * b[i] over i = gid, gid + stride, ... (ascending), then a fixed tree in the block
__global__ __launch_bounds__(256)
void ar_dot_kernel(const double* __restrict__ a, const double* __restrict__ b, size_t n, double* __restrict__ part)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s += a[i] * b[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// out[0] = the kDotBlocks partials summed by a fixed tree
__global__ __launch_bounds__(kDotBlocks)
void ar_dot_final_kernel(const double* __restrict__ part, double* __restrict__ out)
{
    __shared__ double sh[kDotBlocks];
    sh[threadIdx.x] = part[threadIdx.x];
    __syncthreads();
    for (int w = kDotBlocks / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0];
}

// y = a - b
__global__ void ar_diff_kernel(double* __restrict__ y, const double* __restrict__ a, const double* __restrict__ b, size_t n)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < n) y[i] = a[i] - b[i];
}

// Ancestral sampling.  A wave holds 16 chains x 4 lanes; lane w of a chain sums the terms k = w (mod 4), k < l, ascending k
// (lane 0 starting from h_l), the partials join in lane 0 in ascending w and lane 0 draws; the pick is broadcast and stored in
// LDS by the lane that will read it (codes[(k / 4) * 64 + lane] holds s_k of that lane's chain for its k = w mod 4).
// grid: ceil(n / 16) one-wave workgroups.  out: n x L codes (rows).
template <int QM>
__global__ __launch_bounds__(64)
void ar_sample_kernel(const double* __restrict__ x, int L, int q, int n, uint64_t seed, uint64_t first_chain, uint8_t* __restrict__ out)
{
    extern __shared__ uint8_t ar_codes[];
    const int lane = threadIdx.x, w = lane & (kSSlices - 1), base = lane & ~(kSSlices - 1);
    const int c = blockIdx.x * kSChainsPerWave + lane / kSSlices;
    const uint64_t chain = first_chain + (uint64_t)c;
    const int qq = q * q;
    const double* J = x + (size_t)L * q;
    for (int l = 0; l < L; ++l) {
        double u[QM];
#pragma unroll
        for (int b = 0; b < QM; ++b) u[b] = (w == 0 && b < q) ? x[(size_t)l * q + b] : 0.0;
        for (int k = w; k < l; k += kSSlices) {
            const int a = ar_codes[(k / kSSlices) * 64 + lane];
            const double* row = J + pair_index(L, k, l) * (size_t)qq + (size_t)a * q;
#pragma unroll
            for (int b = 0; b < QM; ++b) if (b < q) u[b] += row[b];
        }
#pragma unroll
        for (int s = 1; s < kSSlices; ++s) {
#pragma unroll
            for (int b = 0; b < QM; ++b) {
                const double v = __shfl(u[b], base + s);
                if (w == 0) u[b] += v;
            }
        }
        int pick = 0;
        if (w == 0) {
            double m = u[0];
#pragma unroll
            for (int b = 1; b < QM; ++b) if (b < q) m = fmax(m, u[b]);
            double T = 0.0;
#pragma unroll
            for (int b = 0; b < QM; ++b) {
                u[b] = b < q ? exp(u[b] - m) : 0.0;          // sample.hip's exp(beta * (u - m)) at beta = 1
                T += u[b];
            }
            const double r = philox_uniform(seed, chain, 0, l, 3) * T;
            int last = 0;
            double cum = 0.0;
            pick = -1;
#pragma unroll
            for (int b = 0; b < QM; ++b) {
                if (b < q) {
                    cum += u[b];
                    if (pick < 0 && cum > r) pick = b;
                    if (u[b] > 0.0) last = b;
                }
            }
            if (pick < 0) pick = last;
        }
        pick = __shfl(pick, base);
        if ((l & (kSSlices - 1)) == w) ar_codes[(l / kSSlices) * 64 + lane] = (uint8_t)pick;
        if (w == 0 && c < n) out[(size_t)c * L + l] = (uint8_t)pick;
    }
}

// the logits kernel on the context's stream (callers clock it as "ar_logits")
hipError_t launch_logits(dca_ctx* ctx, const double* x, int L, int q, const uint8_t* QT, int nq, int NpS, const double* W,
                         double* site, double* R, double* cond)
{
    return with_qm(q, [&](auto qm) {
        auto kern = ar_logits_kernel<decltype(qm)::value>;
        const size_t lds = site_lds<double, decltype(qm)::value>(q);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(ceil_div(nq, kSiteSeqBlock), L), dim3(kSiteThreads), lds, ctx->stream, x, L, q, QT, nq, NpS, W, site, R, cond);
        return hipGetLastError();
    });
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

struct ArEngine {
    dca_ctx* ctx;
    int N = 0, L = 0, q = 0;
    size_t P = 0;
    bool configured = false;
    double lh = 0.0, lJ = 0.0;
    DevBuf<double> dx, dg, dW;
    // passes of the fit
    int pass = 0, NpS = 0, npass = 0;
    DevBuf<uint8_t> dQT;
    DevBuf<double> dSite, dR, dLogp, dPassF;
    // scalars: dot partials, results
    DevBuf<double> dPart, dOut;
    // optimiser
    DevBuf<double> dxp, dgp, dd, dS[5], dY[5];
    int evals = 0;

    explicit ArEngine(dca_ctx* c) : ctx(c) {}
    void free_pass() { dQT.reset(); dSite.reset(); dR.reset(); dLogp.reset(); dPassF.reset(); }

    int fail(hipError_t e, const char* what)
    {
        dca_set_error("arDCA %s: %s", what, hipGetErrorString(e));
        return DCA_ERR_HIP;
    }

    // x exists (zeros) for the context's (L, q)
    int ensure_x()
    {
        if (dx && L == ctx->L && q == ctx->q) return DCA_OK;
        dx.reset(); dg.reset();
        L = ctx->L; q = ctx->q;
        P = dca_plm_num_params(L, q);
        HIP_TRY(dx.alloc(P));
        HIP_TRY(dg.alloc(P));
        HIP_TRY(hipMemsetAsync(dx, 0, P * sizeof(double), ctx->stream));
        HIP_TRY(hipMemsetAsync(dg, 0, P * sizeof(double), ctx->stream));
        if (!dPart) HIP_TRY(dPart.alloc(kDotBlocks));
        if (!dOut) HIP_TRY(dOut.alloc(16));
        return DCA_OK;
    }

    int configure(double lambda_h, double lambda_J)
    {
        configured = false;
        DCA_TRY(ensure_x());
        N = ctx->N;
        lh = lambda_h; lJ = lambda_J;
        // W_n = w_n / sum w (the context's Meff: the ascending sum of the weights)
        std::vector<double> w(N);
        HIP_TRY(hipMemcpy(w.data(), ctx->dWd, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        const double meff = ctx->meff;
        if (!(meff > 0.0)) { dca_set_error("arDCA: the weights sum to %g", meff); return DCA_ERR_ARG; }
        for (double& v : w) v = v / meff;
        HIP_TRY(dW.alloc((size_t)N));
        HIP_TRY(hipMemcpy(dW, w.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
        free_pass();
        pass = site_pass_size(N, (size_t)L * (1 + sizeof(double) + (size_t)q * sizeof(double)) + sizeof(double), kAPassBudget, "DCA_AR_PASS", 1);
        NpS = (int)round_up((size_t)pass, kSiteSeqBlock);
        npass = ceil_div(N, pass);
        HIP_TRY(dQT.alloc((size_t)L * NpS, false));
        HIP_TRY(dSite.alloc((size_t)L * NpS, false));
        HIP_TRY(dR.alloc((size_t)L * NpS * q, false));
        HIP_TRY(dLogp.alloc((size_t)NpS, false));
        HIP_TRY(dPassF.alloc((size_t)npass, false));
        configured = true;
        return DCA_OK;
    }

    // dot products a_i . b_i into dOut[slot_i], then one copy of nout values to the host
    hipError_t dot_async(const double* a, const double* b, size_t n, int slot)
    {
        hipLaunchKernelGGL(ar_dot_kernel, dim3(kDotBlocks), dim3(256), 0, ctx->stream, a, b, n, dPart);
        hipLaunchKernelGGL(ar_dot_final_kernel, dim3(1), dim3(kDotBlocks), 0, ctx->stream, dPart, dOut + slot);
        return hipGetLastError();
    }
    int read_out(int count, double* host)
    {
        HIP_TRY(hipMemcpyAsync(host, dOut, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DCA_OK;
    }
    double dot(const double* a, const double* b, int* rc)
    {
        double v = 0.0;
        hipError_t e = dot_async(a, b, P, 0);
        if (e != hipSuccess) { *rc = fail(e, "dot"); return 0.0; }
        *rc = read_out(1, &v);
        return v;
    }

    // fx and g at dx.  With d: also g.d; always |g|^2 and |x|^2.  One round trip.
    int evaluate(double* fx, const double* d, double* gd, double* gg, double* xx)
    {
        const size_t Lq = (size_t)L * q;
        hipError_t e = hipSuccess;
        const ArGradPlan gp = ar_grad_plan(q);
        const int KC = gp.KC, gthreads = gp.threads;
        const size_t glds = gp.lds;
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(ar_grad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)glds);
        for (int p = 0; p < npass && e == hipSuccess; ++p) {
            const int first = p * pass, nq = std::min(pass, N - first);
            e = dca_rows_to_sites(ctx, ctx->dX + (size_t)first * ctx->Ls, (size_t)ctx->Ls, nq, L, NpS, dQT);
            if (e == hipSuccess) {
                ScopedKernelClock kc(ctx, "ar_logits");
                e = launch_logits(ctx, dx, L, q, dQT, nq, NpS, dW + first, dSite, dR, nullptr);
            }
            if (e == hipSuccess) e = dca_site_finish(ctx, dSite, L, nq, NpS, dLogp, nullptr);
            if (e != hipSuccess) break;
            hipLaunchKernelGGL(ar_wsum_kernel, dim3(1), dim3(256), 0, ctx->stream, dLogp, dW + first, nq, dPassF + p);
            {
                ScopedKernelClock kc(ctx, "ar_grad");
                hipLaunchKernelGGL(ar_field_kernel, dim3(blocks_of(Lq)), dim3(256), 0, ctx->stream, dR, L, q, nq, NpS, dg, p > 0 ? 1 : 0);
                hipLaunchKernelGGL(ar_grad_kernel, dim3(ceil_div(L - 1, KC), L - 1), dim3(gthreads), glds, ctx->stream, dQT, dR, L, q, nq,
                                   NpS, KC, dg, p > 0 ? 1 : 0);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(ar_reg_kernel, dim3(blocks_of(P)), dim3(256), 0, ctx->stream, dg, dx, P, Lq, 2.0 * lh, 2.0 * lJ);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = dot_async(dx, dx, Lq, 0);
        if (e == hipSuccess) e = dot_async(dx + Lq, dx + Lq, P - Lq, 1);
        if (e == hipSuccess) e = dot_async(dg, dg, P, 2);
        if (e == hipSuccess && d) e = dot_async(dg, d, P, 3);
        if (e != hipSuccess) return fail(e, "evaluation");
        std::vector<double> pf(npass);
        HIP_TRY(hipMemcpyAsync(pf.data(), dPassF, (size_t)npass * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        double s[4] = {0, 0, 0, 0};
        DCA_TRY(read_out(d ? 4 : 3, s));
        double F = 0.0;
        for (int p = 0; p < npass; ++p) F += pf[p];
        *fx = -F + (lh * s[0] + lJ * s[1]);
        if (xx) *xx = s[0] + s[1];
        if (gg) *gg = s[2];
        if (gd) *gd = d ? s[3] : 0.0;
        ++evals;
        return DCA_OK;
    }

    int gradient(double* fx_out)
    {
        double fx = 0.0;
        DCA_TRY(evaluate(&fx, nullptr, nullptr, nullptr, nullptr));
        if (fx_out) *fx_out = fx;
        return DCA_OK;
    }

    // elementwise vector kernels (vec_kernels.h) over the P parameters
    dim3 vgrid() const { return dim3(std::min(blocks_of(P), (unsigned)kVecBlocks)); }
    void vneg(double* d, const double* g) { hipLaunchKernelGGL(vec_neg_kernel<double>, vgrid(), dim3(kVecThreads), 0, ctx->stream, d, g, P); }
    void vstep(double* x, const double* xp, double t, const double* d) { hipLaunchKernelGGL(vec_step_kernel<double>, vgrid(), dim3(kVecThreads), 0, ctx->stream, x, xp, t, d, P); }
    void vaxpy(double* y, double a, const double* x) { hipLaunchKernelGGL(vec_axpy_kernel<double>, vgrid(), dim3(kVecThreads), 0, ctx->stream, y, a, x, P); }
    void vscale(double* y, double a) { hipLaunchKernelGGL(vec_scale_kernel<double>, vgrid(), dim3(kVecThreads), 0, ctx->stream, y, a, P); }

    // More-Thuente line search (more_thuente.h) from xp along dd (x = xp + stp d): > 0 evaluations on success, < 0 failure;
    // *rc runtime errors
    int line_search(double* stp, double* f, double dginit, double* gg, double* xx, int* rc)
    {
        const MtParams params{1e-4, 0.9, 1e-16, 1e-20, 1e20, 20};
        return mt_line_search(params, stp, f, &dginit, false, [&](double t, double* ft, double* dgt) {
            vstep(dx, dxp, t, dd);
            return evaluate(ft, dd, dgt, gg, xx);
        }, rc);
    }

    int fit(int max_iterations, double epsilon, dca_ar_stats* st)
    {
        constexpr int M = 5;
        const auto t0 = std::chrono::steady_clock::now();
        if (!dxp) {
            for (DevBuf<double>* b : {&dxp, &dgp, &dd}) HIP_TRY(b->alloc(P));
            for (int i = 0; i < M; ++i) {
                HIP_TRY(dS[i].alloc(P));
                HIP_TRY(dY[i].alloc(P));
            }
        }
        evals = 0;
        double fx = 0.0, gg = 0.0, xx = 0.0;
        DCA_TRY(evaluate(&fx, nullptr, nullptr, &gg, &xx));
        int status = DCA_AR_MAX_ITERATIONS, k = 0, stored = 0, newest = -1;
        double ys[M] = {}, alpha[M] = {};
        vneg(dd, dg);
        double dginit = -gg;
        double step = gg > 0.0 ? 1.0 / std::sqrt(gg) : 1.0;
        int rc = DCA_OK;
        for (;;) {
            if (std::sqrt(gg) <= epsilon * std::max(1.0, std::sqrt(xx))) { status = DCA_AR_CONVERGED; break; }
            if (k >= max_iterations) { status = DCA_AR_MAX_ITERATIONS; break; }
            dx.swap(dxp);
            dg.swap(dgp);
            const double fprev = fx, ggprev = gg, xxprev = xx;
            // the search rejects 0 < dginit, as the reference's does, and would take a zero slope; none reaches it: dginit
            // is -gg, where gg = 0 has converged above (epsilon >= 0), or the g.d that the reset below found < 0
            const int ls = line_search(&step, &fx, dginit, &gg, &xx, &rc);
            if (rc) return rc;
            if (ls < 0) {                                     // back to the last accepted point
                dx.swap(dxp);
                dg.swap(dgp);
                fx = fprev; gg = ggprev; xx = xxprev;
                status = DCA_AR_LINE_SEARCH_FAILED;
                break;
            }
            ++k;
            if (std::sqrt(gg) <= epsilon * std::max(1.0, std::sqrt(xx))) { status = DCA_AR_CONVERGED; break; }
            if (k >= max_iterations) { status = DCA_AR_MAX_ITERATIONS; break; }
            // the new pair s = x - xp, y = g - gp
            const int slot = (newest + 1) % M;
            hipLaunchKernelGGL(ar_diff_kernel, dim3(blocks_of(P)), dim3(256), 0, ctx->stream, dS[slot], dx, dxp, P);
            hipLaunchKernelGGL(ar_diff_kernel, dim3(blocks_of(P)), dim3(256), 0, ctx->stream, dY[slot], dg, dgp, P);
            HIP_TRY(dot_async(dY[slot], dS[slot], P, 0));
            HIP_TRY(dot_async(dY[slot], dY[slot], P, 1));
            double sy[2];
            DCA_TRY(read_out(2, sy));
            if (sy[0] > 0.0) {                                // the Wolfe conditions make y.s > 0; a pair without it is dropped
                newest = slot;
                ys[slot] = sy[0];
                stored = std::min(stored + 1, M);
            }
            // two-loop recursion: d = -H g
            vneg(dd, dg);
            for (int i = 0, j = newest; i < stored; ++i, j = (j + M - 1) % M) {
                const double sd = dot(dS[j], dd, &rc);
                if (rc) return rc;
                alpha[j] = sd / ys[j];
                vaxpy(dd, -alpha[j], dY[j]);
            }
            if (stored > 0 && sy[0] > 0.0)
                vscale(dd, sy[0] / sy[1]);
            for (int i = 0, j = (newest + M - stored + 1) % M; i < stored; ++i, j = (j + 1) % M) {
                const double yd = dot(dY[j], dd, &rc);
                if (rc) return rc;
                vaxpy(dd, alpha[j] - yd / ys[j], dS[j]);
            }
            dginit = dot(dg, dd, &rc);
            if (rc) return rc;
            if (!(dginit < 0.0)) {                            // not a descent direction: restart from steepest descent
                vneg(dd, dg);
                dginit = -gg;
                stored = 0;
                step = 1.0 / std::sqrt(gg);
            } else {
                step = 1.0;
            }
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (st) {
            st->status = status; st->iterations = k; st->evaluations = evals;
            st->fx = fx; st->gnorm = std::sqrt(gg);
            st->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        return DCA_OK;
    }

    int log_probabilities(const uint8_t* X, int n, double* logp_out, double* site_out, double* cond_out)
    {
        const SitePasses sp{kAPassBudget, "DCA_AR_PASS", 1, "ar_logits"};
        const hipError_t e = dca_site_passes(ctx, sp, L, q, X, n, logp_out, site_out, cond_out, [&](const uint8_t* dQT, int nq, int NqS, double* dSite, double* dCond) {
            return launch_logits(ctx, dx, L, q, dQT, nq, NqS, nullptr, dSite, nullptr, dCond);
        });
        if (e != hipSuccess) return fail(e, "log-probabilities");
        return DCA_OK;
    }

    // cond_l(b) of ONE sequence (host codes, model order) into dCond (device, L*q): log_probabilities with n = 1, so the values
    // are bit for bit its cond (the wild-type pass of ar_epistasis.hip)
    int conditionals_of(const uint8_t* row, double* dCond)
    {
        double logp = 0.0;
        std::vector<double> cond((size_t)L * q);
        DCA_TRY(log_probabilities(row, 1, &logp, nullptr, cond.data()));
        HIP_TRY(hipMemcpy(dCond, cond.data(), cond.size() * sizeof(double), hipMemcpyHostToDevice));
        return DCA_OK;
    }

    int sample(int n, uint64_t seed, uint64_t first_chain, uint8_t* out)
    {
        const size_t lds = (size_t)64 * ceil_div(L, kSSlices);
        if (lds > 160 * 1024) { dca_set_error("arDCA sample: L = %d exceeds the sampler's %d sites", L, 160 * 1024 / 64 * kSSlices); return DCA_ERR_ARG; }
        static const char* who = "arDCA sample";
        DevBuf<uint8_t> dOutRows;
        HIP_TRY_AS(dOutRows.alloc((size_t)n * L, false), who);
        {
            ScopedKernelClock kc(ctx, "ar_sample");
            auto go = [&](auto kern) {
                HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                hipLaunchKernelGGL(kern, dim3(ceil_div(n, kSChainsPerWave)), dim3(64), lds, ctx->stream, dx.get(), L, q, n, seed, first_chain,
                                   dOutRows.get());
                return hipGetLastError();
            };
            HIP_TRY_AS(with_qm(q, [&](auto qm) { return go(ar_sample_kernel<decltype(qm)::value>); }), who);
        }
        HIP_TRY_AS(hipMemcpyAsync(out, dOutRows, (size_t)n * L, hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
        return DCA_OK;
    }
};

ArEngine* dca_make_ar_engine(dca_ctx* ctx) { return new ArEngine(ctx); }
bool dca_ar_engine_model(ArEngine* e, const double** dx, int* L, int* q)
{
    if (!e || !e->dx) return false;
    *dx = e->dx; *L = e->L; *q = e->q;
    return true;
}
int dca_ar_engine_conditionals(ArEngine* e, const uint8_t* row, double* dCond) { return e->conditionals_of(row, dCond); }
void dca_free_ar_engine(ArEngine* e) { delete e; }
void dca_ar_engine_weights_changed(ArEngine* e) { if (e) e->configured = false; }

// ---- C-ABI (include/dca_hip.h)
extern "C" {

static int ar_need_engine(dca_ctx* ctx, bool need_configured)
{
    if (!ctx) { dca_set_error("null context"); return DCA_ERR_ARG; }
    if (!ctx->ar || !ctx->ar->dx) { dca_set_error("dca_ar_configure first"); return DCA_ERR_STATE; }
    if (need_configured && !ctx->ar->configured) { dca_set_error("dca_ar_configure first (the weights changed since)"); return DCA_ERR_STATE; }
    hipSetDevice(ctx->device);
    return DCA_OK;
}

int dca_ar_configure(dca_ctx* ctx, double lambda_h, double lambda_J)
{
    if (!ctx) { dca_set_error("null context"); return DCA_ERR_ARG; }
    if (!(lambda_h >= 0.0) || !(lambda_J >= 0.0) || std::isinf(lambda_h) || std::isinf(lambda_J)) {
        dca_set_error("dca_ar_configure: lambda_h %g, lambda_J %g must be finite and >= 0", lambda_h, lambda_J);
        return DCA_ERR_ARG;
    }
    if (!ctx->dX) { dca_set_error("dca_set_msa first"); return DCA_ERR_STATE; }
    if (ctx->L < 2) { dca_set_error("the model needs an alignment of at least two sites"); return DCA_ERR_STATE; }
    if (!ctx->have_weights) { dca_set_error("dca_compute_weights or dca_set_weights first"); return DCA_ERR_STATE; }
    hipSetDevice(ctx->device);
    if (!ctx->ar) ctx->ar = dca_make_ar_engine(ctx);
    return ctx->ar->configure(lambda_h, lambda_J);
}

size_t dca_ar_num_params(int L, int q) { return dca_plm_num_params(L, q); }

int dca_ar_init_x(dca_ctx* ctx)
{
    DCA_TRY(ar_need_engine(ctx, false));
    HIP_TRY(hipMemsetAsync(ctx->ar->dx, 0, ctx->ar->P * sizeof(double), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DCA_OK;
}

int dca_ar_set_x(dca_ctx* ctx, const double* x)
{
    DCA_TRY(ar_need_engine(ctx, false));
    if (!x) { dca_set_error("dca_ar_set_x: x is NULL"); return DCA_ERR_ARG; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->ar->dx, x, ctx->ar->P * sizeof(double), hipMemcpyHostToDevice));
    return DCA_OK;
}

int dca_ar_get_x(dca_ctx* ctx, double* x)
{
    DCA_TRY(ar_need_engine(ctx, false));
    if (!x) { dca_set_error("dca_ar_get_x: x is NULL"); return DCA_ERR_ARG; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(x, ctx->ar->dx, ctx->ar->P * sizeof(double), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_ar_gradient(dca_ctx* ctx, double* fx_out)
{
    DCA_TRY(ar_need_engine(ctx, true));
    return ctx->ar->gradient(fx_out);
}

int dca_ar_get_g(dca_ctx* ctx, double* g)
{
    DCA_TRY(ar_need_engine(ctx, false));
    if (!g) { dca_set_error("dca_ar_get_g: g is NULL"); return DCA_ERR_ARG; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(g, ctx->ar->dg, ctx->ar->P * sizeof(double), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_ar_fit(dca_ctx* ctx, int max_iterations, double epsilon, dca_ar_stats* stats_out)
{
    if (max_iterations < 0 || !(epsilon >= 0.0) || std::isinf(epsilon)) {
        dca_set_error("dca_ar_fit: max_iterations %d must be >= 0 and epsilon %g finite and >= 0", max_iterations, epsilon);
        return DCA_ERR_ARG;
    }
    DCA_TRY(ar_need_engine(ctx, true));
    return ctx->ar->fit(max_iterations, epsilon, stats_out);
}

int dca_ar_log_probabilities(dca_ctx* ctx, const uint8_t* X, int n, double* logp, double* site, double* cond)
{
    if (n < 0 || (n > 0 && (!X || !logp))) { dca_set_error("dca_ar_log_probabilities: bad arguments"); return DCA_ERR_ARG; }
    DCA_TRY(ar_need_engine(ctx, false));
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(X, (size_t)n * ctx->ar->L, ctx->ar->q, ""));
    return ctx->ar->log_probabilities(X, n, logp, site, cond);
}

int dca_ar_sample(dca_ctx* ctx, int n, uint64_t seed, uint64_t first_chain, uint8_t* out)
{
    if (n < 0 || (n > 0 && !out)) { dca_set_error("dca_ar_sample: bad arguments (n %d)", n); return DCA_ERR_ARG; }
    DCA_TRY(ar_need_engine(ctx, false));
    if (n == 0) return DCA_OK;
    return ctx->ar->sample(n, seed, first_chain, out);
}

int dca_ar_release(dca_ctx* ctx)
{
    if (!ctx) { dca_set_error("null context"); return DCA_ERR_ARG; }
    if (!ctx->ar) return DCA_OK;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { dca_set_error("dca_ar_release: stream synchronisation failed"); return DCA_ERR_HIP; }
    dca_free_ar_engine(ctx->ar);
    ctx->ar = nullptr;
    return DCA_OK;
}

}  // extern "C"
