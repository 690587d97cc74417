// Annealed importance sampling (Neal 2001) of the partition function Z = sum_s exp(E(s)) of a fitted Potts model (E as in
// energy.hip), along E_beta = E0 + beta * (E - E0), E0(s) = sum_i h0_i(s_i) the independent-site base model:
//   start      chain c draws x_0 from p0 exactly: per site p_a = exp(h0_i(a) - max_b h0_i(b)), the samplers' draw rule, Philox
//              counter (chain, 0, i, 2)  (ais_start_kernel, writes the site-major DcaChains state directly);
//   k = 1..K   log w += (beta_k - beta_{k-1}) * (E(x_{k-1}) - E0(x_{k-1}))  (energy.hip's pair kernels on the chain state, then
//              ais_weight_kernel, which forms E exactly as energy_finish_kernel does), then for k < K s Gibbs sweeps numbered
//              (k-1)s .. ks-1 under E_{beta_k} (sample.hip's sweep kernel, INTERP variant).
// Nothing leaves the device between temperatures; log w and the chains are copied to the host at the end.  Every chain's codes
// and weight depend on its chain number alone (no cross-chain sums), so any batch or split gives the same bits.
#include "dca_internal.h"

#include <cmath>

namespace {

constexpr int kAisStride = 128;                  // chain stride of the state: the energy kernels' multiple
constexpr int kAisMaxChains = 1 << 24;

// x_0 of chain first_chain + c at site s: st[s * nS + c]; chains past n get code 0 (swept, never read)
__global__ void ais_start_kernel(const double* __restrict__ h0, int n, int L, int q, int nS, uint64_t seed, uint64_t first_chain,
                                 uint8_t* __restrict__ st)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)L * nS) return;
    const int s = (int)(t / nS), c = (int)(t % nS);
    if (c >= n) { st[t] = 0; return; }
    const double* h = h0 + (size_t)s * q;
    double m = h[0];
    for (int a = 1; a < q; ++a) m = fmax(m, h[a]);
    double T = 0.0;
    for (int a = 0; a < q; ++a) T += exp(h[a] - m);
    const double r = philox_uniform(seed, first_chain + (uint64_t)c, 0, s, 2) * T;
    int pick = -1, last = 0;
    double cum = 0.0;
    for (int a = 0; a < q; ++a) {
        const double p = exp(h[a] - m);
        cum += p;
        if (pick < 0 && cum > r) pick = a;
        if (p > 0.0) last = a;
    }
    st[t] = (uint8_t)(pick < 0 ? last : pick);
}

// log w[c] += dbeta * (E(x) - E0(x)); E as energy_finish_kernel forms it from the fields and the slabs
template <typename S>
__global__ __launch_bounds__(256)
void ais_weight_kernel(const PottsView<S> pv, const uint8_t* __restrict__ QT, int n, int NqS, const double* __restrict__ slabs, int G,
                       const double* __restrict__ h0, double dbeta, double* __restrict__ logw)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    const int L = pv.L, q = pv.q;
    double e = 0.0;
    for (int i = 0; i < L; ++i) e += pv.field(i, QT[(size_t)i * NqS + c]);
    for (int g = 0; g < G; ++g) e += slabs[(size_t)g * NqS + c];
    double e0 = 0.0;
    for (int i = 0; i < L; ++i) e0 += h0[(size_t)i * q + QT[(size_t)i * NqS + c]];
    logw[c] = logw[c] + dbeta * (e - e0);
}

hipError_t weight_step(dca_ctx* ctx, const PottsSource& ps, const DcaChains& ch, double* dSlabs, int G, const double* dH0, double dbeta,
                       double* dLogW)
{
    ScopedKernelClock kc(ctx, "ais");
    hipError_t e = dca_energy_pairs_device(ctx, ps, ch.dState, ch.n, ch.nS, dSlabs);
    if (e != hipSuccess) return e;
    with_source_type(ps, [&](auto pv) {
        hipLaunchKernelGGL(ais_weight_kernel, dim3(ceil_div(ch.n, 256)), dim3(256), 0, ctx->stream, pv, ch.dState, ch.n, ch.nS, dSlabs, G,
                           dH0, dbeta, dLogW);
    });
    return hipGetLastError();
}

// the model's own fields h (L x q, gap included) on the host
int model_fields(dca_ctx* ctx, const PottsSource& ps, std::vector<double>& h)
{
    const int L = ps.L, q = ps.q;
    h.assign((size_t)L * q, 0.0);
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (ps.kind == 0 && ps.dtype == DCA_F32) {
        std::vector<float> f((size_t)L * q);
        if (e == hipSuccess) e = hipMemcpy(f.data(), ps.src, f.size() * sizeof(float), hipMemcpyDeviceToHost);
        for (size_t k = 0; k < f.size(); ++k) h[k] = (double)f[k];
    } else if (ps.kind == 0) {
        if (e == hipSuccess) e = hipMemcpy(h.data(), ps.src, h.size() * sizeof(double), hipMemcpyDeviceToHost);
    } else {
        std::vector<double> f((size_t)L * (q - 1));
        if (e == hipSuccess) e = hipMemcpy(f.data(), ps.mfh, f.size() * sizeof(double), hipMemcpyDeviceToHost);
        for (int i = 0; i < L; ++i)
            for (int a = 0; a < q - 1; ++a) h[(size_t)i * q + a] = f[(size_t)i * (q - 1) + a];
    }
    if (e != hipSuccess) { dca_set_error("ais: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
    return DCA_OK;
}

}  // namespace

int dca_potts_ais(dca_ctx* ctx, const PottsSource& ps, const dca_ais_args* args, double* log_weights_out, double* log_z0_out,
                  uint8_t* chains_out)
{
    const int L = ps.L, q = ps.q;
    if (!args || !log_weights_out) { dca_set_error("ais: args or log_weights_out is NULL"); return DCA_ERR_ARG; }
    const int n = args->chains, K = args->temperatures, s = args->sweeps_per_temperature;
    if (n < 1 || n > kAisMaxChains || K < 1 || s < 0) {
        dca_set_error("ais: bad counts (chains %d, temperatures %d, sweeps_per_temperature %d)", n, K, s);
        return DCA_ERR_ARG;
    }
    std::vector<double> beta((size_t)K + 1);
    if (args->betas) {
        for (int k = 0; k <= K; ++k) {
            beta[k] = args->betas[k];
            if (!std::isfinite(beta[k]) || (k > 0 && !(beta[k] > beta[k - 1]))) {
                dca_set_error("ais: betas must be finite and strictly increasing (beta[%d] = %g)", k, beta[k]);
                return DCA_ERR_ARG;
            }
        }
        if (beta[0] != 0.0 || beta[K] != 1.0) {
            dca_set_error("ais: the schedule must run from 0 to 1 (%g .. %g)", beta[0], beta[K]);
            return DCA_ERR_ARG;
        }
    } else {
        for (int k = 0; k <= K; ++k) beta[k] = (double)k / (double)K;
    }
    std::vector<double> h0;
    if (args->base_fields) {
        h0.assign(args->base_fields, args->base_fields + (size_t)L * q);
        for (size_t k = 0; k < h0.size(); ++k)
            if (!std::isfinite(h0[k])) { dca_set_error("ais: base field %zu is not finite", k); return DCA_ERR_ARG; }
    } else {
        DCA_TRY(model_fields(ctx, ps, h0));
    }
    if (log_z0_out) *log_z0_out = dca_ais_log_z0(h0.data(), L, q);

    DcaChains ch;
    ch.n = n; ch.L = L; ch.nS = (int)round_up((size_t)n, kAisStride);
    const int G = dca_energy_slab_count(ps);
    DevBuf<double> dH0, dLogW, dSlabs;
    const size_t sites = (size_t)L * ch.nS;
    HIP_TRY_AS(ch.dState.alloc(sites, false), "ais");
    HIP_TRY_AS(dH0.alloc(h0.size(), false), "ais");
    HIP_TRY_AS(dLogW.alloc((size_t)ch.nS, false), "ais");
    HIP_TRY_AS(dSlabs.alloc((size_t)G * ch.nS, false), "ais");
    HIP_TRY_AS(hipMemcpyAsync(dH0, h0.data(), h0.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "ais");
    HIP_TRY_AS(hipMemsetAsync(dLogW, 0, (size_t)ch.nS * sizeof(double), ctx->stream), "ais");
    {
        ScopedKernelClock kc(ctx, "ais");
        hipLaunchKernelGGL(ais_start_kernel, dim3((unsigned)((sites + 255) / 256)), dim3(256), 0, ctx->stream, dH0.get(), n, L, q, ch.nS,
                           args->seed, args->first_chain, ch.dState.get());
        HIP_TRY_AS(hipGetLastError(), "ais");
    }
    for (int k = 1; k <= K; ++k) {
        HIP_TRY_AS(weight_step(ctx, ps, ch, dSlabs, G, dH0, beta[k] - beta[k - 1], dLogW), "ais");
        if (k < K && s > 0)
            DCA_TRY(dca_chains_sweeps(ctx, ch, ps, s, args->seed, args->first_chain, (uint64_t)(k - 1) * (uint64_t)s, 1.0, dH0, beta[k]));
    }
    HIP_TRY_AS(hipMemcpyAsync(log_weights_out, dLogW, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "ais");
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), "ais");
    return chains_out ? dca_chains_read(ctx, ch, chains_out) : DCA_OK;
}

// log Z0 = sum_i (m_i + log sum_a exp(h0_i(a) - m_i)), ascending i and a
double dca_ais_log_z0(const double* h0, int L, int q)
{
    double z = 0.0;
    for (int i = 0; i < L; ++i) {
        const double* h = h0 + (size_t)i * q;
        double m = h[0];
        for (int a = 1; a < q; ++a) m = std::fmax(m, h[a]);
        double t = 0.0;
        for (int a = 0; a < q; ++a) t += std::exp(h[a] - m);
        z += m + std::log(t);
    }
    return z;
}

int dca_ais_estimate(const double* log_weights, int n, double log_z0, double* log_z, double* ess, double* stderr_log_z)
{
    if (!log_weights || n < 1 || !std::isfinite(log_z0)) { dca_set_error("ais estimate: bad arguments (n %d)", n); return DCA_ERR_ARG; }
    double m = log_weights[0];
    for (int c = 0; c < n; ++c) {
        if (!std::isfinite(log_weights[c])) { dca_set_error("ais estimate: log weight %d is not finite", c); return DCA_ERR_ARG; }
        m = std::fmax(m, log_weights[c]);
    }
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < n; ++c) s1 += std::exp(log_weights[c] - m);
    for (int c = 0; c < n; ++c) s2 += std::exp(2.0 * (log_weights[c] - m));
    if (log_z) *log_z = ((log_z0 + m) + std::log(s1)) - std::log((double)n);
    if (ess) *ess = s1 * s1 / s2;
    if (stderr_log_z) *stderr_log_z = std::sqrt(std::fmax(0.0, s2 / (s1 * s1) - 1.0 / (double)n));
    return DCA_OK;
}
