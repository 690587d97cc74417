// Boltzmann machine learning (bmDCA) of the plm parameter vector x (fields L*q, then the q x q blocks of the pairs i < j in
// pair order): gradient ascent on the L2-regularised log-likelihood, with the model's one- and two-site frequencies estimated
// from n persistent Gibbs chains that stay on the device for the whole run (include/dca_hip.h).
//
// One iteration: k sweeps of the chains (sample.hip, tag "sample"), then under the tag "bm_stats"
//   bm_fields_kernel  one workgroup per site: integer counts c_i(a) in LDS, g_i = c_i / n, field update, max |f^_i - g_i|;
//   bm_pairs_kernel   (bm_pairs.h) one workgroup per TB x TB tile of site pairs: each chain's codes of the tile's 2 TB sites are read once
//                     into registers and counted into an LDS histogram of uint32 (ds_add_u32, exact); the same workgroup then
//                     reads f^_ij and theta, writes theta', and writes its max |f^_ij - g_ij| and its five Pearson sums to a
//                     slab of its own;
//   bm_record_kernel  one workgroup: the slabs and the field maxima reduced in a fixed order, the record of the iteration.
// No float atomics.  Every sum runs in double in an order fixed by (L, q): thread e of a tile walks the tile's elements
// e, e + 256, ... in ascending order, the 256 partials meet in a fixed tree; the record kernel does the same over the slabs.
#include "bm_pairs.h"

#include <memory>

namespace {

// grid L.  g_i(a) = c_i(a) / n; UPDATE: fields updated, epsPart[i] = max_a |f^_i(a) - g_i(a)|
template <typename S, bool UPDATE>
__global__ __launch_bounds__(kBmThreads)
void bm_fields_kernel(const uint8_t* __restrict__ st, int nS, int n, int q, const double* __restrict__ fi, double* __restrict__ gi,
                      S* __restrict__ x, double eta, double mu, double* __restrict__ epsPart)
{
    __shared__ uint32_t hist[32];
    const int i = blockIdx.x, t = threadIdx.x;
    if (t < 32) hist[t] = 0u;
    __syncthreads();
    const uint8_t* col = st + (size_t)i * nS;
    for (int c = t; c < n; c += kBmThreads) atomicAdd(&hist[col[c]], 1u);
    __syncthreads();
    if (t != 0) return;
    double m = 0.0;
    for (int a = 0; a < q; ++a) {
        const double g = (double)hist[a] / (double)n;
        gi[(size_t)i * q + a] = g;
        if (UPDATE) {
            const double d = fi[(size_t)i * q + a] - g;
            m = fmax(m, fabs(d));
            bm_update(x + (size_t)i * q + a, d, eta, mu);
        }
    }
    if (UPDATE) epsPart[i] = m;
}

// one workgroup: thread t reduces the slabs t, t + 256, ... (and the field maxima likewise) in ascending order, the 256
// partials meet in a fixed tree; rec = (eps_h, eps_J, pearson) with M = pairs * q^2 values:
//   cov = Sdm / M - (Sd / M)(Sm / M), vd = Sdd / M - (Sd / M)^2, vm = Smm / M - (Sm / M)^2, pearson = cov / sqrt(vd vm) (0 if vd vm <= 0)
__global__ __launch_bounds__(kBmThreads)
void bm_record_kernel(const double* __restrict__ slab, int tiles, const double* __restrict__ epsPart, int L, double M, double* __restrict__ rec)
{
    __shared__ double red[kBmSums + 1][kBmThreads];
    const int t = threadIdx.x;
    double v[kBmSums + 1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = t; k < tiles; k += kBmThreads) {
        v[0] = fmax(v[0], slab[(size_t)k * kBmSums]);
#pragma unroll
        for (int s = 1; s < kBmSums; ++s) v[s] += slab[(size_t)k * kBmSums + s];
    }
    for (int i = t; i < L; i += kBmThreads) v[kBmSums] = fmax(v[kBmSums], epsPart[i]);
#pragma unroll
    for (int s = 0; s <= kBmSums; ++s) red[s][t] = v[s];
    __syncthreads();
    for (int s = kBmThreads / 2; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] = fmax(red[0][t], red[0][t + s]);
#pragma unroll
            for (int k = 1; k < kBmSums; ++k) red[k][t] += red[k][t + s];
            red[kBmSums][t] = fmax(red[kBmSums][t], red[kBmSums][t + s]);
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double md = red[1][0] / M, mm = red[2][0] / M;
    const double cov = red[5][0] / M - md * mm;
    const double vd = red[3][0] / M - md * md, vm = red[4][0] / M - mm * mm;
    const double vv = vd * vm;
    rec[0] = red[kBmSums][0];
    rec[1] = red[0][0];
    rec[2] = vv > 0.0 ? cov / sqrt(vv) : 0.0;
}

// the statistics of the chains ch into gi (and gij); UPDATE: with the update of x and the record written to dRec[slot]
template <typename S, bool UPDATE>
hipError_t bm_stats(dca_ctx* ctx, const BmRun* r, const DcaChains& ch, S* x, int slot, double* gi, double* gij)
{
    ScopedKernelClock kc(ctx, "bm_stats");
    hipLaunchKernelGGL((bm_fields_kernel<S, UPDATE>), dim3(r->L), dim3(kBmThreads), 0, ctx->stream, ch.dState.get(), ch.nS, ch.n, r->q,
                       r->dFi.get(), gi, x, r->eta_h, r->mu_h, r->dEps.get());
    HIP_PASS(hipGetLastError());
    HIP_PASS((launch_pairs<S, UPDATE ? kBmUpdate : kBmCount>(ctx, r, ch, x, gi, gij)));
    if (UPDATE) {
        const double M = (double)((size_t)r->L * (r->L - 1) / 2) * (double)(r->q * r->q);
        hipLaunchKernelGGL(bm_record_kernel, dim3(1), dim3(kBmThreads), 0, ctx->stream, r->dSlab.get(), r->tiles, r->dEps.get(), r->L, M,
                           r->dRec + (size_t)3 * slot);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t dca_bm_count_chains(dca_ctx* ctx, const DcaChains& ch, int q, double* dGi, double* dGij)
{
    BmRun r;                               // the geometry for the launchers above; it owns nothing
    r.L = ch.L; r.q = q;
    r.tb = bm_tile(q);
    r.nb = ceil_div(ch.L, r.tb);
    return bm_stats<float, false>(ctx, &r, ch, nullptr, 0, dGi, dGij);
}

namespace {

bool finite_nonneg(double v) { return v >= 0.0 && std::isfinite(v); }

// the x a run learns, as the sampler's source
PottsSource bm_model(const BmRun* r, const void* dx) { return PottsSource{dx, 0, r->dtype, nullptr, r->L, r->q, 0}; }

}  // namespace

void dca_bm_free(dca_ctx* ctx)
{
    if (!ctx->bm) return;
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    delete ctx->bm;
    ctx->bm = nullptr;
}

int dca_bm_begin_impl(dca_ctx* ctx, void* dx, int dtype, const dca_bm_args* a)
{
    dca_bm_free(ctx);
    const int L = ctx->L, q = ctx->q;
    if (a->chains < 1 || a->sweeps < 1 || a->equilibration_sweeps < 0 || !finite_nonneg(a->eta_h) || !finite_nonneg(a->eta_J) ||
        !finite_nonneg(a->mu_h) || !finite_nonneg(a->mu_J) || !(a->pseudocount >= 0.0 && a->pseudocount < 1.0)) {
        dca_set_error("dca_plm_bm_begin: bad arguments (chains %d, sweeps %d, equilibration %d, eta %g / %g, mu %g / %g, pseudocount %g)",
                      a->chains, a->sweeps, a->equilibration_sweeps, a->eta_h, a->eta_J, a->mu_h, a->mu_J, a->pseudocount);
        return DCA_ERR_ARG;
    }
    if (a->initial) DCA_TRY(dca_check_codes(a->initial, (size_t)a->chains * L, q, "dca_plm_bm_begin: initial "));
    std::unique_ptr<BmRun> r(new BmRun());
    r->L = L; r->q = q; r->dtype = dtype;
    r->k = a->sweeps; r->E = a->equilibration_sweeps; r->seed = a->seed;
    r->eta_h = a->eta_h; r->eta_J = a->eta_J; r->mu_h = a->mu_h; r->mu_J = a->mu_J;
    r->tb = bm_tile(q);
    r->nb = ceil_div(L, r->tb);
    r->tiles = r->nb * (r->nb + 1) / 2;
    r->active = (long long)L * (L - 1) / 2 * q * q;
    const size_t Lq = (size_t)L * q, pairs = (size_t)L * (L - 1) / 2;
    if (r->dFi.alloc(Lq, false) != hipSuccess || r->dFij.alloc(pairs * q * q, false) != hipSuccess || r->dGi.alloc(Lq) != hipSuccess ||
        r->dEps.alloc((size_t)L) != hipSuccess || r->dSlab.alloc((size_t)r->tiles * kBmSums) != hipSuccess) {
        dca_set_error("dca_plm_bm_begin: out of device memory");
        return DCA_ERR_NOMEM;
    }
    // data statistics from the mf engine's weighted counts: a private engine, so the context's own mf state stays as it is
    {
        MfEngine* m = dca_make_mf_engine(ctx);
        const int rc = dca_mf_engine_bm_freqs(m, a->pseudocount, r->dFi, r->dFij);
        dca_free_mf_engine(m);
        DCA_TRY(rc);
    }
    DCA_TRY(dca_chains_start(ctx, &r->ch, a->chains, L, q, a->seed, 0, a->initial));
    DCA_TRY(dca_chains_sweeps(ctx, r->ch, bm_model(r.get(), dx), r->E, r->seed, 0, 0, 1.0));
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { dca_set_error("dca_plm_bm_begin: stream failed"); return DCA_ERR_HIP; }
    ctx->bm = r.release();
    return DCA_OK;
}

int dca_bm_iterate_impl(dca_ctx* ctx, void* dx, int iterations, dca_bm_record* records_out)
{
    BmRun* r = ctx->bm;
    if (!r) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    if (iterations < 0) { dca_set_error("dca_plm_bm_iterate: iterations %d < 0", iterations); return DCA_ERR_ARG; }
    if (iterations == 0) return DCA_OK;
    if (iterations > r->recCap) {
        r->recCap = 0;
        HIP_TRY(r->dRec.alloc((size_t)iterations * 3));
        r->recCap = iterations;
    }
    for (int it = 0; it < iterations; ++it) {
        const uint64_t first = (uint64_t)r->E + (uint64_t)r->t * (uint64_t)r->k;
        DCA_TRY(dca_chains_sweeps(ctx, r->ch, bm_model(r, dx), r->k, r->seed, 0, first, 1.0));
        const hipError_t e = r->dtype == DCA_F32 ? bm_stats<float, true>(ctx, r, r->ch, static_cast<float*>(dx), it, r->dGi, nullptr)
                                                 : bm_stats<double, true>(ctx, r, r->ch, static_cast<double*>(dx), it, r->dGi, nullptr);
        if (e != hipSuccess) { dca_set_error("dca_plm_bm_iterate: %s", hipGetErrorString(e)); return DCA_ERR_HIP; }
        ++r->t;
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (records_out) HIP_TRY(hipMemcpy(records_out, r->dRec, (size_t)iterations * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return DCA_OK;
}

int dca_bm_freqs_impl(dca_ctx* ctx, int which, double* fi_out, double* fij_out)
{
    BmRun* r = ctx->bm;
    if (which != 0 && which != 1) { dca_set_error("dca_plm_bm_freqs: which must be 0 or 1"); return DCA_ERR_ARG; }
    if (!r) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    const size_t Lq = (size_t)r->L * r->q, nij = (size_t)r->L * (r->L - 1) / 2 * r->q * r->q;
    if (which == 0) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (fi_out) HIP_TRY(hipMemcpy(fi_out, r->dFi, Lq * sizeof(double), hipMemcpyDeviceToHost));
        if (fij_out) HIP_TRY(hipMemcpy(fij_out, r->dFij, nij * sizeof(double), hipMemcpyDeviceToHost));
        return DCA_OK;
    }
    if (r->t == 0) { dca_set_error("dca_plm_bm_freqs: no iteration has run yet"); return DCA_ERR_STATE; }
    // the chains are those of the last iteration's statistics (its sweeps came before them): count them again, x untouched
    static const char* who = "dca_plm_bm_freqs";
    DevBuf<double> dG;
    HIP_TRY(dG.alloc(std::max<size_t>(nij, 1), false));
    HIP_TRY_AS((r->dtype == DCA_F32 ? bm_stats<float, false>(ctx, r, r->ch, nullptr, 0, r->dGi, dG)
                                    : bm_stats<double, false>(ctx, r, r->ch, nullptr, 0, r->dGi, dG)), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    if (fi_out) HIP_TRY_AS(hipMemcpy(fi_out, r->dGi, Lq * sizeof(double), hipMemcpyDeviceToHost), who);
    if (fij_out) HIP_TRY_AS(hipMemcpy(fij_out, dG, nij * sizeof(double), hipMemcpyDeviceToHost), who);
    return DCA_OK;
}

int dca_bm_chains_impl(dca_ctx* ctx, uint8_t* out)
{
    if (!ctx->bm) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    if (!out) { dca_set_error("dca_plm_bm_chains: out is NULL"); return DCA_ERR_ARG; }
    return dca_chains_read(ctx, ctx->bm->ch, out);
}
