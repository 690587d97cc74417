// One- and two-site frequencies of a sequence set and their comparison with the alignment's (dca_sequence_statistics,
// dca_alignment_statistics).  The pieces exist: the alignment's weighted full-q frequencies come from a private mf engine exactly
// as a Boltzmann-learning run obtains its data statistics (dca_mf_engine_bm_freqs with lambda = 0), the set's counts from the
// statistics kernels of boltzmann.hip without their update (exact integer LDS histograms, one division by nq).  New here is
//   set_compare_kernel   one workgroup per site i: the q terms of f_i and the (L - 1 - i) q^2 terms of f_ij and c_ij of the pairs
//                        (i, j > i), which are contiguous in pair order.  Thread t walks the elements t, t + 256, ... in
//                        ascending order, the 256 partials meet in a fixed tree, the twelve results go to slab i;
//   set_reduce_kernel    one workgroup: thread t reduces the slabs t, t + 256, ... in ascending order, the same tree.
// Per quantity Sxx = sum (x - mu)^2, Syy, Sxy and max |x - y| with the ANALYTIC means mu = 1/q, 1/q^2, 0 (each block of f sums
// to 1, each block of c to 0): no sum of squares minus squared sum, so nothing cancels.  Double, no contraction, no float
// atomics; the order is fixed by (L, q).
#include "dca_internal.h"

#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kVals = 12;          // quantity k (0 f_i, 1 f_ij, 2 c_ij): Sxx, Syy, Sxy, max |x - y| at 4 k ..

__device__ __forceinline__ void tree_reduce(double (*red)[kThreads], const double* v, int t)
{
#pragma unroll
    for (int s = 0; s < kVals; ++s) red[s][t] = v[s];
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int s = 0; s < kVals; ++s) red[s][t] = (s & 3) == 3 ? fmax(red[s][t], red[s][t + w]) : red[s][t] + red[s][t + w];
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void add_term(double* v, double dx, double dy, double diff)
{
    v[0] += dx * dx; v[1] += dy * dy; v[2] += dx * dy; v[3] = fmax(v[3], fabs(diff));
}

// x: the alignment's fi / fij, y: the set's
__global__ __launch_bounds__(kThreads)
void set_compare_kernel(const double* __restrict__ xi, const double* __restrict__ xij, const double* __restrict__ yi,
                        const double* __restrict__ yij, int L, int q, double* __restrict__ slab)
{
    __shared__ double red[kVals][kThreads];
    const int i = blockIdx.x, t = threadIdx.x, qq = q * q;
    const double mu1 = 1.0 / (double)q, mu2 = 1.0 / (double)qq;
    double v[kVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (t < q) {
        const double x = xi[(size_t)i * q + t], y = yi[(size_t)i * q + t];
        add_term(v, x - mu1, y - mu1, x - y);
    }
    const int count = (L - 1 - i) * qq;            // < 2^31: L q^2 is
    const size_t base = i < L - 1 ? pair_index(L, i, i + 1) * qq : 0;
    for (int e = t; e < count; e += kThreads) {
        const int jj = e / qq, ab = e - jj * qq;
        const int j = i + 1 + jj, a = ab / q, b = ab - a * q;
        const double x = xij[base + e], y = yij[base + e];
        add_term(v + 4, x - mu2, y - mu2, x - y);
        const double cx = x - xi[(size_t)i * q + a] * xi[(size_t)j * q + b];
        const double cy = y - yi[(size_t)i * q + a] * yi[(size_t)j * q + b];
        add_term(v + 8, cx, cy, cx - cy);
    }
    tree_reduce(red, v, t);
    if (t < kVals) slab[(size_t)i * kVals + t] = red[t][0];
}

__global__ __launch_bounds__(kThreads)
void set_reduce_kernel(const double* __restrict__ slab, int L, double* __restrict__ out)
{
    __shared__ double red[kVals][kThreads];
    const int t = threadIdx.x;
    double v[kVals] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = t; k < L; k += kThreads) {
#pragma unroll
        for (int s = 0; s < kVals; ++s) v[s] = (s & 3) == 3 ? fmax(v[s], slab[(size_t)k * kVals + s]) : v[s] + slab[(size_t)k * kVals + s];
    }
    tree_reduce(red, v, t);
    if (t < kVals) out[t] = red[t][0];
}

}  // namespace

int dca_set_statistics_impl(dca_ctx* ctx, const uint8_t* Q, int nq, double* fi_out, double* fij_out, dca_set_comparison* cmp_out)
{
    const int L = ctx->L, q = ctx->q;
    const size_t Lq = (size_t)L * q, pairs = (size_t)L * (L - 1) / 2, nij = pairs * q * q;
    if (Q) DCA_TRY(dca_check_codes(Q, (size_t)nq * L, q, "dca_sequence_statistics: "));
    const bool wantX = !Q || cmp_out;
    static const char* who = "dca_sequence_statistics";
    DevBuf<double> dXi, dXij, dYi, dYij, dSlab;
    DcaChains ch;
    if ((wantX && (dXi.alloc(Lq, false) != hipSuccess || dXij.alloc(nij, false) != hipSuccess)) ||
        (Q && (dYi.alloc(Lq, false) != hipSuccess || dYij.alloc(nij, false) != hipSuccess)) ||
        (cmp_out && dSlab.alloc(((size_t)L + 1) * kVals, false) != hipSuccess)) {
        dca_set_error("%s: out of device memory", who);
        return DCA_ERR_NOMEM;
    }
    if (wantX) {
        // a private engine, so the context's own mf state (counts, correlation matrix, couplings, hooks) stays as it is
        MfEngine* m = dca_make_mf_engine(ctx);
        if (!m) return DCA_ERR_NOMEM;
        const int rc = dca_mf_engine_bm_freqs(m, 0.0, dXi, dXij);
        dca_free_mf_engine(m);
        DCA_TRY(rc);
    }
    if (Q) {
        // the set as site-major device codes, the layout the statistics kernels count
        DCA_TRY(dca_chains_start(ctx, &ch, nq, L, q, 0, 0, Q));
        HIP_TRY_AS(dca_bm_count_chains(ctx, ch, q, dYi, dYij), who);
    }
    if (cmp_out) {
        ScopedKernelClock kc(ctx, "set_compare");
        hipLaunchKernelGGL(set_compare_kernel, dim3(L), dim3(kThreads), 0, ctx->stream, dXi.get(), dXij.get(), dYi.get(), dYij.get(), L, q,
                           dSlab.get());
        hipLaunchKernelGGL(set_reduce_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, dSlab.get(), L, dSlab + (size_t)L * kVals);
        HIP_TRY_AS(hipGetLastError(), who);
    }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    if (fi_out) HIP_TRY_AS(hipMemcpy(fi_out, (Q ? dYi : dXi).get(), Lq * sizeof(double), hipMemcpyDeviceToHost), who);
    if (fij_out) HIP_TRY_AS(hipMemcpy(fij_out, (Q ? dYij : dXij).get(), nij * sizeof(double), hipMemcpyDeviceToHost), who);
    double r[kVals];
    if (cmp_out) HIP_TRY_AS(hipMemcpy(r, dSlab + (size_t)L * kVals, sizeof(r), hipMemcpyDeviceToHost), who);
    if (cmp_out) {
        for (int k = 0; k < 3; ++k) {
            const double sxx = r[4 * k], syy = r[4 * k + 1], sxy = r[4 * k + 2];
            const double vv = sxx * syy;
            cmp_out->sxx[k] = sxx; cmp_out->syy[k] = syy; cmp_out->sxy[k] = sxy;
            cmp_out->max_abs_diff[k] = r[4 * k + 3];
            cmp_out->pearson[k] = vv > 0.0 ? sxy / std::sqrt(vv) : 0.0;
            cmp_out->slope[k] = sxx > 0.0 ? sxy / sxx : 0.0;
            cmp_out->terms[k] = k == 0 ? (double)Lq : (double)nij;
        }
    }
    return DCA_OK;
}
