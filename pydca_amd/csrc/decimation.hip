// Decimation of the couplings during Boltzmann learning (sparse bmDCA; DESIGN.md section 27, include/dca_hip.h) and the
// zero-sum gauge of the held model.
//
// dca_plm_bm_decimate, under the tag "bm_decimate":
//   bm_pairs_kernel<kBmScore>  (bm_pairs.h) the chains' pair histogram of a tile in LDS, every element scored from it;
//   dec_hist_kernel            eight passes, most significant byte first, over the scores read as 64-bit keys (a removed element's
//                              key is 2^64 - 1): the elements that share the key prefix found so far are counted by their next
//                              byte in an LDS histogram of uint32, the workgroups' histograms meet in 256 global uint64 counters
//                              by integer atomics; the host picks the byte that holds the remove-th smallest key;
//   dec_count_kernel           workgroup b counts the keys equal to the threshold key among its kDecChunk consecutive elements;
//   dec_scan_kernel            one workgroup: the exclusive scan of those counts;
//   dec_apply_kernel           workgroup b ranks its threshold keys by offset (a ballot per wave, the waves' counts in LDS) on top
//                              of its scan entry, and removes every element below the threshold and the threshold keys of rank <
//                              the number still needed: x = +0, mask = 0.  The removed scores above zero are appended to a list
//                              through one integer atomic per wave; the host sorts the list and sums it in ascending order.
// Which elements go depends on the keys and the offsets alone: no float atomics, and no launch geometry enters a result.
//
// dca_plm_zero_sum_gauge, under the tag "gauge":
//   gauge_pairs_kernel  one workgroup per pair i < j: the block in LDS as doubles, row means r(a) = (sum_b J(a,b)) / q and
//                       column means c(b) = (sum_a J(a,b)) / q (each sum from 0.0 in ascending index), m = (sum_a r(a)) / q,
//                       J'(a,b) = ((J(a,b) - r(a)) - c(b)) + m rounded once to the storage type; r(a) - m and c(b) - m go to the
//                       scratch [pair][2][q];
//   gauge_fields_kernel one workgroup per site i: t(a) = h_i(a) widened, then for j = 0 .. L-1, j != i in ascending order
//                       t(a) += scratch[pair(j,i)][1][a] (j < i) or scratch[pair(i,j)][0][a] (j > i); u = (sum_a t(a)) / q from 0.0
//                       in ascending a; h'_i(a) = t(a) - u rounded once to the storage type.
#include "bm_pairs.h"

#include <algorithm>
#include <vector>

namespace {

// ---------------------------------------------------------------- selection
__device__ __forceinline__ uint64_t dec_key(double d)
{
    const uint64_t k = (uint64_t)__double_as_longlong(d);
    return (k >> 63) ? ~(uint64_t)0 : k;          // -1.0: a removed element, after every active one
}

// hist[d] += the number of elements whose key has the bits above shift + 8 equal to prefix and the byte d at shift
__global__ __launch_bounds__(kDecThreads)
void dec_hist_kernel(const double* __restrict__ sc, size_t n, uint64_t prefix, int shift, unsigned long long* __restrict__ ghist)
{
    __shared__ uint32_t h[256];
    const int t = threadIdx.x;
    h[t] = 0u;
    __syncthreads();
    for (size_t e = (size_t)blockIdx.x * kDecThreads + t; e < n; e += (size_t)gridDim.x * kDecThreads) {
        const uint64_t k = dec_key(sc[e]);
        if (shift == 56 || (k >> (shift + 8)) == prefix) atomicAdd(&h[(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[t]) atomicAdd(&ghist[t], (unsigned long long)h[t]);
}

__global__ __launch_bounds__(kDecThreads)
void dec_count_kernel(const double* __restrict__ sc, size_t n, uint64_t T, unsigned long long* __restrict__ cnt)
{
    __shared__ uint32_t c;
    const int t = threadIdx.x;
    if (t == 0) c = 0u;
    __syncthreads();
    uint32_t mine = 0;
    const size_t base = (size_t)blockIdx.x * kDecChunk;
    for (int it = 0; it < kDecChunk / kDecThreads; ++it) {
        const size_t e = base + (size_t)it * kDecThreads + t;
        if (e < n && dec_key(sc[e]) == T) ++mine;
    }
    if (mine) atomicAdd(&c, mine);
    __syncthreads();
    if (t == 0) cnt[blockIdx.x] = c;
}

// one workgroup: cnt[0 .. G) becomes its exclusive scan; thread t owns the entries [t * per, (t + 1) * per)
__global__ __launch_bounds__(kDecThreads)
void dec_scan_kernel(unsigned long long* __restrict__ cnt, size_t G)
{
    __shared__ unsigned long long part[kDecThreads];
    const int t = threadIdx.x;
    const size_t per = (G + kDecThreads - 1) / kDecThreads;
    const size_t lo = (size_t)t * per < G ? (size_t)t * per : G, hi = lo + per < G ? lo + per : G;
    unsigned long long s = 0;
    for (size_t k = lo; k < hi; ++k) s += cnt[k];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < kDecThreads; ++k) { const unsigned long long v = part[k]; part[k] = run; run += v; }
    }
    __syncthreads();
    s = part[t];
    for (size_t k = lo; k < hi; ++k) { const unsigned long long v = cnt[k]; cnt[k] = s; s += v; }
}

template <typename S>
__global__ __launch_bounds__(kDecThreads)
void dec_apply_kernel(const double* __restrict__ sc, size_t n, uint64_t T, unsigned long long needEq,
                      const unsigned long long* __restrict__ tieBase, S* __restrict__ J, uint8_t* __restrict__ mask,
                      double* __restrict__ list, unsigned long long* __restrict__ listCount)
{
    __shared__ uint32_t wc[kDecThreads / 64];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    unsigned long long run = tieBase[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * kDecChunk;
    for (int it = 0; it < kDecChunk / kDecThreads; ++it) {
        const size_t e = base + (size_t)it * kDecThreads + t;
        const double d = e < n ? sc[e] : -1.0;
        const uint64_t k = dec_key(d);
        const bool tie = k == T;
        const unsigned long long bal = __ballot(tie);
        if (lane == 0) wc[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (int v = 0; v < kDecThreads / 64; ++v) { all += wc[v]; if (v < w) before += wc[v]; }
        const unsigned long long rank = run + before + (unsigned long long)__popcll(bal & below);
        const bool rem = e < n && (k < T || (tie && rank < needEq));
        run += all;
        __syncthreads();
        if (rem) { J[e] = (S)0; mask[e] = 0; }
        const bool app = rem && k != 0;
        const unsigned long long ab = __ballot(app);
        if (ab) {
            const int leader = __ffsll((long long)ab) - 1;
            unsigned long long pos = 0;
            if (lane == leader) pos = atomicAdd(listCount, (unsigned long long)__popcll(ab));
            pos = __shfl(pos, leader);
            if (app) list[pos + (unsigned long long)__popcll(ab & below)] = d;
        }
    }
}

template <typename S>
__global__ void mask_zero_kernel(const uint8_t* __restrict__ mask, size_t n, S* __restrict__ J)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x)
        if (!mask[e]) J[e] = (S)0;
}

size_t pair_elements(const BmRun* r) { return (size_t)r->L * (r->L - 1) / 2 * r->q * r->q; }

int ensure_mask(dca_ctx* ctx, BmRun* r, const char* who)
{
    if (r->dMask) return DCA_OK;
    const size_t n = pair_elements(r);
    HIP_TRY_AS_NOMEM(r->dMask.alloc(std::max<size_t>(n, 1), false), who);
    HIP_TRY_AS(hipMemsetAsync(r->dMask.get(), 1, std::max<size_t>(n, 1), ctx->stream), who);
    return DCA_OK;
}

// the remove smallest of the n keys: *T the largest of them, *needEq how many keys equal to *T are among them
int dec_select(dca_ctx* ctx, const double* dSc, size_t n, unsigned long long remove, unsigned long long* dHist, uint64_t* T,
               unsigned long long* needEq)
{
    static const char* who = "dca_plm_bm_decimate";
    unsigned long long h[256], remaining = remove;
    uint64_t prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        HIP_TRY_AS(hipMemsetAsync(dHist, 0, sizeof(h), ctx->stream), who);
        hipLaunchKernelGGL(dec_hist_kernel, dim3(dec_hist_blocks(n)), dim3(kDecThreads), 0, ctx->stream, dSc, n, prefix, shift, dHist);
        HIP_TRY_AS(hipGetLastError(), who);
        HIP_TRY_AS(hipMemcpyAsync(h, dHist, sizeof(h), hipMemcpyDeviceToHost, ctx->stream), who);
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
        unsigned long long cum = 0;
        int d = 0;
        for (; d < 256; ++d) {
            if (cum + h[d] >= remaining) break;
            cum += h[d];
        }
        if (d == 256) { dca_set_error("%s: the key histogram holds fewer than %llu elements", who, remove); return DCA_ERR_HIP; }
        remaining -= cum;
        prefix = (prefix << 8) | (uint64_t)d;
    }
    *T = prefix;
    *needEq = remaining;
    return DCA_OK;
}

template <typename S>
int decimate_t(dca_ctx* ctx, BmRun* r, S* x, long long remove, double* scores_out, dca_bm_decimation* info)
{
    static const char* who = "dca_plm_bm_decimate";
    const size_t n = pair_elements(r), Lq = (size_t)r->L * r->q;
    dca_bm_decimation out{r->active, remove, r->active - remove, 0.0, 0.0};
    DevBuf<double> dSc, dList;
    DevBuf<unsigned long long> dWork;            // 256 histogram counters, the list's length, then the chunks' counts
    const size_t G = dec_chunks(n);
    HIP_TRY_AS_NOMEM(dSc.alloc(std::max<size_t>(n, 1), false), who);
    std::vector<double> list;
    {
        ScopedKernelClock kc(ctx, "bm_decimate");
        if (n) HIP_TRY_AS((launch_pairs<S, kBmScore>(ctx, r, r->ch, x, r->dGi.get(), dSc.get())), who);
        if (remove > 0) {
            DCA_TRY(ensure_mask(ctx, r, who));
            HIP_TRY_AS_NOMEM(dWork.alloc(257 + G, false), who);
            HIP_TRY_AS_NOMEM(dList.alloc((size_t)remove, false), who);
            uint64_t T = 0;
            unsigned long long needEq = 0, listLen = 0;
            DCA_TRY(dec_select(ctx, dSc, n, (unsigned long long)remove, dWork, &T, &needEq));
            unsigned long long* dLen = dWork + 256;
            unsigned long long* dCnt = dWork + 257;
            HIP_TRY_AS(hipMemsetAsync(dLen, 0, sizeof(unsigned long long), ctx->stream), who);
            hipLaunchKernelGGL(dec_count_kernel, dim3(G), dim3(kDecThreads), 0, ctx->stream, dSc.get(), n, T, dCnt);
            hipLaunchKernelGGL(dec_scan_kernel, dim3(1), dim3(kDecThreads), 0, ctx->stream, dCnt, G);
            hipLaunchKernelGGL((dec_apply_kernel<S>), dim3(G), dim3(kDecThreads), 0, ctx->stream, dSc.get(), n, T, needEq, dCnt, x + Lq,
                               r->dMask.get(), dList.get(), dLen);
            HIP_TRY_AS(hipGetLastError(), who);
            r->active -= remove;                 // the apply pass is queued: the count follows the mask even if a read-back below fails
            HIP_TRY_AS(hipMemcpyAsync(&listLen, dLen, sizeof(listLen), hipMemcpyDeviceToHost, ctx->stream), who);
            HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
            memcpy(&out.threshold, &T, sizeof(double));
            if (info && listLen) {
                list.resize(listLen);
                HIP_TRY_AS(hipMemcpy(list.data(), dList, listLen * sizeof(double), hipMemcpyDeviceToHost), who);
            }
        }
    }
    if (!list.empty()) {
        std::sort(list.begin(), list.end());          // positive doubles: the order of their bit patterns
        double s = 0.0;
        for (double v : list) s += v;
        out.removed_sum = s;
    }
    if (scores_out) {
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
        if (n) HIP_TRY_AS(hipMemcpy(scores_out, dSc, n * sizeof(double), hipMemcpyDeviceToHost), who);
    }
    if (info) *info = out;
    return DCA_OK;
}

// ---------------------------------------------------------------- zero-sum gauge
template <typename S>
__global__ __launch_bounds__(kGaugeThreads)
void gauge_pairs_kernel(S* __restrict__ Jall, int L, int q, double* __restrict__ scratch)
{
    __shared__ double Jd[kGaugeMaxQ * kGaugeMaxQ], rm[kGaugeMaxQ], cm[kGaugeMaxQ], tm;       // q <= kGaugeMaxQ: gauge_t checks it
    const int i = blockIdx.y, j = blockIdx.x, t = threadIdx.x, qq = q * q;
    if (j <= i) return;
    const size_t pr = pair_index(L, i, j);
    S* blk = Jall + pr * qq;
    for (int e = t; e < qq; e += kGaugeThreads) Jd[e] = (double)blk[e];
    __syncthreads();
    if (t < q) {
        double s = 0.0;
        for (int b = 0; b < q; ++b) s += Jd[t * q + b];
        rm[t] = s / (double)q;
    } else if (t >= 64 && t < 64 + q) {
        double s = 0.0;
        for (int a = 0; a < q; ++a) s += Jd[a * q + (t - 64)];
        cm[t - 64] = s / (double)q;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int a = 0; a < q; ++a) s += rm[a];
        tm = s / (double)q;
    }
    __syncthreads();
    for (int e = t; e < qq; e += kGaugeThreads) {
        const int a = e / q, b = e - a * q;
        blk[e] = (S)(((Jd[e] - rm[a]) - cm[b]) + tm);
    }
    if (t < q) scratch[(pr * 2 + 0) * q + t] = rm[t] - tm;
    else if (t >= 64 && t < 64 + q) scratch[(pr * 2 + 1) * q + (t - 64)] = cm[t - 64] - tm;
}

template <typename S>
__global__ __launch_bounds__(64)
void gauge_fields_kernel(S* __restrict__ h, int L, int q, const double* __restrict__ scratch)
{
    __shared__ double v[kGaugeMaxQ], u;
    const int i = blockIdx.x, t = threadIdx.x;
    double acc = 0.0;
    if (t < q) {
        acc = (double)h[(size_t)i * q + t];
        for (int j = 0; j < L; ++j) {
            if (j == i) continue;
            const size_t at = j < i ? pair_index(L, j, i) * 2 + 1 : pair_index(L, i, j) * 2;
            acc += scratch[at * q + t];
        }
        v[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int a = 0; a < q; ++a) s += v[a];
        u = s / (double)q;
    }
    __syncthreads();
    if (t < q) h[(size_t)i * q + t] = (S)(acc - u);
}

template <typename S>
int gauge_t(dca_ctx* ctx, S* x, int L, int q)
{
    static const char* who = "dca_plm_zero_sum_gauge";
    static_assert(kGaugeMaxQ <= 64 && 64 + kGaugeMaxQ <= kGaugeThreads, "rows on the threads 0 .., columns on the threads 64 ..");
    if (q > kGaugeMaxQ) { dca_set_error("%s: q = %d above the %d states the kernels hold in LDS", who, q, kGaugeMaxQ); return DCA_ERR_ARG; }
    const size_t pairs = (size_t)L * (L - 1) / 2;
    DevBuf<double> dScratch;
    HIP_TRY_AS_NOMEM(dScratch.alloc(std::max<size_t>(pairs * 2 * q, 1), false), who);
    {
        ScopedKernelClock kc(ctx, "gauge");
        if (pairs) hipLaunchKernelGGL((gauge_pairs_kernel<S>), dim3(L, L), dim3(kGaugeThreads), 0, ctx->stream, x + (size_t)L * q, L, q, dScratch.get());
        hipLaunchKernelGGL((gauge_fields_kernel<S>), dim3(L), dim3(64), 0, ctx->stream, x, L, q, dScratch.get());
        HIP_TRY_AS(hipGetLastError(), who);
    }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}

}  // namespace

int dca_bm_decimate_impl(dca_ctx* ctx, void* dx, long long remove, double* scores_out, dca_bm_decimation* info)
{
    BmRun* r = ctx->bm;
    if (!r) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    if (r->t == 0) { dca_set_error("dca_plm_bm_decimate: no iteration has run yet"); return DCA_ERR_STATE; }
    if (remove < 0 || remove > r->active) {
        dca_set_error("dca_plm_bm_decimate: remove %lld outside [0, %lld active elements]", remove, r->active);
        return DCA_ERR_ARG;
    }
    return r->dtype == DCA_F32 ? decimate_t(ctx, r, static_cast<float*>(dx), remove, scores_out, info)
                               : decimate_t(ctx, r, static_cast<double*>(dx), remove, scores_out, info);
}

int dca_bm_set_mask_impl(dca_ctx* ctx, void* dx, const uint8_t* mask)
{
    static const char* who = "dca_plm_bm_set_mask";
    BmRun* r = ctx->bm;
    if (!r) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    if (!mask) { dca_set_error("%s: mask is NULL", who); return DCA_ERR_ARG; }
    const size_t n = pair_elements(r);
    long long active = 0;
    for (size_t e = 0; e < n; ++e) {
        if (mask[e] > 1) { dca_set_error("%s: mask[%zu] = %d is neither 0 nor 1", who, e, (int)mask[e]); return DCA_ERR_ARG; }
        active += mask[e];
    }
    DCA_TRY(ensure_mask(ctx, r, who));
    if (n == 0) return DCA_OK;
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    HIP_TRY_AS(hipMemcpy(r->dMask.get(), mask, n, hipMemcpyHostToDevice), who);
    r->active = active;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    const size_t Lq = (size_t)r->L * r->q;
    if (r->dtype == DCA_F32) hipLaunchKernelGGL((mask_zero_kernel<float>), dim3(blocks), dim3(256), 0, ctx->stream, r->dMask.get(), n, static_cast<float*>(dx) + Lq);
    else hipLaunchKernelGGL((mask_zero_kernel<double>), dim3(blocks), dim3(256), 0, ctx->stream, r->dMask.get(), n, static_cast<double*>(dx) + Lq);
    HIP_TRY_AS(hipGetLastError(), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}

int dca_bm_get_mask_impl(dca_ctx* ctx, uint8_t* out)
{
    static const char* who = "dca_plm_bm_get_mask";
    BmRun* r = ctx->bm;
    if (!r) { dca_set_error("dca_plm_bm_begin first"); return DCA_ERR_STATE; }
    if (!out) { dca_set_error("%s: out is NULL", who); return DCA_ERR_ARG; }
    const size_t n = pair_elements(r);
    if (!r->dMask) { memset(out, 1, n); return DCA_OK; }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    if (n) HIP_TRY_AS(hipMemcpy(out, r->dMask.get(), n, hipMemcpyDeviceToHost), who);
    return DCA_OK;
}

bool dca_bm_has_removed(const dca_ctx* ctx)
{
    const BmRun* r = ctx->bm;
    return r && r->dMask && r->active < (long long)pair_elements(r);
}

int dca_zero_sum_gauge_impl(dca_ctx* ctx, void* dx, int dtype)
{
    return dtype == DCA_F32 ? gauge_t(ctx, static_cast<float*>(dx), ctx->L, ctx->q) : gauge_t(ctx, static_cast<double*>(dx), ctx->L, ctx->q);
}
