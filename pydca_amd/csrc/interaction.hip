// Inter-protein interaction energies of a Potts model on a concatenated alignment (dca_plm_interaction_energies,
// dca_mf_interaction_energies).  Sites [0, LA) are protein A, sites [LA, L) protein B.  The model
// arrives as a PottsSource and is read through potts_coupling (potts_source.h).
//
// The rule (include/dca_hip.h): every term widened to double, no contraction,
//   phi_m(j, b) = sum over i = 0 .. LA-1, ascending, of Jt_{i, LA+j}(a^m_i, b)      one sequential double sum from 0.0
//   E(m, n)     = sum over j = 0 .. LB-1, ascending, of phi_m(j, b^n_j)             one sequential double sum from 0.0
// with Jt the stored block (gauge 0) or its zero-sum form over all q states, kept in double (gauge 1).
//
// Two kernels (geometry: interaction_plan.h):
//   cross_fields_kernel   the geometry of cond_fields_kernel (sample_conditional.hip; its staging, potts_rows.h, is not shared:
//                         see below): grid (blocks of 256 A-sequences,
//                         B-site j), thread = A-sequence with QM double accumulators, the blocks (i, LA + j) of CJ A-sites
//                         staged through LDS in double-buffered chunks (the next chunk's loads are in flight in registers while
//                         the current one is summed).  The blocks are staged as doubles, row a holding Jt(a, .) padded to QM
//                         values; with gauge 1 the shift is applied in place while the block sits in LDS.  Output
//                         phi[(m * LB + j) * q + b].  Doubles staged untransposed and a gauge shift in LDS: a body of its own.
//   cross_energy_kernel   one workgroup per item (a run of A-rows and a window over each row's B-partners); the rows' phi
//                         sits in LDS a chunk of sites at a time, the B-codes are read site-major as in energy.hip, pair
//                         p of the item is summed by thread p % 256 in slot p / 256; the running sums stay in registers across
//                         the chunks, so the ascending-j order holds.
// No atomics, no cross-lane sums: E(m, n) has the same bits in any grouping, batch, block split or call.
#include "dca_internal.h"
#include "interaction_plan.h"

#include <type_traits>

namespace {

static_assert(kXFieldRegs == 8 && kXThreads == 256, "cross_fields_kernel's register chunk");

// f(std::integral_constant<int, cross_qm(q)>)
template <typename F>
auto with_cross_qm(int q, F&& f)
{
    switch (cross_qm(q)) {
    case 8: return f(std::integral_constant<int, 8>());
    case 24: return f(std::integral_constant<int, 24>());
    default: return f(std::integral_constant<int, 32>());
    }
}

// registers <- the blocks (i, jB) of the A-sites i = i0 .. i0 + CJ - 1 (those below LA): element e of the chunk is value
// e % q^2 = a * q + b of block e / q^2 and goes to dst = kk * blk + a * QM + b
template <typename S, int QM>
__device__ __forceinline__ void cross_chunk_load(const S* __restrict__ src, int kind, int L, int q, int ld, int LA, int jB, int i0,
                                                 int chunkVals, double (&val)[kXFieldRegs], int (&dst)[kXFieldRegs])
{
    const int qq = q * q, blk = q * QM;
#pragma unroll
    for (int r = 0; r < kXFieldRegs; ++r) {
        const int e = threadIdx.x + r * kXThreads;
        dst[r] = -1;
        if (e >= chunkVals) continue;
        const int kk = e / qq, el = e - kk * qq;
        const int i = i0 + kk;
        if (i >= LA) continue;
        const int a = el / q, b = el - a * q;
        val[r] = potts_coupling(src, kind, L, q, ld, i, jB, a, b);
        dst[r] = kk * blk + a * QM + b;
    }
}

__device__ __forceinline__ void cross_chunk_store(double* __restrict__ buf, const double (&val)[kXFieldRegs], const int (&dst)[kXFieldRegs])
{
#pragma unroll
    for (int r = 0; r < kXFieldRegs; ++r)
        if (dst[r] >= 0) buf[dst[r]] = val[r];
}

// The zero-sum shift of the nblk staged blocks of buf, in place (all threads; ends with a barrier):
//   r(a) = (sum_b J(a, b)) / q, c(b) = (sum_a J(a, b)) / q, m = (sum_a r(a)) / q, each sum from 0.0 in ascending index,
//   Jt = ((J - r(a)) - c(b)) + m
template <int QM>
__device__ __forceinline__ void cross_zero_sum(double* __restrict__ buf, double* __restrict__ rc, int nblk, int q)
{
    const int blk = q * QM, per = 2 * q + 1;
    const double dq = (double)q;
    for (int e = threadIdx.x; e < nblk * 2 * q; e += kXThreads) {
        const int kk = e / (2 * q), x = e - kk * 2 * q;
        const double* B = buf + kk * blk;
        double s = 0.0;
        if (x < q) for (int b = 0; b < q; ++b) s += B[x * QM + b];
        else for (int a = 0; a < q; ++a) s += B[a * QM + (x - q)];
        rc[kk * per + x] = s / dq;
    }
    __syncthreads();
    for (int kk = threadIdx.x; kk < nblk; kk += kXThreads) {
        double s = 0.0;
        for (int a = 0; a < q; ++a) s += rc[kk * per + a];
        rc[kk * per + 2 * q] = s / dq;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < nblk * q * q; e += kXThreads) {
        const int kk = e / (q * q), el = e - kk * q * q;
        const int a = el / q, b = el - a * q;
        double* p = buf + kk * blk + a * QM + b;
        *p = ((*p - rc[kk * per + a]) - rc[kk * per + q + b]) + rc[kk * per + 2 * q];
    }
    __syncthreads();
}

// grid (ceil(nrows / 256), LB): the row blocks on x, whose limit is 2^31 - 1 (the caller holds LB below 65 536); thread =
// A-sequence m0 + c of the block.  QA: site-major codes of all A-rows, QA[i * NaS + m].
template <typename S, int QM>
__global__ __launch_bounds__(kXThreads)
void cross_fields_kernel(const S* __restrict__ src, int kind, int L, int q, int ld, int LA, int CJ, int gauge,
                         const uint8_t* __restrict__ QA, int NaS, int m0, int nrows, double* __restrict__ phi)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cross_smem[];
    const int blk = q * QM;
    const int bufVals = CJ * blk;
    double* buf0 = reinterpret_cast<double*>(cross_smem);
    double* rc = buf0 + 2 * bufVals;
    const int tid = threadIdx.x;
    const int j = blockIdx.y, jB = LA + j, LB = L - LA;
    const int c = blockIdx.x * kXThreads + tid;
    const bool live = c < nrows;
    const int steps = (LA + CJ - 1) / CJ;
    const int chunkVals = CJ * q * q;

    for (int e = tid; e < 2 * bufVals; e += kXThreads) buf0[e] = 0.0;          // the row padding stays zero

    double u[QM];
#pragma unroll
    for (int b = 0; b < QM; ++b) u[b] = 0.0;

    double val[kXFieldRegs];
    int dst[kXFieldRegs];
    __syncthreads();
    cross_chunk_load<S, QM>(src, kind, L, q, ld, LA, jB, 0, chunkVals, val, dst);
    cross_chunk_store(buf0, val, dst);
    __syncthreads();
    if (gauge) cross_zero_sum<QM>(buf0, rc, min(CJ, LA), q);

    for (int t = 0; t < steps; ++t) {
        const int i0 = t * CJ;
        if (t + 1 < steps) cross_chunk_load<S, QM>(src, kind, L, q, ld, LA, jB, i0 + CJ, chunkVals, val, dst);
        const double* cur = buf0 + (t & 1) * bufVals;
        if (live) {
#pragma unroll 1
            for (int kk = 0; kk < CJ; ++kk) {
                if (i0 + kk >= LA) break;
                const double* row = cur + kk * blk + (int)QA[(size_t)(i0 + kk) * NaS + m0 + c] * QM;
#pragma unroll
                for (int b = 0; b < QM; b += 2) {
                    const double2 v = *reinterpret_cast<const double2*>(row + b);
                    u[b] += v.x; u[b + 1] += v.y;
                }
            }
        }
        if (t + 1 < steps) {
            double* nxt = buf0 + ((t + 1) & 1) * bufVals;
            cross_chunk_store(nxt, val, dst);
            __syncthreads();
            if (gauge) cross_zero_sum<QM>(nxt, rc, min(CJ, LA - (i0 + CJ)), q);
        }
    }
    if (live) {
        double* o = phi + ((size_t)c * LB + j) * q;
#pragma unroll
        for (int b = 0; b < QM; ++b)
            if (b < q) o[b] = u[b];
    }
}

// One workgroup per item.  rowB0 / rowCnt / rowOut: per A-row of the block, the first B-row and the number of B-rows of its
// group and where its output row starts in `out`.  QB: site-major codes of all B-rows, QB[j * NbS + n].
__global__ __launch_bounds__(kXThreads)
void cross_energy_kernel(const CrossItem* __restrict__ items, const int* __restrict__ rowB0, const int* __restrict__ rowCnt,
                         const long long* __restrict__ rowOut, const double* __restrict__ phi, int LB, int q,
                         const uint8_t* __restrict__ QB, int NbS, double* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char cross_smem[];
    double* ph = reinterpret_cast<double*>(cross_smem);
    __shared__ int pre[kXSparseRows + 1], sCnt[kXSparseRows], sB0[kXSparseRows];
    __shared__ long long sOut[kXSparseRows];
    const int tid = threadIdx.x;
    const CrossItem it = items[blockIdx.x];
    const int a0 = it.a0, na = it.na, k0 = it.k0;
    if (tid < na) {
        sCnt[tid] = max(0, min(kXWindow, rowCnt[a0 + tid] - k0));
        sB0[tid] = rowB0[a0 + tid];
        sOut[tid] = rowOut[a0 + tid];
    }
    __syncthreads();
    if (tid == 0) {
        int s = 0;
        for (int r = 0; r < na; ++r) { pre[r] = s; s += sCnt[r]; }
        pre[na] = s;
    }
    __syncthreads();
    const int P = pre[na];

    int rowOf[kXSlots], nOf[kXSlots];                 // slot s: pair p = s * 256 + tid = (row rowOf, B-row nOf); -1: none
    double acc[kXSlots];
#pragma unroll
    for (int s = 0; s < kXSlots; ++s) {
        const int p = s * kXThreads + tid;
        acc[s] = 0.0;
        rowOf[s] = -1; nOf[s] = 0;
        if (p < P) {
            int r = 0;
            while (pre[r + 1] <= p) ++r;
            rowOf[s] = r;
            nOf[s] = sB0[r] + k0 + (p - pre[r]);
        }
    }

    const int jc = max(1, min(LB, (int)(kXPhiLds / ((size_t)na * q * sizeof(double)))));     // cross_chunk_sites
    const int rowVals = jc * q;
    const size_t LBq = (size_t)LB * q;
    for (int j0 = 0; j0 < LB; j0 += jc) {
        const int nj = min(jc, LB - j0), vals = nj * q;
        __syncthreads();                               // the previous chunk is no longer read
        for (int r = 0; r < na; ++r) {
            const double* g = phi + (size_t)(a0 + r) * LBq + (size_t)j0 * q;
            for (int e = tid; e < vals; e += kXThreads) ph[r * rowVals + e] = g[e];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kXSlots; ++s) {
            if (rowOf[s] < 0) continue;
            const double* base = ph + rowOf[s] * rowVals;
            const uint8_t* code = QB + (size_t)j0 * NbS + nOf[s];
            double e = acc[s];
#pragma unroll 4
            for (int jj = 0; jj < nj; ++jj) e += base[jj * q + (int)code[(size_t)jj * NbS]];
            acc[s] = e;
        }
    }
#pragma unroll
    for (int s = 0; s < kXSlots; ++s) {
        if (rowOf[s] < 0) continue;
        const int r = rowOf[s];
        out[sOut[r] + (nOf[s] - sB0[r])] = acc[s];
    }
}

template <typename S>
hipError_t launch_cross_fields(dca_ctx* ctx, const PottsView<S>& pv, int LA, int gauge, const uint8_t* dQA, int NaS, int m0, int nrows,
                               double* dPhi)
{
    return with_cross_qm(pv.q, [&](auto qm) {
        constexpr int QM = decltype(qm)::value;
        auto kern = cross_fields_kernel<S, QM>;
        const size_t lds = cross_field_lds(pv.q);
        HIP_PASS(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(ceil_div(nrows, kXThreads), pv.L - LA), dim3(kXThreads), lds, ctx->stream, pv.src, pv.kind, pv.L,
                           pv.q, pv.ld, LA, cross_field_chunk(pv.q), gauge, dQA, NaS, m0, nrows, dPhi);
        return hipGetLastError();
    });
}

// host rows (n x len) -> device site-major codes dst[s * nS + c] (zero past n)
int upload_site_major(dca_ctx* ctx, const uint8_t* X, int n, int len, int nS, DevBuf<uint8_t>& dst, const char* who)
{
    DevBuf<uint8_t> dRows;
    HIP_TRY_AS_NOMEM(dst.alloc((size_t)len * nS, false), who);
    HIP_TRY_AS_NOMEM(dRows.alloc((size_t)std::max(n, 1) * len, false), who);
    HIP_TRY_AS(hipMemcpyAsync(dRows, X, (size_t)n * len, hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS(dca_rows_to_sites(ctx, dRows, (size_t)len, n, len, nS, dst), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}

}  // namespace

int dca_potts_interaction_energies(dca_ctx* ctx, const PottsSource& ps, int split, const uint8_t* XA, int nA, const uint8_t* XB, int nB,
                                   const int32_t* offsets_a, const int32_t* offsets_b, int G, int gauge, double* out)
{
    static const char* who = "interaction_energies";
    const int L = ps.L, q = ps.q, LA = split, LB = L - split;
    if (split < 1 || split > L - 1) { dca_set_error("%s: split %d outside [1, %d]", who, split, L - 1); return DCA_ERR_ARG; }
    if (nA < 0 || nB < 0 || G < 1 || (gauge != 0 && gauge != 1) || !offsets_a || !offsets_b) {
        dca_set_error("%s: bad arguments (nA %d, nB %d, G %d, gauge %d, offsets %s)", who, nA, nB, G, gauge,
                      offsets_a && offsets_b ? "given" : "NULL");
        return DCA_ERR_ARG;
    }
    if (offsets_a[0] != 0 || offsets_b[0] != 0 || offsets_a[G] != nA || offsets_b[G] != nB) {
        dca_set_error("%s: the offsets must start at 0 and end at nA = %d and nB = %d", who, nA, nB);
        return DCA_ERR_ARG;
    }
    size_t total = 0;
    for (int g = 0; g < G; ++g) {
        if (offsets_a[g + 1] < offsets_a[g] || offsets_b[g + 1] < offsets_b[g]) {
            dca_set_error("%s: the offsets decrease at group %d", who, g);
            return DCA_ERR_ARG;
        }
        total += (size_t)(offsets_a[g + 1] - offsets_a[g]) * (size_t)(offsets_b[g + 1] - offsets_b[g]);
    }
    if (total == 0) return DCA_OK;
    if (LB > 65535) { dca_set_error("%s: %d B-sites, at most 65535", who, LB); return DCA_ERR_ARG; }      // cross_fields' grid.y
    if (!XA || !XB || !out) { dca_set_error("%s: NULL array with %zu energies to form", who, total); return DCA_ERR_ARG; }
    DCA_TRY(dca_check_codes(XA, (size_t)nA * LA, q, "interaction_energies: A "));
    DCA_TRY(dca_check_codes(XB, (size_t)nB * LB, q, "interaction_energies: B "));

    // per A-row: the B-rows of its group and where its output row starts
    std::vector<int32_t> rowB0((size_t)nA), rowCnt((size_t)nA);
    std::vector<long long> rowOut((size_t)nA + 1);
    {
        long long o = 0;
        for (int g = 0; g < G; ++g) {
            const int cnt = offsets_b[g + 1] - offsets_b[g];
            for (int m = offsets_a[g]; m < offsets_a[g + 1]; ++m) { rowB0[m] = offsets_b[g]; rowCnt[m] = cnt; rowOut[m] = o; o += cnt; }
        }
        rowOut[nA] = o;
    }

    const int NaS = (int)round_up((size_t)nA, 128), NbS = (int)round_up((size_t)nB, 128);
    DevBuf<uint8_t> dQA, dQB;
    DCA_TRY(upload_site_major(ctx, XA, nA, LA, NaS, dQA, who));
    DCA_TRY(upload_site_major(ctx, XB, nB, LB, NbS, dQB, who));

    const int cap = cross_pass_cap();
    int maxRows = 0, maxItems = 0;
    size_t maxOut = 0;
    for (int m0 = 0; m0 < nA;) {
        const int rows = cross_pass_rows(rowCnt.data(), nA, m0, LB, q, cap);
        maxRows = std::max(maxRows, rows);
        maxOut = std::max(maxOut, (size_t)(rowOut[m0 + rows] - rowOut[m0]));
        maxItems = std::max(maxItems, (int)cross_items(rowCnt.data() + m0, rows).size());
        m0 += rows;
    }
    DevBuf<double> dPhi, dOut;
    DevBuf<int> dB0, dCnt;
    DevBuf<long long> dRowOut;
    DevBuf<CrossItem> dItems;
    HIP_TRY_AS_NOMEM(dPhi.alloc((size_t)maxRows * LB * q, false), who);
    HIP_TRY_AS_NOMEM(dOut.alloc(std::max<size_t>(maxOut, 1), false), who);
    HIP_TRY_AS_NOMEM(dB0.alloc((size_t)maxRows, false), who);
    HIP_TRY_AS_NOMEM(dCnt.alloc((size_t)maxRows, false), who);
    HIP_TRY_AS_NOMEM(dRowOut.alloc((size_t)maxRows, false), who);
    HIP_TRY_AS_NOMEM(dItems.alloc((size_t)std::max(maxItems, 1), false), who);
    HIP_TRY_AS(hipFuncSetAttribute(reinterpret_cast<const void*>(cross_energy_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kXPhiLds), who);

    std::vector<long long> localOut;
    for (int m0 = 0; m0 < nA;) {
        const int rows = cross_pass_rows(rowCnt.data(), nA, m0, LB, q, cap);
        const size_t nOut = (size_t)(rowOut[m0 + rows] - rowOut[m0]);
        if (nOut > 0) {
            const std::vector<CrossItem> items = cross_items(rowCnt.data() + m0, rows);
            localOut.assign(rowOut.begin() + m0, rowOut.begin() + m0 + rows);
            for (auto& v : localOut) v -= rowOut[m0];
            HIP_TRY_AS(hipMemcpyAsync(dB0, rowB0.data() + m0, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);
            HIP_TRY_AS(hipMemcpyAsync(dCnt, rowCnt.data() + m0, (size_t)rows * sizeof(int), hipMemcpyHostToDevice, ctx->stream), who);
            HIP_TRY_AS(hipMemcpyAsync(dRowOut, localOut.data(), (size_t)rows * sizeof(long long), hipMemcpyHostToDevice, ctx->stream), who);
            HIP_TRY_AS(hipMemcpyAsync(dItems, items.data(), items.size() * sizeof(CrossItem), hipMemcpyHostToDevice, ctx->stream), who);
            {
                ScopedKernelClock kc(ctx, "cross_fields");
                HIP_TRY_AS(with_source_type(ps, [&](auto pv) { return launch_cross_fields(ctx, pv, LA, gauge, dQA.get(), NaS, m0, rows, dPhi.get()); }), who);
            }
            {
                ScopedKernelClock kc(ctx, "cross_energy");
                hipLaunchKernelGGL(cross_energy_kernel, dim3((unsigned)items.size()), dim3(kXThreads), kXPhiLds, ctx->stream,
                                   (const CrossItem*)dItems.get(), (const int*)dB0.get(), (const int*)dCnt.get(),
                                   (const long long*)dRowOut.get(), (const double*)dPhi.get(), LB, q, (const uint8_t*)dQB.get(), NbS,
                                   dOut.get());
                HIP_TRY_AS(hipGetLastError(), who);
            }
            HIP_TRY_AS(hipMemcpyAsync(out + rowOut[m0], dOut, nOut * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), who);
            HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);     // the host tables of this block are free again
        }
        m0 += rows;
    }
    return DCA_OK;
}
