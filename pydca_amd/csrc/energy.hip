// Statistical energies of query sequences and single-mutant scans under a fitted Potts model:
//   E(s) = sum_i h_i(s_i) + sum_{i<j} J_ij(s_i, s_j),
//   dE(i,a) = h_i(a) - h_i(w_i) + sum_{j != i} [J_ij(a, w_j) - J_ij(w_i, w_j)].
// The model arrives as a PottsSource and is read through PottsView (potts_source.h).
//
// Every term is widened to double and summed in double in an order fixed by (L, q, dtype) alone:
//   pair kernel: the site pairs are cut into TS x TS tiles (site blocks bi <= bj, row-major), the tiles into G groups of
//     consecutive tiles; a workgroup holds one tile at a time in LDS and streams a block of query sequences against it,
//     one thread per sequence; per sequence its group's tiles are added in ascending order, each tile's pairs in (i, j)
//     order, and the group's sum goes to slab g.  No float atomics; the model is read once per sequence block.
//   finish kernel: per sequence the fields in ascending site order, then the slabs in ascending g.
// Neither order depends on the number of query sequences or on a sequence's place among them.
//
// The tile size and the grouping are energy_geometry's (potts_plan.h).
//
// The query codes are kept site-major (code of site s of sequence n at s * NqS + n, NqS a multiple of 128): the lanes of a
// wave, one sequence each, then read one contiguous 64-byte run per site instead of 64 cache lines.
#include "dca_internal.h"

namespace {

constexpr int kEThreads = 512;                     // pair-kernel workgroup: 8 waves
constexpr int kESeqPerThread = 8;                  // sequences per thread: one tile load serves 4096 sequences
static_assert(kESeqBlock == kEThreads * kESeqPerThread, "potts_plan.h holds the sequence block of this workgroup");

// grid (G, sequence blocks).  LDS: one tile, TS*TS pairs of q*q values of type S (pair (ii, jj) at (ii*TS + jj) * q*q).
template <typename S, int TS>
__global__ __launch_bounds__(kEThreads)
void energy_pairs_kernel(const S* __restrict__ src, int kind, int L, int q, int ld, const uint8_t* __restrict__ QT, int nq,
                         int NqS, int nb, int ntiles, int tpg, double* __restrict__ slabs)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char energy_smem[];
    S* tile = reinterpret_cast<S*>(energy_smem);
    const int qq = q * q;
    const int g = blockIdx.x;
    const int seq0 = blockIdx.y * kESeqBlock + threadIdx.x;
    int t = g * tpg;
    const int tEnd = min(ntiles, t + tpg);
    int bi = 0, rowStart = 0;                      // tile t = (bi, bj): row bi holds tiles rowStart .. rowStart + nb - bi - 1
    while (t >= rowStart + nb - bi) { rowStart += nb - bi; ++bi; }
    int bj = bi + (t - rowStart);
    double acc[kESeqPerThread];
#pragma unroll
    for (int r = 0; r < kESeqPerThread; ++r) acc[r] = 0.0;

    for (; t < tEnd; ++t) {
        const int i0 = bi * TS, j0 = bj * TS;
        const int ni = min(TS, L - i0), nj = min(TS, L - j0);
        const bool diag = bi == bj;
        __syncthreads();                           // the previous tile is no longer read
        for (int e = threadIdx.x; e < TS * TS * qq; e += kEThreads) {
            const int k = e / qq, ab = e - k * qq;
            const int ii = k / TS, jj = k - ii * TS;
            S v = (S)0;
            if (ii < ni && jj < nj && (!diag || jj > ii)) v = (S)potts_coupling(src, kind, L, q, ld, i0 + ii, j0 + jj, ab / q, ab % q);
            tile[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kESeqPerThread; ++r) {
            const int n = seq0 + r * kEThreads;
            if (n < nq) {
                int cjo[TS];
#pragma unroll
                for (int jj = 0; jj < TS; ++jj) cjo[jj] = jj * qq + (jj < nj ? (int)QT[(size_t)(j0 + jj) * NqS + n] : 0);
                double s = acc[r];
#pragma unroll 1
                for (int ii = 0; ii < ni; ++ii) {
                    const S* row = tile + ii * TS * qq + (int)QT[(size_t)(i0 + ii) * NqS + n] * q;
#pragma unroll
                    for (int jj = 0; jj < TS; ++jj)
                        if (jj < nj && (!diag || jj > ii)) s += (double)row[cjo[jj]];
                }
                acc[r] = s;
            }
        }
        if (++bj == nb) { ++bi; bj = bi; }
    }
#pragma unroll
    for (int r = 0; r < kESeqPerThread; ++r) {
        const int n = seq0 + r * kEThreads;
        if (n < nq) slabs[(size_t)g * NqS + n] = acc[r];
    }
}

// E(n) = sum_i h_i(s_i) (ascending i) + sum_g slab[g][n] (ascending g)
template <typename S>
__global__ __launch_bounds__(256)
void energy_finish_kernel(const PottsView<S> pv, const uint8_t* __restrict__ QT, int nq, int NqS, const double* __restrict__ slabs,
                          int G, double* __restrict__ out)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= nq) return;
    double e = 0.0;
    for (int i = 0; i < pv.L; ++i) e += pv.field(i, QT[(size_t)i * NqS + n]);
    for (int g = 0; g < G; ++g) e += slabs[(size_t)g * NqS + n];
    out[n] = e;
}

// One 64-lane workgroup per site i; lane a < q: S(a) = sum_{j != i, ascending} J_ij(a, w_j) (block (min, max) of the
// pair, as the energy reads it), dE(i, a) = (h_i(a) - h_i(w_i)) + (S(a) - S(w_i)); dE(i, w_i) = 0.
template <typename S>
__global__ __launch_bounds__(64)
void mutation_scan_kernel(const PottsView<S> pv, const uint8_t* __restrict__ wt, double* __restrict__ dE)
{
    __shared__ double sumW, hW;
    const int L = pv.L, q = pv.q;
    const int i = blockIdx.x, a = threadIdx.x;
    const int wi = wt[i];
    double s = 0.0, h = 0.0;
    if (a < q) {
        for (int j = 0; j < L; ++j) {
            if (j == i) continue;
            s += j > i ? pv.coupling(i, j, a, wt[j]) : pv.coupling(j, i, wt[j], a);
        }
        h = pv.field(i, a);
        if (a == wi) { sumW = s; hW = h; }
    }
    __syncthreads();
    if (a < q) dE[(size_t)i * q + a] = a == wi ? 0.0 : (h - hW) + (s - sumW);
}

template <typename S, int TS>
hipError_t launch_pairs(dca_ctx* ctx, const EnergyGeom& eg, const PottsView<S>& pv, const uint8_t* QT, int nq, int NqS, double* slabs)
{
    const size_t lds = energy_lds(TS, pv.q, sizeof(S));
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(energy_pairs_kernel<S, TS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((energy_pairs_kernel<S, TS>), dim3(eg.G, ceil_div(nq, kESeqBlock)), dim3(kEThreads), lds, ctx->stream,
                       pv.src, pv.kind, pv.L, pv.q, pv.ld, QT, nq, NqS, eg.nb, eg.ntiles, eg.tpg, slabs);
    return hipGetLastError();
}

template <typename S>
hipError_t dispatch_pairs(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* QT, int nq, int NqS, double* slabs)
{
    const EnergyGeom eg = energy_geometry(pv.L, pv.q, sizeof(S));
    switch (eg.TS) {
    case 24: return launch_pairs<S, 24>(ctx, eg, pv, QT, nq, NqS, slabs);
    case 16: return launch_pairs<S, 16>(ctx, eg, pv, QT, nq, NqS, slabs);
    case 12: return launch_pairs<S, 12>(ctx, eg, pv, QT, nq, NqS, slabs);
    case 8: return launch_pairs<S, 8>(ctx, eg, pv, QT, nq, NqS, slabs);
    case 6: return launch_pairs<S, 6>(ctx, eg, pv, QT, nq, NqS, slabs);
    case 4: return launch_pairs<S, 4>(ctx, eg, pv, QT, nq, NqS, slabs);
    default: return launch_pairs<S, 3>(ctx, eg, pv, QT, nq, NqS, slabs);
    }
}

template <typename S>
int energies_t(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* X, int n, double* out)
{
    const int L = pv.L;
    const EnergyGeom eg = energy_geometry(L, pv.q, sizeof(S));
    const int cap = std::min(n, kEChunk);
    const int NqS = (int)round_up((size_t)cap, 128);
    DevBuf<uint8_t> dRows, dQT;
    DevBuf<double> dSlabs, dOut;
    HIP_TRY_AS(dRows.alloc((size_t)cap * L, false), "energies");
    HIP_TRY_AS(dQT.alloc((size_t)L * NqS, false), "energies");
    HIP_TRY_AS(dSlabs.alloc((size_t)eg.G * NqS, false), "energies");
    HIP_TRY_AS(dOut.alloc((size_t)NqS, false), "energies");
    for (int first = 0; first < n; first += cap) {
        const int nq = std::min(cap, n - first);
        HIP_TRY_AS(hipMemcpyAsync(dRows, X + (size_t)first * L, (size_t)nq * L, hipMemcpyHostToDevice, ctx->stream), "energies");
        HIP_TRY_AS(dca_rows_to_sites(ctx, dRows, (size_t)L, nq, L, NqS, dQT), "energies");
        {
            ScopedKernelClock kc(ctx, "energies");
            HIP_TRY_AS(dispatch_pairs<S>(ctx, pv, dQT, nq, NqS, dSlabs), "energies");
            hipLaunchKernelGGL(energy_finish_kernel<S>, dim3(ceil_div(nq, 256)), dim3(256), 0, ctx->stream, pv, dQT.get(), nq, NqS,
                               dSlabs.get(), eg.G, dOut.get());
        }
        HIP_TRY_AS(hipGetLastError(), "energies");
        HIP_TRY_AS(hipMemcpyAsync(out + first, dOut, (size_t)nq * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "energies");
        HIP_TRY_AS(hipStreamSynchronize(ctx->stream), "energies");
    }
    return DCA_OK;
}

template <typename S>
int mutation_scan_t(dca_ctx* ctx, const PottsView<S>& pv, const uint8_t* wt, double* out)
{
    const int L = pv.L, q = pv.q;
    DevBuf<uint8_t> dWt;
    DevBuf<double> dOut;
    HIP_TRY_AS(dWt.alloc((size_t)L), "mutation scan");
    HIP_TRY_AS(dOut.alloc((size_t)L * q, false), "mutation scan");
    HIP_TRY_AS(hipMemcpyAsync(dWt, wt, (size_t)L, hipMemcpyHostToDevice, ctx->stream), "mutation scan");
    {
        ScopedKernelClock kc(ctx, "mutation_scan");
        hipLaunchKernelGGL(mutation_scan_kernel<S>, dim3(L), dim3(64), 0, ctx->stream, pv, dWt.get(), dOut.get());
        HIP_TRY_AS(hipGetLastError(), "mutation scan");
    }
    HIP_TRY_AS(hipMemcpyAsync(out, dOut, (size_t)L * q * sizeof(double), hipMemcpyDeviceToHost, ctx->stream), "mutation scan");
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), "mutation scan");
    return DCA_OK;
}

}  // namespace

int dca_check_codes(const uint8_t* codes, size_t count, int q, const char* what)
{
    for (size_t k = 0; k < count; ++k)
        if (codes[k] >= q) { dca_set_error("%scode %d >= q at element %zu", what, (int)codes[k], k); return DCA_ERR_ARG; }
    return DCA_OK;
}

int dca_potts_energies(dca_ctx* ctx, const PottsSource& ps, const uint8_t* X, int n, double* out)
{
    if (n < 0 || (n > 0 && (!X || !out))) { dca_set_error("energies: bad arguments"); return DCA_ERR_ARG; }
    if (n == 0) return DCA_OK;
    DCA_TRY(dca_check_codes(X, (size_t)n * ps.L, ps.q, ""));
    return with_source_type(ps, [&](auto pv) { return energies_t(ctx, pv, X, n, out); });
}

int dca_potts_mutation_scan(dca_ctx* ctx, const PottsSource& ps, const uint8_t* wt, double* out)
{
    if (!wt || !out) { dca_set_error("mutation scan: bad arguments"); return DCA_ERR_ARG; }
    DCA_TRY(dca_check_codes(wt, (size_t)ps.L, ps.q, ""));
    return with_source_type(ps, [&](auto pv) { return mutation_scan_t(ctx, pv, wt, out); });
}

// ---- the pair stage on device-resident site-major codes (ais.hip): the same kernels, geometry and order as above
int dca_energy_slab_count(const PottsSource& ps)
{
    return energy_geometry(ps.L, ps.q, ps.dtype == DCA_F32 ? sizeof(float) : sizeof(double)).G;
}

hipError_t dca_energy_pairs_device(dca_ctx* ctx, const PottsSource& ps, const uint8_t* dQT, int nq, int NqS, double* dSlabs)
{
    return with_source_type(ps, [&](auto pv) { return dispatch_pairs(ctx, pv, dQT, nq, NqS, dSlabs); });
}
