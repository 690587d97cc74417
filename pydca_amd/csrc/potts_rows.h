// Row i of the couplings J staged through LDS, once for the kernels that sum u(a) = ... + sum_j J_ij(a, s_j) with one lane per
// chain or query and compile to the same instructions with it: the conditional sweep and field pass (sample_conditional.hip), the
// ascent's table pass (ascent.hip) and the row add of site_conditionals.h.  gibbs_sweep_kernel (sample.hip) keeps its own inline
// text: at its register limit any factored form moved the allocator's result and cost 2.8 %.
//
// A staged chunk holds CJ blocks of q x q values, block kk at kk * blk (blk = q * QM), stored transposed, T[b][a] = J_ij(a, b), rows
// padded to QM values (the padding is zeroed once by the kernel and never written), so that a lane reads J_ij(., s_j) as QM
// contiguous values.  The blocks of a chunk are those of the POSITIONS k0 .. k0 + CJ - 1 of a site mapping.
#pragma once
#include "dca_internal.h"

// Position -> site.  A template argument of the kernels: AllSites compiles to the plain loop over j with no list load.
struct AllSites {                                   // count = L, site(k) = k
    static constexpr bool listed = false;
    int count;
    __device__ __forceinline__ AllSites(const int*, int n) : count(n) {}
    __device__ __forceinline__ int site(int k) const { return k; }
};
struct ListedSites {                                // site(k) = list[k], ascending; the list in global memory or LDS
    static constexpr bool listed = true;
    const int* list;
    int count;
    __device__ __forceinline__ ListedSites(const int* l, int n) : list(l), count(n) {}
    __device__ __forceinline__ int site(int k) const { return list[k]; }
};

// registers <- the blocks of row i at the positions k0 .. k0 + CJ - 1 of `map` (the position `self` is left out; -1: none):
// element e of the chunk is value e % q^2 of the stored block of position k0 + e / q^2, and goes to dst = kk * blk + b * QM + a
// for the term J_ij(a, b).  THREADS threads, R elements each; chunkVals = CJ * q^2, mqq and mq: fast_div's factors of q^2 and q.
template <typename S, int QM, int R, int THREADS, typename MAP>
__device__ __forceinline__ void row_chunk_load(const S* __restrict__ src, int kind, int L, int q, int ld, const MAP& map, int self, int i,
                                               int k0, int chunkVals, uint32_t mqq, uint32_t mq, S (&val)[R], int (&dst)[R])
{
    const int qq = q * q, blk = q * QM;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int e = threadIdx.x + r * THREADS;
        dst[r] = -1;
        if (e >= chunkVals) continue;
        const int kk = fast_div(e, mqq), el = e - kk * qq;
        const int k = k0 + kk;
        if (k >= map.count || k == self) continue;
        const int j = map.site(k);
        const int hi = fast_div(el, mq), lo = el - hi * q;
        const int a = j > i ? hi : lo, b = j > i ? lo : hi;          // source order: (a, b) rows for j > i, (b, a) for j < i
        val[r] = (S)(j > i ? potts_coupling(src, kind, L, q, ld, i, j, a, b) : potts_coupling(src, kind, L, q, ld, j, i, b, a));
        dst[r] = kk * blk + b * QM + a;
    }
}

template <typename S, int R>
__device__ __forceinline__ void row_chunk_store(S* __restrict__ buf, const S (&val)[R], const int (&dst)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (dst[r] >= 0) buf[dst[r]] = val[r];
}

// u[a] += row[a], a < QM, every term widened to double
template <typename S, int QM>
__device__ __forceinline__ void add_row(double (&u)[QM], const S* __restrict__ row)
{
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
