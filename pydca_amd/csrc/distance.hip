// Nearest neighbours and the distance histogram of a query set against a reference set (dca_hamming_nearest):
// dist[k] = min_m d(Q_k, R_m), index[k] = the smallest m that attains it, hist[d] = #{(k, m) compared : d(Q_k, R_m) = d}.
//
// The inner loop is that of weights_count_kernel (weights.hip): both sets are re-coded into bit planes (PL = 5 dwords per 32
// sites for q <= 32, 3 for q <= 8; file order for both sets -- the distance does not depend on the column order), a pair costs
// PL xor + or + one popcount-add per 32 sites; 64 x 64 (query x reference) tiles, a 4 x 4 register block per lane, plane rows
// staged through LDS (row stride 26 / 18 dwords, 8-byte reads: conflict free).  What differs is the shape and the reductions:
//   * the tile matrix is rectangular (Q != R in general) and walked in 32 x 32 super-tiles so that the workgroups in flight
//     share row and column tiles in L2.  For Q == R both halves are computed (one code path; twice the triangle's compares);
//   * no early exit: the histogram needs every distance (see DESIGN.md section 17 for the pruned variant that was not built);
//   * minimum: each lane forms the smallest packed key (distance << 32) | m of its 4 columns per row, the 16 lanes of a row meet
//     by wave shuffles, and ONE 64-bit unsigned atomicMin per query and tile goes to a key array initialised to all-ones
//     (skipped when the key in memory is already smaller: keys only fall).  The minimum over packed keys is associative and
//     commutative, so the result does not depend on arrival order, and ties resolve to the smallest index by construction;
//   * histogram: uint32 bins in LDS (ds_add_u32; at most 4096 per workgroup and bin), flushed with 64-bit integer atomicAdd
//     into the global bins -- integer sums, order-free.  L + 1 bins beside the 13 KiB of staging: up to L = kLdsHistMaxL the
//     bins live in LDS, above it every pair adds to the global bins directly (slower, same integers).
// Rows past nq / nr and the skipped pairs (k == m) reach neither reduction.  Everything is integer: the outputs do not depend
// on the batch, the pass split or the launch geometry.
#include <cstdlib>
#include <vector>

#include "dca_internal.h"
#include "hamming_planes.h"

namespace {

constexpr int kTile = 64;      // sequences per tile side
constexpr int kKG = 4;         // 32-site groups per LDS stage
constexpr int kSuper = 32;     // tiles per super-tile side
constexpr int kLdsHistMaxL = 12287;        // (L + 1) * 4 bytes <= 48 KiB of dynamic LDS beside the static staging buffers
constexpr unsigned long long kNoKey = ~0ull;

// nn_bitplanes_kernel: hamming_planes.h (shared with redundancy.hip)

__global__ void nn_fill_keys_kernel(unsigned long long* __restrict__ keys, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) keys[k] = kNoKey;
}

__global__ void nn_unpack_kernel(const unsigned long long* __restrict__ keys, int32_t* __restrict__ dist, int32_t* __restrict__ index, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const unsigned long long key = keys[k];
    dist[k] = key == kNoKey ? -1 : (int32_t)(key >> 32);
    index[k] = key == kNoKey ? -1 : (int32_t)(key & 0xffffffffull);
}

// HIST 0: no histogram, 1: LDS bins (dynamic LDS of (L + 1) uint32), 2: global bins
// kOff: the index of query row 0 of this launch within the whole query set (the pass offset; what skipSame compares with m)
template <int PL, int HIST>
__global__ __launch_bounds__(256)
void nn_tile_kernel(const uint32_t* __restrict__ PQ, const uint32_t* __restrict__ PR, int nq, int nr, int G, int L, int kOff, int skipSame,
                    int tilesQ, int tilesR, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ hist)
{
    constexpr int PLP = (PL + 1) & ~1;
    constexpr int ROWDW = kKG * PLP;
    constexpr int STRIDE = ROWDW + 2;
    __shared__ __attribute__((aligned(8))) uint32_t sA[kTile * STRIDE];
    __shared__ __attribute__((aligned(8))) uint32_t sB[kTile * STRIDE];
    extern __shared__ uint32_t sHist[];
    const int superCols = (tilesR + kSuper - 1) / kSuper;
    const int sid = blockIdx.x / (kSuper * kSuper), within = blockIdx.x % (kSuper * kSuper);
    const int tileY = (sid / superCols) * kSuper + within / kSuper;
    const int tileX = (sid % superCols) * kSuper + within % kSuper;
    if (tileY >= tilesQ || tileX >= tilesR) return;          // workgroup-uniform
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int rowBase = tileY * kTile, colBase = tileX * kTile;
    if (HIST == 1)
        for (int d = threadIdx.x; d <= L; d += 256) sHist[d] = 0u;        // the first barrier of the loop below orders these
    const int rowDwords = G * PLP;
    unsigned mism[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) mism[r][c] = 0u;

    for (int g0 = 0; g0 < G; g0 += kKG) {
        __syncthreads();
        // a stage is ROWDW dwords (64 or 96 bytes, 16-byte aligned: G is a multiple of kKG) of every row; rows past the sets are zeros
        constexpr int Q4 = ROWDW / 4;
        for (int t = threadIdx.x; t < kTile * Q4; t += 256) {
            const int r = t / Q4, k4 = t % Q4;
            uint4 a = make_uint4(0, 0, 0, 0), b = a;
            if (rowBase + r < nq) a = *reinterpret_cast<const uint4*>(PQ + (size_t)(rowBase + r) * rowDwords + g0 * PLP + 4 * k4);
            if (colBase + r < nr) b = *reinterpret_cast<const uint4*>(PR + (size_t)(colBase + r) * rowDwords + g0 * PLP + 4 * k4);
            uint2* da = reinterpret_cast<uint2*>(&sA[r * STRIDE + 4 * k4]);
            uint2* db = reinterpret_cast<uint2*>(&sB[r * STRIDE + 4 * k4]);
            da[0] = make_uint2(a.x, a.y); da[1] = make_uint2(a.z, a.w);
            db[0] = make_uint2(b.x, b.y); db[1] = make_uint2(b.z, b.w);
        }
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < kKG; ++gg) {
            uint32_t a[4][PLP], b[4][PLP];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int h = 0; h < PLP / 2; ++h) {
                    const uint2 v = *reinterpret_cast<const uint2*>(&sA[(ty + 16 * r) * STRIDE + gg * PLP + 2 * h]);
                    a[r][2 * h] = v.x; a[r][2 * h + 1] = v.y;
                }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int h = 0; h < PLP / 2; ++h) {
                    const uint2 v = *reinterpret_cast<const uint2*>(&sB[(tx + 16 * c) * STRIDE + gg * PLP + 2 * h]);
                    b[c][2 * h] = v.x; b[c][2 * h + 1] = v.y;
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    uint32_t d = a[r][0] ^ b[c][0];
#pragma unroll
                    for (int p = 1; p < PL; ++p) d |= a[r][p] ^ b[c][p];
                    mism[r][c] += __popc(d);
                }
        }
    }
    // a compared pair: both rows inside their sets and not the skipped diagonal.  Its distance is <= L (the padding sites
    // are state 0 on both sides), so the bins 0..L hold every one.
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = rowBase + ty + 16 * r;
        unsigned long long best = kNoKey;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int m = colBase + tx + 16 * c;
            if (k >= nq || m >= nr || (skipSame && kOff + k == m)) continue;
            const unsigned long long key = ((unsigned long long)mism[r][c] << 32) | (unsigned)m;
            best = key < best ? key : best;
            if (HIST == 1) atomicAdd(&sHist[mism[r][c]], 1u);
            if (HIST == 2) atomicAdd(&hist[mism[r][c]], 1ull);
        }
        // the 16 tx lanes that share this row differ in the low 4 lane bits
        for (int off = 8; off > 0; off >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)best, off), hi = __shfl_xor((unsigned)(best >> 32), off);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other < best ? other : best;
        }
        if (tx == 0 && k < nq && best != kNoKey && best < __hip_atomic_load(&keys[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMin(&keys[k], best);
    }
    if (HIST == 1) {
        __syncthreads();
        for (int d = threadIdx.x; d <= L; d += 256)
            if (sHist[d]) atomicAdd(&hist[d], (unsigned long long)sHist[d]);
    }
}

template <int PL>
hipError_t launch_planes(dca_ctx* ctx, const uint8_t* dRows, size_t stride, int n, uint32_t* dP)
{
    const int G = ctx->Ls / 32;
    const unsigned tb = (unsigned)(((size_t)n * G + 255) / 256);
    hipLaunchKernelGGL(nn_bitplanes_kernel<PL>, dim3(tb), dim3(256), 0, ctx->stream, dRows, stride, ctx->L, dP, n, G);
    return hipGetLastError();
}

template <int PL>
hipError_t launch_tiles(dca_ctx* ctx, const uint32_t* dPQ, const uint32_t* dPR, int nq, int nr, int kOff, bool skipSame,
                        unsigned long long* dKeys, unsigned long long* dHist)
{
    const int G = ctx->Ls / 32, L = ctx->L;
    const int tilesQ = ceil_div(nq, kTile), tilesR = ceil_div(nr, kTile);
    const size_t blocks = (size_t)ceil_div(tilesQ, kSuper) * ceil_div(tilesR, kSuper) * kSuper * kSuper;
    const dim3 grid((unsigned)blocks);
    if (!dHist)
        hipLaunchKernelGGL((nn_tile_kernel<PL, 0>), grid, dim3(256), 0, ctx->stream, dPQ, dPR, nq, nr, G, L, kOff, (int)skipSame, tilesQ, tilesR, dKeys, dHist);
    else if (L <= kLdsHistMaxL)
        hipLaunchKernelGGL((nn_tile_kernel<PL, 1>), grid, dim3(256), (size_t)(L + 1) * sizeof(uint32_t), ctx->stream, dPQ, dPR, nq, nr, G, L, kOff,
                           (int)skipSame, tilesQ, tilesR, dKeys, dHist);
    else
        hipLaunchKernelGGL((nn_tile_kernel<PL, 2>), grid, dim3(256), 0, ctx->stream, dPQ, dPR, nq, nr, G, L, kOff, (int)skipSame, tilesQ, tilesR, dKeys, dHist);
    return hipGetLastError();
}

}  // namespace

int dca_hamming_nearest_impl(dca_ctx* ctx, const uint8_t* Q, int nq, const uint8_t* R, int nr, bool skipSame, int32_t* dist_out,
                             int32_t* index_out, uint64_t* hist_out)
{
    const int L = ctx->L, q = ctx->q, G = ctx->Ls / 32;
    const bool small = q <= 8;
    const int PLP = small ? 4 : 6;
    if (!R) nr = ctx->N;
    if (!Q) nq = nr;
    if (R) DCA_TRY(dca_check_codes(R, (size_t)nr * L, q, "dca_hamming_nearest: R "));
    if (Q) DCA_TRY(dca_check_codes(Q, (size_t)nq * L, q, "dca_hamming_nearest: Q "));
    // tile counts and the launch's workgroup count stay far inside int / unsigned: (2^31 / 64 / 32)^2 * 1024 would not
    if ((double)ceil_div(ceil_div(nq, kTile), kSuper) * ceil_div(ceil_div(nr, kTile), kSuper) * kSuper * kSuper > 2e9) {
        dca_set_error("dca_hamming_nearest: %d x %d sequences are more than one launch holds; split the reference set", nq, nr);
        return DCA_ERR_ARG;
    }
    const int pass = Q ? std::min(nq, dca_nn_pass_size()) : nq;
    static const char* who = "dca_hamming_nearest";
    DevBuf<uint8_t> dR, dQ;
    DevBuf<uint32_t> dPR, dPQ;
    DevBuf<unsigned long long> dKeys, dHist;
    DevBuf<int32_t> dOut;
    HIP_TRY_AS(dPR.alloc((size_t)nr * G * PLP, false), who);
    if (R) HIP_TRY_AS(dR.alloc((size_t)nr * L, false), who);
    if (Q) HIP_TRY_AS(dQ.alloc((size_t)pass * L, false), who);
    if (Q) HIP_TRY_AS(dPQ.alloc((size_t)pass * G * PLP, false), who);
    HIP_TRY_AS(dKeys.alloc((size_t)nq, false), who);
    HIP_TRY_AS(dOut.alloc((size_t)nq * 2, false), who);
    if (hist_out) HIP_TRY_AS(dHist.alloc((size_t)(L + 1), false), who);
    if (hist_out) HIP_TRY_AS(hipMemsetAsync(dHist, 0, (size_t)(L + 1) * sizeof(unsigned long long), ctx->stream), who);
    if (R) HIP_TRY_AS(hipMemcpyAsync(dR, R, (size_t)nr * L, hipMemcpyHostToDevice, ctx->stream), who);
    {
        ScopedKernelClock kc(ctx, "hamming");
        hipLaunchKernelGGL(nn_fill_keys_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, ctx->stream, dKeys.get(), nq);
        const uint8_t* rows = R ? dR.get() : ctx->dX;
        const size_t stride = R ? (size_t)L : (size_t)ctx->Ls;
        HIP_TRY_AS(small ? launch_planes<3>(ctx, rows, stride, nr, dPR) : launch_planes<5>(ctx, rows, stride, nr, dPR), who);
    }
    // the passes: queries [k0, k0 + n) against the whole reference set; a query's key sees the same pairs whatever the split
    for (int k0 = 0; k0 < nq; k0 += pass) {
        const int n = std::min(pass, nq - k0);
        if (Q) HIP_TRY_AS(hipMemcpyAsync(dQ, Q + (size_t)k0 * L, (size_t)n * L, hipMemcpyHostToDevice, ctx->stream), who);
        ScopedKernelClock kc(ctx, "hamming");
        if (Q) HIP_TRY_AS(small ? launch_planes<3>(ctx, dQ, (size_t)L, n, dPQ) : launch_planes<5>(ctx, dQ, (size_t)L, n, dPQ), who);
        const uint32_t* pq = Q ? dPQ.get() : dPR.get();
        HIP_TRY_AS(small ? launch_tiles<3>(ctx, pq, dPR, n, nr, k0, skipSame, dKeys + k0, dHist)
                         : launch_tiles<5>(ctx, pq, dPR, n, nr, k0, skipSame, dKeys + k0, dHist), who);
        if (Q && k0 + pass < nq) HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);       // the next pass refills dQ / dPQ
    }
    {
        ScopedKernelClock kc(ctx, "hamming");
        hipLaunchKernelGGL(nn_unpack_kernel, dim3(ceil_div(nq, 256)), dim3(256), 0, ctx->stream, dKeys.get(), dOut.get(), dOut + nq, nq);
        HIP_TRY_AS(hipGetLastError(), who);
    }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    HIP_TRY_AS(hipMemcpy(dist_out, dOut, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    if (index_out) HIP_TRY_AS(hipMemcpy(index_out, dOut + nq, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    if (hist_out) HIP_TRY_AS(hipMemcpy(hist_out, dHist, (size_t)(L + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost), who);
    return DCA_OK;
}
