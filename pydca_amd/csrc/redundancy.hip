// Redundancy filter and identity clusters of an alignment (dca_identity_filter, dca_identity_clusters).
// Two rows are SIMILAR iff ident = #{i : X_mi = X_ni} >= T, T an integer number of sites (the gap state counts like any other,
// as in weights.hip).  Everything is integer and every reduction is a minimum or a sum of integers, so the outputs depend on
// neither the launch geometry nor the order in which atomics arrive.
//
// The compares are those of weights.hip and distance.hip: rows re-coded into bit planes (hamming_planes.h; PL = 5 dwords per 32
// sites for q <= 32, 3 for q <= 8), a pair costs PL xor + or + one popcount-add per 32 sites, 64 x 64 tiles, a 4 x 4 register
// block per lane, plane rows staged through LDS (row stride 26 / 18 dwords, 8-byte reads).  One tile routine (tile_mismatches)
// serves three epilogues:
//   * COVER (filter): rows of a block of rank positions against the compact list of the plane rows kept so far; a similar pair
//     sends the kept row's RANK POSITION to a 32-bit unsigned atomicMin on the candidate's key (preset to all-ones; the 16 lanes
//     of a row meet by shuffles first).  The count of kept rows is read from device memory: the launch covers the worst case
//     and the tiles past the count return.  With the weight kernel's early exit (pairs past L - T mismatches cannot be similar);
//   * BITS (filter's block pass, clusters): a lane's 16 compare results meet by __ballot; lane 16 j of a wave assembles the
//     64-bit word of row j and writes it with one 8-byte vector store.  A tile owns whole dwords: no atomics.  No early exit:
//     every wave compares all groups, like the self leg of dca_hamming_nearest, both halves on one code path;
//   * HOOK (clusters above DCA_CLUSTER_BITS_MAX): the hook step straight from the compares, nothing stored; degrees by integer
//     atomicAdd in the first round.  With the early exit.
#include <cstdlib>
#include <vector>

#include "dca_internal.h"
#include "hamming_planes.h"
#include "redundancy_plan.h"

namespace {

constexpr int kTile = kRedTile;
constexpr int kKG = kRedKG;
constexpr int kSuper = kRedSuper;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kPast = 0x40000000;        // the mismatch count of a pair with a row past its set: beyond every threshold

enum { MODE_COVER = 0, MODE_BITS = 1, MODE_HOOK = 2 };

// mism[r][c] of the tile's pairs (row rowBase + ty + 16 r of PA, row colBase + tx + 16 c of PB); pairs with a row past nA / nB
// hold kPast.  EXIT: the early exit of weights_count_kernel; returns true for a wave whose pairs have all passed maxMism.
template <int PL, bool EXIT>
__device__ __forceinline__ bool tile_mismatches(const uint32_t* __restrict__ PA, const uint32_t* __restrict__ PB, int nA, int nB, int rowBase,
                                                int colBase, int G, int maxMism, int (&mism)[4][4], uint32_t* sA, uint32_t* sB)
{
    constexpr int PLP = (PL + 1) & ~1;
    constexpr int ROWDW = kKG * PLP;
    constexpr int STRIDE = ROWDW + 2;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int rowDwords = G * PLP;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) mism[r][c] = (rowBase + ty + 16 * r < nA && colBase + tx + 16 * c < nB) ? 0 : kPast;
    bool waveDone = false;       // wave-uniform
    auto all_passed = [&]() {
        int mn = mism[0][0];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) mn = min(mn, mism[r][c]);
        return mn > maxMism;
    };
    for (int g0 = 0; g0 < G; g0 += kKG) {
        if (EXIT) {
            if (__syncthreads_and(waveDone)) break;      // also the barrier that protects sA / sB
        } else {
            __syncthreads();
        }
        // a stage is ROWDW dwords (64 or 96 bytes, 16-byte aligned: G is a multiple of kKG) of every row; rows past the sets are zeros
        constexpr int Q4 = ROWDW / 4;
        for (int t = threadIdx.x; t < kTile * Q4; t += kRedThreads) {
            const int r = t / Q4, k4 = t % Q4;
            uint4 a = make_uint4(0, 0, 0, 0), b = a;
            if (rowBase + r < nA) a = *reinterpret_cast<const uint4*>(PA + (size_t)(rowBase + r) * rowDwords + g0 * PLP + 4 * k4);
            if (colBase + r < nB) b = *reinterpret_cast<const uint4*>(PB + (size_t)(colBase + r) * rowDwords + g0 * PLP + 4 * k4);
            uint2* da = reinterpret_cast<uint2*>(&sA[r * STRIDE + 4 * k4]);
            uint2* db = reinterpret_cast<uint2*>(&sB[r * STRIDE + 4 * k4]);
            da[0] = make_uint2(a.x, a.y); da[1] = make_uint2(a.z, a.w);
            db[0] = make_uint2(b.x, b.y); db[1] = make_uint2(b.z, b.w);
        }
        __syncthreads();
#pragma unroll
        for (int gg = 0; gg < kKG; ++gg) {
            if (EXIT) {
                if (g0 + gg > 0 && !waveDone) waveDone = __all(all_passed());
                if (waveDone) continue;
            }
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
        if (EXIT && !waveDone) waveDone = __all(all_passed());
    }
    return waveDone;
}

struct TileArgs {
    const uint32_t* PA;
    const uint32_t* PB;
    int nA, nB;
    const int* nBDev;            // COVER: the count of kept rows, in device memory (replaces nB)
    int G, maxMism;              // similar iff mismatches <= maxMism = L - T (-1: nothing is)
    int tilesQ, tilesR;          // the tile rectangle the launch covers
    uint32_t* keys;              // COVER: per row of PA
    const int32_t* keptRank;     // COVER: rank position of every row of PB
    uint32_t* bits;              // BITS: row stride W dwords
    int W;
    int32_t* label;              // HOOK
    uint32_t* degree;            // HOOK: first round only, else NULL
    int* flag;                   // HOOK
};

template <int PL, int MODE>
__global__ __launch_bounds__(kRedThreads)
void sim_tile_kernel(const TileArgs A)
{
    constexpr int PLP = (PL + 1) & ~1;
    constexpr int STRIDE = kKG * PLP + 2;
    __shared__ __attribute__((aligned(8))) uint32_t sA[kTile * STRIDE];
    __shared__ __attribute__((aligned(8))) uint32_t sB[kTile * STRIDE];
    // the 1-D grid walks the tile matrix in 32 x 32 super-tiles, as hamming_kernel does
    const int superCols = (A.tilesR + kSuper - 1) / kSuper;
    const int sid = blockIdx.x / (kSuper * kSuper), within = blockIdx.x % (kSuper * kSuper);
    const int tileY = (sid / superCols) * kSuper + within / kSuper;
    const int tileX = (sid % superCols) * kSuper + within % kSuper;
    if (tileY >= A.tilesQ || tileX >= A.tilesR) return;          // workgroup-uniform
    const int nB = MODE == MODE_COVER ? *A.nBDev : A.nB;
    const int rowBase = tileY * kTile, colBase = tileX * kTile;
    if (MODE == MODE_COVER && colBase >= nB) return;             // beyond the rows kept so far: workgroup-uniform
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    int mism[4][4];
    const bool waveDone = tile_mismatches<PL, MODE != MODE_BITS>(A.PA, A.PB, A.nA, nB, rowBase, colBase, A.G, A.maxMism, mism, sA, sB);

    if (MODE == MODE_COVER) {
        if (waveDone) return;                                    // wave-uniform: no pair of this wave is similar
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint32_t best = kNone;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int m = colBase + tx + 16 * c;
                if (mism[r][c] <= A.maxMism) best = min(best, (uint32_t)A.keptRank[m]);       // in range: a pair past nA / nB holds kPast
            }
            for (int off = 8; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));     // the 16 tx lanes of this row
            const int k = rowBase + ty + 16 * r;
            if (tx == 0 && best != kNone) atomicMin(&A.keys[k], best);
        }
    }
    if (MODE == MODE_BITS) {
        // ballot bit (ty & 3) * 16 + tx of (r, c) is the pair (row ty + 16 r, column tx + 16 c): lane 16 j of the wave gathers the
        // 64 columns of row 4 wave + j + 16 r
        const int j = ty & 3;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned long long word = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned long long bal = __ballot(mism[r][c] <= A.maxMism);
                word |= ((bal >> (16 * j)) & 0xffffull) << (16 * c);
            }
            if (tx == 0)
                *reinterpret_cast<uint2*>(&A.bits[(size_t)(rowBase + ty + 16 * r) * A.W + 2 * tileX]) = make_uint2((uint32_t)word, (uint32_t)(word >> 32));
        }
    }
    if (MODE == MODE_HOOK) {
        if (waveDone) return;
        bool any = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = rowBase + ty + 16 * r;
            unsigned cnt = 0;
            int li = 0;
            bool have = false;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (mism[r][c] > A.maxMism) continue;
                ++cnt;
                const int m = colBase + tx + 16 * c;
                if (!have) { li = __hip_atomic_load(&A.label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); have = true; }
                const int lj = __hip_atomic_load(&A.label[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lj < li) { atomicMin(&A.label[li], lj); any = true; }
            }
            if (A.degree) {
                for (int off = 8; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
                if (tx == 0 && cnt) atomicAdd(&A.degree[i], cnt);         // integer sums: order-free
            }
        }
        if (any) *A.flag = 1;
    }
}

__global__ void red_fill_keys_kernel(uint32_t* __restrict__ keys, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) keys[k] = kNone;
}

__global__ void red_iota_kernel(int32_t* __restrict__ label, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) label[k] = k;
}

// plane rows in rank order: Prank[p] = Pfile[order[p]]
__global__ void red_gather_rows_kernel(const uint32_t* __restrict__ Pfile, const int32_t* __restrict__ order, uint32_t* __restrict__ Prank,
                                       int n, int rowDwords)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * rowDwords) return;
    const size_t p = idx / rowDwords;
    const int d = (int)(idx % rowDwords);
    Prank[idx] = Pfile[(size_t)order[p] * rowDwords + d];
}

// One workgroup resolves the block [p0, p0 + Bn) in ascending rank position.  sRep[j]: the representative's rank position of
// position p0 + j, kNone while it has none (at the end: kept).  The positions are taken in groups of 64: wave 0 settles a group
// in registers (lane = position; the group's diagonal 64 x 64 bits are one 64-bit word per lane), then all lanes hand the
// group's kept positions to the later positions of the block -- by symmetry bit (j, i) of the LATER row j tells whether the
// kept position i covers it, and the lowest set bit of (row word & kept mask) is the earliest such position.  A position is
// only ever given a representative while it has none, and groups run in ascending order, so it ends with the earliest one.
__global__ __launch_bounds__(kRedThreads)
void filter_resolve_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ bits, int W, int p0, int Bn,
                           int32_t* __restrict__ repRank, int32_t* __restrict__ slotOf, int32_t* __restrict__ keptRank, int* __restrict__ keptCount)
{
    extern __shared__ uint32_t sRep[];
    __shared__ unsigned long long sKept;
    const int tid = threadIdx.x;
    for (int j = tid; j < Bn; j += kRedThreads) sRep[j] = keys[p0 + j];
    int count = *keptCount;
    __syncthreads();
    const int groups = (Bn + 63) / 64;
    for (int g = 0; g < groups; ++g) {
        if (tid < 64) {                                           // wave 0
            const int j = g * 64 + tid;
            uint32_t rep = j < Bn ? sRep[j] : 0u;                 // a position past the block counts as covered
            unsigned long long m = 0;
            if (j < Bn) {
                const uint2 v = *reinterpret_cast<const uint2*>(&bits[(size_t)j * W + 2 * g]);
                m = (unsigned long long)v.x | ((unsigned long long)v.y << 32);
            }
            unsigned long long kept = 0;
            for (int i = 0; i < 64; ++i) {
                const unsigned long long open = __ballot(rep == kNone);
                if (!((open >> i) & 1ull)) continue;              // wave-uniform: position i already has a representative
                kept |= 1ull << i;
                if (tid > i && ((m >> i) & 1ull) && rep == kNone) rep = (uint32_t)(p0 + g * 64 + i);
            }
            if (j < Bn) {
                const bool isKept = rep == kNone;
                const int slot = count + __popcll(kept & ((1ull << tid) - 1ull));
                sRep[j] = rep;
                repRank[p0 + j] = isKept ? p0 + j : (int32_t)rep;
                slotOf[p0 + j] = isKept ? slot : -1;
                if (isKept) keptRank[slot] = p0 + j;
            }
            count += __popcll(kept);
            if (tid == 0) sKept = kept;
        }
        __syncthreads();
        const unsigned long long kept = sKept;
        if (kept)
            for (int j = (g + 1) * 64 + tid; j < Bn; j += kRedThreads) {
                if (sRep[j] != kNone) continue;
                const uint2 v = *reinterpret_cast<const uint2*>(&bits[(size_t)j * W + 2 * g]);
                const unsigned long long cand = ((unsigned long long)v.x | ((unsigned long long)v.y << 32)) & kept;
                if (cand) sRep[j] = (uint32_t)(p0 + g * 64 + (__ffsll((long long)cand) - 1));
            }
        __syncthreads();
    }
    if (tid == 0) *keptCount = count;
}

// the block's kept plane rows go to their slots of the compact list
__global__ void filter_append_kernel(const uint32_t* __restrict__ Prank, const int32_t* __restrict__ slotOf, uint32_t* __restrict__ Pkept,
                                     int p0, int Bn, int rowDwords)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)Bn * rowDwords) return;
    const size_t p = p0 + idx / rowDwords;
    const int d = (int)(idx % rowDwords);
    const int s = slotOf[p];
    if (s >= 0) Pkept[(size_t)s * rowDwords + d] = Prank[p * rowDwords + d];
}

// rank positions -> row indices
__global__ void filter_unpack_kernel(const int32_t* __restrict__ repRank, const int32_t* __restrict__ order, uint8_t* __restrict__ keep,
                                     int32_t* __restrict__ rep, int n)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int rp = repRank[p];
    const int r = order ? order[p] : p;
    keep[r] = rp == p ? 1 : 0;
    rep[r] = order ? order[rp] : rp;
}

// hook step from the stored bits: one thread per dword of the n x W matrix
__global__ void cluster_hook_bits_kernel(const uint32_t* __restrict__ bits, int n, int W, int32_t* __restrict__ label, int* __restrict__ flag)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * W) return;
    uint32_t d = bits[idx];
    if (!d) return;
    const int i = (int)(idx / W), w = (int)(idx % W);
    const int li = __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool any = false;
    while (d) {
        const int j = 32 * w + __ffs((int)d) - 1;
        d &= d - 1;
        const int lj = __hip_atomic_load(&label[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lj < li) { atomicMin(&label[li], lj); any = true; }
    }
    if (any) *flag = 1;
}

// pointer jumping to the root: labels only fall (label[x] <= x) and the roots do not move while this kernel runs, so every
// chain ends and label[i] is i's root afterwards -- "until stable" in one launch
__global__ void cluster_jump_kernel(int32_t* __restrict__ label, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int l = __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        const int p = __hip_atomic_load(&label[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == l) break;
        l = p;
    }
    __hip_atomic_store(&label[i], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// degree[r] = popcount of row r of the bits: one wave per row, lanes over the dwords, the 64 partial sums met by shuffles
__global__ __launch_bounds__(kRedThreads)
void cluster_degree_kernel(const uint32_t* __restrict__ bits, int n, int W, uint32_t* __restrict__ degree)
{
    const int row = blockIdx.x * (kRedThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;                   // wave-uniform
    unsigned cnt = 0;
    for (int w = lane; w < W; w += 64) cnt += __popc(bits[(size_t)row * W + w]);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) degree[row] = cnt;
}

template <int MODE>
hipError_t launch_tiles(dca_ctx* ctx, bool small, const TileArgs& a)
{
    const dim3 grid((unsigned)red_walk_blocks(a.tilesQ, a.tilesR));
    if (small) hipLaunchKernelGGL((sim_tile_kernel<3, MODE>), grid, dim3(kRedThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL((sim_tile_kernel<5, MODE>), grid, dim3(kRedThreads), 0, ctx->stream, a);
    return hipGetLastError();
}

// the rows (host X, or the context's alignment) as bit planes in file order
int build_planes(dca_ctx* ctx, const uint8_t* X, int n, DevBuf<uint8_t>& dRows, DevBuf<uint32_t>& dP, const char* who)
{
    const int L = ctx->L, G = ctx->Ls / 32;
    const bool small = ctx->q <= 8;
    const int PLP = small ? 4 : 6;
    HIP_TRY_AS_NOMEM(dP.alloc((size_t)n * G * PLP, false), who);
    if (X) {
        HIP_TRY_AS_NOMEM(dRows.alloc((size_t)n * L, false), who);
        HIP_TRY_AS(hipMemcpyAsync(dRows, X, (size_t)n * L, hipMemcpyHostToDevice, ctx->stream), who);
    }
    const uint8_t* rows = X ? dRows.get() : ctx->dX;
    const size_t stride = X ? (size_t)L : (size_t)ctx->Ls;
    const unsigned tb = (unsigned)(((size_t)n * G + 255) / 256);
    if (small) hipLaunchKernelGGL(nn_bitplanes_kernel<3>, dim3(tb), dim3(256), 0, ctx->stream, rows, stride, L, dP.get(), n, G);
    else hipLaunchKernelGGL(nn_bitplanes_kernel<5>, dim3(tb), dim3(256), 0, ctx->stream, rows, stride, L, dP.get(), n, G);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}

long env_long(const char* name)
{
    const char* e = getenv(name);
    return e ? atol(e) : 0;
}

}  // namespace

int dca_identity_filter_impl(dca_ctx* ctx, const uint8_t* X, int n, int T, const int32_t* order, uint8_t* keep_out, int32_t* rep_out,
                             dca_filter_info* info)
{
    static const char* who = "dca_identity_filter";
    const int L = ctx->L, q = ctx->q, G = ctx->Ls / 32;
    const bool small = q <= 8;
    const int PLP = small ? 4 : 6, rowDwords = G * PLP;
    if (!X) n = ctx->N;
    if (X) DCA_TRY(dca_check_codes(X, (size_t)n * L, q, "dca_identity_filter: "));
    if (order) {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int p = 0; p < n; ++p) {
            const int r = order[p];
            if (r < 0 || r >= n || seen[r]) { dca_set_error("dca_identity_filter: order is not a permutation of 0..%d (entry %d is %d)", n - 1, p, r); return DCA_ERR_ARG; }
            seen[r] = 1;
        }
    }
    const FilterPlan plan = filter_plan(n, env_long("DCA_FILTER_BLOCK"));
    if ((double)red_walk_blocks(plan.B / kTile, red_ceil_div(n, kTile)) > 2e9) {
        dca_set_error("dca_identity_filter: %d sequences are more than one launch holds", n);
        return DCA_ERR_ARG;
    }
    DevBuf<uint8_t> dRows, dKeep;
    DevBuf<uint32_t> dPfile, dPrank, dPkept, dKeys, dBits;
    DevBuf<int32_t> dOrder, dRepRank, dSlot, dKeptRank, dRep;
    DevBuf<int> dCount;
    HIP_TRY_AS_NOMEM(dPkept.alloc((size_t)n * rowDwords, false), who);
    HIP_TRY_AS_NOMEM(dKeys.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dBits.alloc((size_t)plan.B * plan.W, false), who);
    HIP_TRY_AS_NOMEM(dRepRank.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dSlot.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dKeptRank.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dRep.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dKeep.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dCount.alloc(1), who);
    if (order) {
        HIP_TRY_AS_NOMEM(dOrder.alloc((size_t)n, false), who);
        HIP_TRY_AS_NOMEM(dPrank.alloc((size_t)n * rowDwords, false), who);
        HIP_TRY_AS(hipMemcpyAsync(dOrder, order, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    }
    HIP_TRY_AS(hipMemsetAsync(dCount, 0, sizeof(int), ctx->stream), who);
    {
        ScopedKernelClock kc(ctx, "identity_filter");
        DCA_TRY(build_planes(ctx, X, n, dRows, dPfile, who));
        if (order)
            hipLaunchKernelGGL(red_gather_rows_kernel, dim3((unsigned)(((size_t)n * rowDwords + 255) / 256)), dim3(256), 0, ctx->stream,
                               dPfile.get(), dOrder.get(), dPrank.get(), n, rowDwords);
        const uint32_t* P = order ? dPrank.get() : dPfile.get();
        hipLaunchKernelGGL(red_fill_keys_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dKeys.get(), n);
        HIP_TRY_AS(hipGetLastError(), who);
        for (int p0 = 0; p0 < n; p0 += plan.B) {
            const int Bn = std::min(plan.B, n - p0);
            TileArgs a{};
            a.PA = P + (size_t)p0 * rowDwords;
            a.nA = Bn;
            a.G = G;
            a.maxMism = L - T;
            a.tilesQ = ceil_div(Bn, kTile);
            if (p0 > 0) {            // cover: against everything kept so far -- at most p0 rows, the count itself stays on the device
                a.PB = dPkept.get();
                a.nBDev = dCount.get();
                a.tilesR = ceil_div(p0, kTile);
                a.keys = dKeys.get() + p0;
                a.keptRank = dKeptRank.get();
                HIP_TRY_AS(launch_tiles<MODE_COVER>(ctx, small, a), who);
            }
            a.PB = a.PA;             // block: the B x B similarity bits
            a.nB = Bn;
            a.nBDev = nullptr;
            a.tilesR = a.tilesQ;
            a.bits = dBits.get();
            a.W = plan.W;
            HIP_TRY_AS(launch_tiles<MODE_BITS>(ctx, small, a), who);
            hipLaunchKernelGGL(filter_resolve_kernel, dim3(1), dim3(kRedThreads), plan.ldsResolve, ctx->stream, dKeys.get(), dBits.get(), plan.W,
                               p0, Bn, dRepRank.get(), dSlot.get(), dKeptRank.get(), dCount.get());
            hipLaunchKernelGGL(filter_append_kernel, dim3((unsigned)(((size_t)Bn * rowDwords + 255) / 256)), dim3(256), 0, ctx->stream, P,
                               dSlot.get(), dPkept.get(), p0, Bn, rowDwords);
            HIP_TRY_AS(hipGetLastError(), who);
        }
        hipLaunchKernelGGL(filter_unpack_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dRepRank.get(), dOrder.get(), dKeep.get(),
                           dRep.get(), n);
        HIP_TRY_AS(hipGetLastError(), who);
    }
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);       // the one synchronisation
    int kept = 0;
    HIP_TRY_AS(hipMemcpy(keep_out, dKeep, (size_t)n, hipMemcpyDeviceToHost), who);
    if (rep_out) HIP_TRY_AS(hipMemcpy(rep_out, dRep, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    HIP_TRY_AS(hipMemcpy(&kept, dCount, sizeof(int), hipMemcpyDeviceToHost), who);
    if (info) { info->kept = kept; info->blocks = plan.blocks; info->block_rows = plan.B; info->tile_pairs = plan.tilePairs; }
    return DCA_OK;
}

int dca_identity_clusters_impl(dca_ctx* ctx, const uint8_t* X, int n, int T, int32_t* label_out, int32_t* degree_out, dca_cluster_info* info)
{
    static const char* who = "dca_identity_clusters";
    const int L = ctx->L, q = ctx->q, G = ctx->Ls / 32;
    const bool small = q <= 8;
    if (!X) n = ctx->N;
    if (X) DCA_TRY(dca_check_codes(X, (size_t)n * L, q, "dca_identity_clusters: "));
    const char* capEnv = getenv("DCA_CLUSTER_BITS_MAX");
    const unsigned long long cap = capEnv ? strtoull(capEnv, nullptr, 10) : kClusterBitsMaxDefault;
    const ClusterPlan plan = cluster_plan(n, cap);
    if ((double)red_walk_blocks(plan.tiles, plan.tiles) > 2e9) {
        dca_set_error("dca_identity_clusters: %d sequences are more than one launch holds", n);
        return DCA_ERR_ARG;
    }
    DevBuf<uint8_t> dRows;
    DevBuf<uint32_t> dP, dBits, dDegree;
    DevBuf<int32_t> dLabel;
    DevBuf<int> dFlag;
    HIP_TRY_AS_NOMEM(dLabel.alloc((size_t)n, false), who);
    HIP_TRY_AS_NOMEM(dDegree.alloc((size_t)n), who);
    HIP_TRY_AS_NOMEM(dFlag.alloc(1), who);
    if (plan.stored) HIP_TRY_AS_NOMEM(dBits.alloc((size_t)plan.allocDwords, false), who);
    TileArgs a{};
    a.nA = a.nB = n;
    a.G = G;
    a.maxMism = L - T;
    a.tilesQ = a.tilesR = plan.tiles;
    int rounds = 0;
    {
        ScopedKernelClock kc(ctx, "identity_clusters");
        DCA_TRY(build_planes(ctx, X, n, dRows, dP, who));
        a.PA = a.PB = dP.get();
        hipLaunchKernelGGL(red_iota_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dLabel.get(), n);
        HIP_TRY_AS(hipGetLastError(), who);
        if (plan.stored) {
            {
                ScopedKernelClock kb(ctx, "identity_clusters_bits");
                a.bits = dBits.get();
                a.W = plan.W;
                HIP_TRY_AS(launch_tiles<MODE_BITS>(ctx, small, a), who);
            }
            ScopedKernelClock kd(ctx, "identity_clusters_degrees");
            hipLaunchKernelGGL(cluster_degree_kernel, dim3(ceil_div(n, kRedThreads / 64)), dim3(kRedThreads), 0, ctx->stream, dBits.get(), n, plan.W,
                               dDegree.get());
            HIP_TRY_AS(hipGetLastError(), who);
        } else {
            HIP_TRY_AS(hipMemsetAsync(dDegree, 0, (size_t)n * sizeof(uint32_t), ctx->stream), who);
            a.label = dLabel.get();
            a.flag = dFlag.get();
        }
        // rounds of hook + pointer jumping until one passes without a change; the flag comes back once per round
        for (;;) {
            int changed = 0;
            {
                ScopedKernelClock kr(ctx, "identity_clusters_rounds");
                HIP_TRY_AS(hipMemsetAsync(dFlag, 0, sizeof(int), ctx->stream), who);
                if (plan.stored) {
                    hipLaunchKernelGGL(cluster_hook_bits_kernel, dim3((unsigned)(((size_t)n * plan.W + 255) / 256)), dim3(256), 0, ctx->stream,
                                       dBits.get(), n, plan.W, dLabel.get(), dFlag.get());
                    HIP_TRY_AS(hipGetLastError(), who);
                } else {
                    a.degree = rounds == 0 ? dDegree.get() : nullptr;
                    HIP_TRY_AS(launch_tiles<MODE_HOOK>(ctx, small, a), who);
                }
                hipLaunchKernelGGL(cluster_jump_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, dLabel.get(), n);
                HIP_TRY_AS(hipGetLastError(), who);
                HIP_TRY_AS(hipMemcpyAsync(&changed, dFlag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream), who);
            }
            HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
            ++rounds;
            if (!changed) break;
        }
    }
    HIP_TRY_AS(hipMemcpy(label_out, dLabel, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    if (degree_out) HIP_TRY_AS(hipMemcpy(degree_out, dDegree, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost), who);
    if (info) {
        std::vector<int32_t> size((size_t)n, 0);
        for (int r = 0; r < n; ++r) size[label_out[r]]++;
        int clusters = 0, largest = 0;
        for (int r = 0; r < n; ++r) { clusters += size[r] > 0; largest = std::max(largest, (int)size[r]); }
        info->clusters = clusters; info->largest = largest; info->rounds = rounds; info->stored_bits = plan.stored ? 1 : 0;
    }
    return DCA_OK;
}
