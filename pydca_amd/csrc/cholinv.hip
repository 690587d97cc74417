// Inverse of a symmetric positive definite float64 matrix on MI355X, used for
// couplings = -inv(C)  (reference: compute_couplings, pydca/meanfield_dca/msa_numerics.py:321-342,
// which goes through LAPACK getrf/getri; C is SPD for pseudocount > 0, so the Cholesky route
// inv(A) = L^-T L^-1 is used: ~n^3 flop instead of 2 n^3).
//
// Everything that is a GEMM runs on the f64 matrix cores (v_mfma_f64_16x16x4_f64):
//   recursive block step on A = [[A11, .], [A21, A22]]  (sizes multiples of 64)
//     (X11)        <- cholinv(A11)                 X = L^-1, stored lower + mirrored upper
//     L21          <- A21 * X11^T                  (TRSM as a GEMM with the inverse)
//     A22          <- A22 - L21 * L21^T            (SYRK, lower tiles only)
//     (X22)        <- cholinv(A22)
//     T^T          <- X11^T * L21^T
//     X21          <- -X22 * T                     (written to (2,1) and mirrored to (1,2))
//   finally inv(A) = X^T X as one triangular-aware GEMM.
// All products are of the form C[i][j] = sum_k A[i][k] * B[j][k] ("NT", both operands
// K-contiguous), which is why X is kept mirrored: X^T rows are then plain rows.
// The 64x64 diagonal leaves (Cholesky + triangular inverse) run in one workgroup in LDS.
#include <climits>
#include <mutex>
#include <atomic>

#include <string>

#include "dca_internal.h"
#include "cholinv_plan.h"      // MASK_*, WALK_*, and every launch decision that is host arithmetic

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 64, BN = 64;

// The kernels of the factorisation's serial chain (leaves, few-tile products) raise their waves' issue priority: when the
// bulk products of another stream (the recursion's background product, the sweep's update launches) share a CU with them, the
// chain's instructions go first on the shared SIMDs and matrix pipes (s_setprio arbitrates between the waves of a CU; it is not a queue priority -- those made the chain slower, round 3).
#ifndef DCA_CHAIN_PRIO_LEVEL
#define DCA_CHAIN_PRIO_LEVEL 3
#endif
#define DCA_CHAIN_PRIO() __builtin_amdgcn_s_setprio(DCA_CHAIN_PRIO_LEVEL)

struct GemmArgs {
    const double* A; int lda; int maskA;
    const double* B; int ldb; int maskB;
    double* C; int ldc;
    double* Cm; int ldcm;          // optional mirror: Cm[j][i] = C[i][j]
    int M, N, K;
    double alpha, beta;
    int lowerOnly;                 // square output: only tiles with tj <= ti; strict mirror rule on the diagonal
    int walk;                      // order in which the tiles are started, so that with a triangular operand the tiles with the
                                   // longest k range are not the ones that start last (WALK_*)
    int row0 = 0;                  // first tile row of this launch (WALK_ROWS only): a product issued as several row bands
    const double* Cin = nullptr; int ldcin = 0;   // beta != 0: the addend is read from here instead of from C (C is then written only)
};

// The deep-k product on 32 x 32 output tiles, for launches that are far fewer than one 64 x 64 tile per CU: a tile's
// time is its k loop on the matrix pipe (64 cycles per 16 x 16 x 4 MFMA, one wave per SIMD) and 256 CUs are there, so a
// quarter of the work per workgroup on four times as many CUs is what shortens the chain of small products in the
// recursion (plain product of n = 640: 34 -> 21 us, n = 256: 16 -> 8, the 2 x 2-tile products of the 256-nodes 10.6 -> 5.2 us;
// inverse at n = 10 048: 27.1 -> 24.2 ms, at n = 4000: 4.96 -> 3.95 ms).  Each wave one 16 x 16 accumulator.
// Staging: global -> registers (raw) -> LDS in 16-byte pieces, one wave-wide load covering 8 full 128-byte lines; the triangular
// masks are applied when a tile is WRITTEN to LDS, after the MFMAs of the current tile, so the loads of the next tile are in
// flight during those MFMAs.  (The register-staged kernel on 64 x 64 tiles that this one descends from sat between two
// dispatch bounds that were equal in every setting, 400 / 400 and 16 / 16 in the sweep: no size reached it, and it is gone.)
__device__ __forceinline__ void gemm_nt_f64_small_tile(const GemmArgs& g, int bx, int by, int gy)
{
    constexpr int TM = 32, BK = 64;
    constexpr int LDS_STRIDE = BK + 2;
    constexpr int PG = BK / 16;
    typedef double double2_t __attribute__((ext_vector_type(2)));
    DCA_CHAIN_PRIO();
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_gemm_smem[];
    double* const As = reinterpret_cast<double*>(dca_gemm_smem);      // [2][TM * LDS_STRIDE]
    double* const Bs = As + 2 * TM * LDS_STRIDE;
    const int ti = g.walk == WALK_COLUMNS_REVERSED ? bx : g.walk == WALK_ROWS_REVERSED ? gy - 1 - by : by + g.row0;
    const int tj = g.walk == WALK_COLUMNS_REVERSED ? gy - 1 - by : bx;
    if (g.lowerOnly && tj > ti) return;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    int kLo = 0, kHi = g.K;
    if (g.maskA == MASK_LOWER) kHi = min(kHi, (ti + 1) * TM);
    if (g.maskA == MASK_UPPER) kLo = max(kLo, ti * TM);
    if (g.maskB == MASK_LOWER) kHi = min(kHi, (tj + 1) * TM);
    if (g.maskB == MASK_UPPER) kLo = max(kLo, tj * TM);
    kLo = kLo / BK * BK;
    const int nk = (kHi - kLo + BK - 1) / BK;

    double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int sr = tid >> 3, sp = (tid & 7) * 2;                      // row 0 .. 31, doubles sp + 16 pg, + 1 of the k-tile
    const double* Ap = g.A + (size_t)(ti * TM + sr) * g.lda + sp;
    const double* Bp = g.B + (size_t)(tj * TM + sr) * g.ldb + sp;
    double2_t ra[PG], rb[PG];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int pg = 0; pg < PG; ++pg) {
            ra[pg] = *reinterpret_cast<const double2_t*>(Ap + k0 + 16 * pg);
            rb[pg] = *reinterpret_cast<const double2_t*>(Bp + k0 + 16 * pg);
        }
    };
    auto store_tile = [&](int buf, int k0) {
        const bool diagA = g.maskA != MASK_NONE && k0 + BK > ti * TM && k0 < (ti + 1) * TM;
        const bool diagB = g.maskB != MASK_NONE && k0 + BK > tj * TM && k0 < (tj + 1) * TM;
        if (diagA || diagB) {
            const int aRow = ti * TM + sr, bRow = tj * TM + sr;
            const int aLo = g.maskA == MASK_UPPER ? aRow : INT_MIN, aHi = g.maskA == MASK_LOWER ? aRow : INT_MAX;
            const int bLo = g.maskB == MASK_UPPER ? bRow : INT_MIN, bHi = g.maskB == MASK_LOWER ? bRow : INT_MAX;
#pragma unroll
            for (int pg = 0; pg < PG; ++pg)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int k = k0 + 16 * pg + sp + u;
                    ra[pg][u] = (k < aLo || k > aHi) ? 0.0 : ra[pg][u];
                    rb[pg][u] = (k < bLo || k > bHi) ? 0.0 : rb[pg][u];
                }
        }
#pragma unroll
        for (int pg = 0; pg < PG; ++pg) {
            *reinterpret_cast<double2_t*>(As + buf * TM * LDS_STRIDE + sr * LDS_STRIDE + 16 * pg + sp) = ra[pg];
            *reinterpret_cast<double2_t*>(Bs + buf * TM * LDS_STRIDE + sr * LDS_STRIDE + 16 * pg + sp) = rb[pg];
        }
    };
    auto mma_tile = [&](int buf) {
        const double* as = As + buf * TM * LDS_STRIDE;
        const double* bs = Bs + buf * TM * LDS_STRIDE;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const int kcol = kk * 8 + 2 * (lane >> 4);
            const double2_t a = *reinterpret_cast<const double2_t*>(&as[(wm * 16 + (lane & 15)) * LDS_STRIDE + kcol]);
            const double2_t b = *reinterpret_cast<const double2_t*>(&bs[(wn * 16 + (lane & 15)) * LDS_STRIDE + kcol]);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc, 0, 0, 0);
        }
    };
    if (nk > 0) { load_tile(kLo); store_tile(0, kLo); }
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) load_tile(kLo + (t + 1) * BK);
        mma_tile(buf);
        if (t + 1 < nk) store_tile(buf ^ 1, kLo + (t + 1) * BK);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = ti * TM + wm * 16 + (lane >> 4) + 4 * r;
        const int j = tj * TM + wn * 16 + (lane & 15);
        if (g.lowerOnly && j > i) continue;
        double v = g.alpha * acc[r];
        double* cp = g.C + (size_t)i * g.ldc + j;
        if (g.beta != 0.0) v += g.beta * (g.Cin ? g.Cin[(size_t)i * g.ldcin + j] : *cp);
        *cp = v;
        if (g.Cm && !(g.lowerOnly && i == j)) g.Cm[(size_t)j * g.ldcm + i] = v;
    }
}

__global__ __launch_bounds__(256)
void gemm_nt_f64_small_kernel(GemmArgs g)
{
    gemm_nt_f64_small_tile(g, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

// Two INDEPENDENT few-tile products in one launch (blockIdx.z picks; the grid is the larger of the two): the recursion's
// A22 -= L21 L21^T and T^T = X11^T L21^T both need L21 and nothing of each other, and at the lower levels a launch costs
// what its handful of tiles cost.
__global__ __launch_bounds__(256)
void gemm_nt_f64_small_pair_kernel(GemmArgs g0, int gx0, int gy0, GemmArgs g1, int gx1, int gy1)
{
    const bool second = blockIdx.z != 0;
    const int gx = second ? gx1 : gx0, gy = second ? gy1 : gy0;
    if ((int)blockIdx.x >= gx || (int)blockIdx.y >= gy) return;
    gemm_nt_f64_small_tile(second ? g1 : g0, (int)blockIdx.x, (int)blockIdx.y, gy);
}

// The same product with the operand tiles brought into LDS by LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane straight
// from global memory into LDS, no staging registers and no ds_write).  In a register-staged kernel on the same tiles a quarter of the matrix-core
// time was lost around the register -> LDS stores (59.6 -> 66.2 TF
// without them, 67.7 with MFMAs and fragment reads alone, which is the f64 MFMA rate at the sustained clock).
// A DMA instruction writes the 64 lanes' 16-byte pieces to CONTIGUOUS LDS (1 KiB), so a tile row is exactly its 16
// doubles (128 bytes, no padding) and bank conflicts are avoided by a swizzle instead: the piece that lies in 16-byte
// slot s of row R is k-piece s ^ ((R >> 1) & 7) -- chosen on the global side, where every lane may fetch what it likes.
// A fragment read (16 rows x 4 lane groups, ds_read_b128) then touches 16 different slots of the 256-byte bank window in
// each of its four lane groups.  Triangular operands: masked on the fragments of the k-tiles that cross the diagonal.
// MFMA tiles per wave along M and N: <2,2> -> 64 x 64 output tile per workgroup, <4,4> -> 128 x 128 (twice the flop per
// operand byte), <4,2> -> 128 x 64 (10.7 instead of 8 flop per operand byte at three workgroups per CU: for the products
// with two triangular operands, where the 128 x 128 form loses to its tails)
template <int TWM, int TWN = TWM>
__global__ __launch_bounds__(256, (TWM == 4 && TWN == 4) ? 2 : (TWM == 4 || TWN == 4) ? 3 : 4)
void gemm_nt_f64_dma_kernel(GemmArgs g)
{
    constexpr int BK = 16;
    constexpr int BM = 32 * TWM, BN = 32 * TWN;               // shadow the file-level 64 x 64
    constexpr int PWA = BM / 8 / 4, PWB = BN / 8 / 4;         // 1 KiB DMA pieces (8 tile rows) per wave and operand
    constexpr int OPA = BM * BK * (int)sizeof(double), OPB = BN * BK * (int)sizeof(double);       // bytes of the operand tiles
    typedef double double2_t __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_gemm_smem[];   // [2][A | B]
    const int ti = g.walk == WALK_COLUMNS_REVERSED ? (int)blockIdx.x : g.walk == WALK_ROWS_REVERSED ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.y + g.row0;
    const int tj = g.walk == WALK_COLUMNS_REVERSED ? (int)(gridDim.y - 1 - blockIdx.y) : (int)blockIdx.x;
    if (g.lowerOnly && tj * BN >= (ti + 1) * BM) return;       // the tile lies entirely above the diagonal
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    unsigned char* const smem = dca_gemm_smem;

    int kLo = 0, kHi = g.K;
    if (g.maskA == MASK_LOWER) kHi = min(kHi, (ti + 1) * BM);
    if (g.maskA == MASK_UPPER) kLo = max(kLo, ti * BM);
    if (g.maskB == MASK_LOWER) kHi = min(kHi, (tj + 1) * BN);
    if (g.maskB == MASK_UPPER) kLo = max(kLo, tj * BN);
    kLo = kLo / BK * BK;
    const int nk = (kHi - kLo + BK - 1) / BK;

    double4_t acc[TWM][TWN];
#pragma unroll
    for (int m = 0; m < TWM; ++m)
#pragma unroll
        for (int n = 0; n < TWN; ++n) acc[m][n] = (double4_t){0.0, 0.0, 0.0, 0.0};

    // DMA role of the lane: pieces PW wave .. PW wave + PW - 1 of each operand (piece = 8 tile rows); row-in-piece lane >> 3,
    // slot lane & 7.  Rows past the end of the operand (M, N multiples of 64, not of 128) are fetched from its last row:
    // their results are not stored.
    const double* srcA[PWA];
    const double* srcB[PWB];
#pragma unroll
    for (int i = 0; i < PWA; ++i) {
        const int R = 8 * (PWA * wave + i) + (lane >> 3);
        const int piece = (lane & 7) ^ ((R >> 1) & 7);
        srcA[i] = g.A + (size_t)min(ti * BM + R, g.M - 1) * g.lda + 2 * piece;
    }
#pragma unroll
    for (int i = 0; i < PWB; ++i) {
        const int R = 8 * (PWB * wave + i) + (lane >> 3);
        const int piece = (lane & 7) ^ ((R >> 1) & 7);
        srcB[i] = g.B + (size_t)min(tj * BN + R, g.N - 1) * g.ldb + 2 * piece;
    }
    auto issue = [&](int buf, int k0) {
#pragma unroll
        for (int i = 0; i < PWA; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcA[i] + k0),
                                             (__attribute__((address_space(3))) void*)(smem + buf * (OPA + OPB) + (PWA * wave + i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < PWB; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcB[i] + k0),
                                             (__attribute__((address_space(3))) void*)(smem + buf * (OPA + OPB) + OPA + (PWB * wave + i) * 1024), 16, 0, 0);
    };
    const int fr = lane & 15, fg = lane >> 4, swz = (fr >> 1) & 7;
    auto mma_tile = [&](int buf, int k0) {
        const unsigned char* as = smem + buf * (OPA + OPB);
        const unsigned char* bs = as + OPA;
        const bool diagA = g.maskA != MASK_NONE && k0 + BK > ti * BM && k0 < (ti + 1) * BM;    // wave-uniform
        const bool diagB = g.maskB != MASK_NONE && k0 + BK > tj * BN && k0 < (tj + 1) * BN;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const int slot = (4 * kk + fg) ^ swz;             // lane group fg holds k = 8 kk + 2 fg, + 1
            double2_t a[TWM], b[TWN];
#pragma unroll
            for (int m = 0; m < TWM; ++m) a[m] = *reinterpret_cast<const double2_t*>(as + (wm * 16 * TWM + 16 * m + fr) * 128 + slot * 16);
#pragma unroll
            for (int m = 0; m < TWN; ++m) b[m] = *reinterpret_cast<const double2_t*>(bs + (wn * 16 * TWN + 16 * m + fr) * 128 + slot * 16);
            if (diagA || diagB) {
                // only the 16-row fragments whose rows the 8 k values of this slab actually cross need the per-element test
                // (wave-uniform per fragment): the masking is vector-ALU work in front of the MFMAs
                const int kmin = k0 + 8 * kk, kmax = kmin + 7;
#pragma unroll
                for (int m = 0; m < TWM; ++m) {
                    const int aBase = ti * BM + wm * 16 * TWM + 16 * m;
                    const bool needA = diagA && ((g.maskA == MASK_UPPER && kmin < aBase + 15) || (g.maskA == MASK_LOWER && kmax > aBase));
                    if (needA) {
                        const int aRow = aBase + fr;
                        const int aLo = g.maskA == MASK_UPPER ? aRow : INT_MIN, aHi = g.maskA == MASK_LOWER ? aRow : INT_MAX;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int k = kmin + 2 * fg + h;
                            a[m][h] = (k < aLo || k > aHi) ? 0.0 : a[m][h];
                        }
                    }
                }
#pragma unroll
                for (int m = 0; m < TWN; ++m) {
                    const int bBase = tj * BN + wn * 16 * TWN + 16 * m;
                    const bool needB = diagB && ((g.maskB == MASK_UPPER && kmin < bBase + 15) || (g.maskB == MASK_LOWER && kmax > bBase));
                    if (needB) {
                        const int bRow = bBase + fr;
                        const int bLo = g.maskB == MASK_UPPER ? bRow : INT_MIN, bHi = g.maskB == MASK_LOWER ? bRow : INT_MAX;
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int k = kmin + 2 * fg + h;
                            b[m][h] = (k < bLo || k > bHi) ? 0.0 : b[m][h];
                        }
                    }
                }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int m = 0; m < TWM; ++m)
#pragma unroll
                    for (int n = 0; n < TWN; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][h], b[n][h], acc[m][n], 0, 0, 0);
        }
    };

    if (nk > 0) issue(0, kLo);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        const int buf = t & 1;
        if (t + 1 < nk) issue(buf ^ 1, kLo + (t + 1) * BK);
        mma_tile(buf, kLo + t * BK);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's pieces of the next tile have landed
        __syncthreads();                                       // ... everyone's; and the tile just used may be overwritten
    }

#pragma unroll
    for (int m = 0; m < TWM; ++m)
#pragma unroll
        for (int n = 0; n < TWN; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = ti * BM + wm * 16 * TWM + m * 16 + (lane >> 4) + 4 * r;
                const int j = tj * BN + wn * 16 * TWN + n * 16 + (lane & 15);
                if (i >= g.M || j >= g.N) continue;
                if (g.lowerOnly && j > i) continue;
                double v = g.alpha * acc[m][n][r];
                double* cp = g.C + (size_t)i * g.ldc + j;
                if (g.beta != 0.0) v += g.beta * (g.Cin ? g.Cin[(size_t)i * g.ldcin + j] : *cp);
                *cp = v;
                if (g.Cm && !(g.lowerOnly && i == j)) g.Cm[(size_t)j * g.ldcm + i] = v;
            }
}

// ---------------------------------------------------------------------------------------------------------------
// The diagonal leaves: A (lower triangle valid) -> X = inv(chol(A)), written lower + mirrored upper, one workgroup per leaf.
// 1 / sqrt(pivot): hardware seed, DCA_RSQ_NEWTON Newton steps and a step on the residual.
#ifndef DCA_RSQ_NEWTON
#define DCA_RSQ_NEWTON 1        // + the residual step: 7e-16 against LAPACK with 1 as with 2 (tools/experiments/inv_err.py)
#endif
__device__ __forceinline__ double rsqrt_refined(double a)
{
    double y = __builtin_amdgcn_rsq(a);
#pragma unroll
    for (int it = 0; it < DCA_RSQ_NEWTON; ++it) {
        const double h = 0.5 * y;
        const double e = __builtin_fma(-a * y, y, 1.0);     // 1 - a y^2
        y = __builtin_fma(h, e, y);
    }
    // last step on the residual of s = a y: one more correct digit than another Newton step on y
    const double sq = a * y;
    const double res = __builtin_fma(-sq, sq, a);
    return __builtin_fma(0.5 * y * y, res * y, y);          // y + y^3 (a - s^2) / 2
}

// Barrier of the leaf's steps: what the waves exchange goes through LDS, so only the LDS counter is drained.  __syncthreads()
// also waits for the global stores of the finished X rows, which nobody in the kernel reads.
__device__ __forceinline__ void leaf_step_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The leaf in steps of SIXTEEN columns (round 6; NB = 64 or 128: with halves in multiples of 128 the recursion meets no other).
// The leaves of rounds 1 - 5 advanced four columns per step: two workgroup barriers, three LDS round trips and the 4 x 4 diagonal
// block factored by ONE lane (600 ns) for every four columns -- 1.44 us per step, 46 us per 128 columns, and with 8 x 189
// registers such a leaf needed a CU of its own.  Here a step is one 16-column tile column T:
//   1. [D16 = inv(chol(C(T,T))) is in LDS]  L(i,T) = C(i,T) D16^T for the tile rows below (4 MFMAs per tile, operands through
//      LDS), X(T,j) = D16 B(T,j) for the tiles left of the diagonal (4 MFMAs on the owner's own accumulators -- the
//      accumulator layout IS the B-operand layout), X(T,T) = D16; X rows go to memory, all of it to the `panel` buffer;
//   2. the tiles of column T+1 take their rank-16 update first and publish themselves (next diagonal tile, next column);
//   3. wave 0 factors and inverts the next diagonal tile WHILE the other waves update the remaining tiles.
// The 16 x 16 diagonal tile is done by one WAVE with one matrix row per lane (registers, v_readlane broadcasts of the pivot
// row, no LDS, no barrier): Gaussian elimination of [S | I] with the multipliers s_rk / p_k (reciprocal: one seed + one
// cubic correction, 4 dependent operations) leaves the inverse of the unit factor in the right half, scaled at the end by
// 1 / sqrt(p_r).  Per column the dependent chain is 7 operations instead of ~11 per column of the one-lane 4 x 4 form.
// Seven worker waves + the chain wave; NB <= 128 fits in 128 registers per lane (a CU that runs one of the sweep's update
// workgroups still has room for it).  NB = 256 (136 tiles) needed 256 and measured slower.
__device__ __forceinline__ double lane_bcast(double v, int src)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double rcp_cubic(double a)
{
    // v_rcp_f64 is good to ~2^-23; y (1 + e + e^2), e = 1 - a y, leaves e^3 ~ 2^-69
    const double y = __builtin_amdgcn_rcp(a);
    const double e = __builtin_fma(-a, y, 1.0);
    const double t = __builtin_fma(e, e, e);
    return __builtin_fma(y, t, y);
}
// S: 16 x 16 symmetric tile in LDS (row-major, both halves); D <- inv(chol(S)) (lower, zeros above).  One whole wave.
// One COLUMN of [S | I] per lane (lanes 0 .. 15 the columns of S, 16 .. 31 those of the right half): eliminating column k
// is  v[r] -= m_r v[k]  in every lane, with the multipliers m_r = S[r][k] / p_k formed in lane k and broadcast -- 15 - k
// broadcasts per column serve both halves (one matrix ROW per lane needed 16: the pivot row of both halves).
__device__ __forceinline__ void factor16(const double* __restrict__ S, double* __restrict__ D, int lane, int* __restrict__ info, int pivot0)
{
    const int c = lane & 15;
    const bool right = (lane & 16) != 0;
    double v[16], rs[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const double sv = S[c * 16 + r];                    // column c = row c
        v[r] = right ? (r == c ? 1.0 : 0.0) : sv;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const double p = lane_bcast(v[k], k);
        if (!(p > 0.0) && lane == 0) atomicCAS(info, 0, pivot0 + k + 1);
        const double ik = rcp_cubic(p);
        rs[k] = lane_bcast(rsqrt_refined(p), 0);            // beside the chain; uniform: kept in scalar registers
#pragma unroll
        for (int r = k + 1; r < 16; ++r) {
            const double m = lane_bcast(v[r] * ik, k);
            v[r] = __builtin_fma(-m, v[k], v[r]);
        }
    }
    if (lane >= 16 && lane < 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) D[r * 16 + c] = (r >= c) ? rs[r] * v[r] : 0.0;
    }
}

#ifndef DCA_LEAF16_ABLATE
#define DCA_LEAF16_ABLATE 0      // tools/experiments/leaf16_bench.hip, timing only: 1 no diagonal tiles, 2 no panel, 4 no updates, 8 no X stores
#endif
template <int NB>
__device__ __forceinline__ void cholinv_leaf16_body(double* __restrict__ M, int ld, int pivotBase, int* __restrict__ info)
{
    DCA_CHAIN_PRIO();
    constexpr int NT = NB / 16;
    constexpr int NTILES = NT * (NT + 1) / 2;
    constexpr int WORKERS = 7;
    constexpr int SLOTS = (NTILES + WORKERS - 1) / WORKERS;
    constexpr int PS = NB + 2;                        // row stride of the k-major buffers (doubles)
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_gemm_smem[];
    double* const colbuf = reinterpret_cast<double*>(dca_gemm_smem);        // [16][PS]: C(i, T) of the tile rows below T, [column][row]
    double* const panel = colbuf + 16 * PS;                                 // [16][PS]: [m][idx] = X(T, idx)[m] up to the tile, L(idx, T)[m] below
    double* const diagbuf = panel + 16 * PS;                                // [16][16]: the next diagonal tile
    double* const dinv = diagbuf + 256;                                     // [16][16]: D16
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lc = lane & 15, lr = lane >> 4;

    if (wave == 0) {
        // the chain wave: nothing but the diagonal tiles (same barriers as the workers below)
        __syncthreads();
        factor16(diagbuf, dinv, lane, info, pivotBase);
        leaf_step_barrier();
#pragma unroll 1
        for (int T = 0; T < NT; ++T) {
            leaf_step_barrier();
            if (T + 1 == NT) break;
            if (!(DCA_LEAF16_ABLATE & 1)) factor16(diagbuf, dinv, lane, info, pivotBase + 16 * (T + 1));
            leaf_step_barrier();
        }
        return;
    }

    int tI[SLOTS], tJ[SLOTS];
    double4_t acc[SLOTS];
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int t = wave - 1 + sl * WORKERS;
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
        tI[sl] = t < NTILES ? ti : -1;
        tJ[sl] = t - ti * (ti + 1) / 2;
        acc[sl] = (double4_t){0.0, 0.0, 0.0, 0.0};
        if (tI[sl] >= 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ti + lr + 4 * r, j = 16 * tJ[sl] + lc;
                acc[sl][r] = M[(size_t)max(i, j) * ld + min(i, j)];          // diagonal tiles: the full symmetric tile
            }
        }
    }
    // the tiles of column T1 BELOW the diagonal publish themselves as C(i, T1) and start over as B(i, T1) = 0
    auto publish_column = [&](int T1) {
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (tI[sl] <= T1 || tJ[sl] != T1) continue;                      // wave-uniform (also passes over empty slots: -1)
#pragma unroll
            for (int r = 0; r < 4; ++r) colbuf[lc * PS + 16 * tI[sl] + lr + 4 * r] = acc[sl][r];
            acc[sl] = (double4_t){0.0, 0.0, 0.0, 0.0};
        }
    };
    auto publish_diag = [&](int sl) {
#pragma unroll
        for (int r = 0; r < 4; ++r) diagbuf[(lr + 4 * r) * 16 + lc] = acc[sl][r];
    };
    auto update = [&](int sl) {
        const int i0 = 16 * tI[sl], j0 = 16 * tJ[sl];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const double a = -panel[(4 * kk + lr) * PS + i0 + lc];
            const double b = panel[(4 * kk + lr) * PS + j0 + lc];
            acc[sl] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[sl], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);          // one tile's operands at a time: hoisting every slot's LDS reads costs more registers than a wave has
    };
    auto panel_row = [&](int i) {                   // L(i, T) = C(i, T) D16^T -> panel
        double4_t l = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            l = __builtin_amdgcn_mfma_f64_16x16x4f64(colbuf[(4 * kk + lr) * PS + 16 * i + lc], dinv[lc * 16 + 4 * kk + lr], l, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) panel[lc * PS + 16 * i + lr + 4 * r] = l[r];
        __builtin_amdgcn_sched_barrier(0);
    };
    // rows 16 T .. 16 T + 15 of X (final: they stand in `panel`) go to memory, lower part and mirror; all worker lanes, no per-tile addresses
    auto store_x_rows = [&](int T) {
        if (DCA_LEAF16_ABLATE & 8) return;
        const int W = 16 * (T + 1);
#pragma unroll 1
        for (int e = tid - 64; e < 16 * W; e += 64 * WORKERS) {
            const int m = e / W, col = e - m * W, row = 16 * T + m;
            const double x = panel[m * PS + col];
            if (col <= row) {
                M[(size_t)row * ld + col] = x;
                if (col < row) M[(size_t)col * ld + row] = x;
            }
        }
    };
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl)
        if (tI[sl] == 0) publish_diag(sl);
    publish_column(0);
    __syncthreads();
    leaf_step_barrier();

#pragma unroll 1
    for (int T = 0; T < NT; ++T) {
        // ---- A. the panel of the step.  The owner of the NEXT diagonal tile makes that tile's row of the panel itself, updates the
        // tile and publishes it: the chain wave waits for nothing else
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (tI[sl] != T + 1 || tJ[sl] != T + 1) continue;
            if (!(DCA_LEAF16_ABLATE & 2)) panel_row(T + 1);
            update(sl);                                                      // reads what this wave has just written (LDS keeps a wave's order)
            publish_diag(sl);
        }
#pragma unroll 1
        for (int i = T + 1 + wave; i < NT && !(DCA_LEAF16_ABLATE & 2); i += WORKERS) panel_row(i);
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl) {
            if (tI[sl] != T) continue;
            double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
            if (tJ[sl] < T) {
#pragma unroll
                for (int r = 0; r < 4; ++r) x = __builtin_amdgcn_mfma_f64_16x16x4f64(dinv[lc * 16 + lr + 4 * r], acc[sl][r], x, 0, 0, 0);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = dinv[(lr + 4 * r) * 16 + lc];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) panel[(lr + 4 * r) * PS + 16 * tJ[sl] + lc] = x[r];
            __builtin_amdgcn_sched_barrier(0);
        }
        leaf_step_barrier();
        if (T + 1 == NT) break;
        // ---- B. everybody's updates, column T + 1 first (wave 0 factors the next diagonal tile meanwhile)
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
            if (tI[sl] > T + 1 && tJ[sl] == T + 1) update(sl);
        publish_column(T + 1);
#pragma unroll
        for (int sl = 0; sl < SLOTS; ++sl)
            if (tI[sl] > T && tJ[sl] != T + 1 && !(DCA_LEAF16_ABLATE & 4)) update(sl);      // (T + 1, T + 1) is in column T + 1: done in A
        store_x_rows(T);
        leaf_step_barrier();
    }
    store_x_rows(NT - 1);
}
// 144 registers: two of its waves per SIMD next to one wave of an update workgroup (224)
template <int NB>
__global__ __launch_bounds__(512) __attribute__((amdgpu_num_vgpr(144)))
void cholinv_leaf16_small_kernel(double* __restrict__ M, int ld, int pivotBase, int* __restrict__ info) { cholinv_leaf16_body<NB>(M, ld, pivotBase, info); }
template <int NB> constexpr size_t leaf16_lds_bytes() { return (size_t)(2 * 16 * (NB + 2) + 512) * sizeof(double); }

struct Arena {
    double* base; size_t cap, top = 0;
    double* alloc(size_t n) { if (top + n > cap) return nullptr; double* p = base + top; top += n; return p; }
};

// Dynamic LDS sizes above the default limit need an attribute per kernel AND PER DEVICE; set for all of them the first time an
// inverse runs on a device (contexts may live on several host threads and several devices).
int gemm_kernels_prepare(int device)
{
    static std::mutex mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(mu);
    for (int d : done) if (d == device) return DCA_OK;
    const int small = (int)((size_t)2 * (32 + 32) * (64 + 2) * sizeof(double));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_f64_dma_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 128 * 16 * 8));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_f64_dma_kernel<4, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (128 + 64) * 16 * 8));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_f64_small_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, small));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_nt_f64_small_pair_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, small));
    done.push_back(device);
    return DCA_OK;
}

// Background form of a product (side stream of the recursion): 128 x 128 tiles, issued as bands of tile rows of at most
// `maxWGs` workgroups each.  MI355X places one such workgroup per CU before it doubles up, so a launch of fewer
// workgroups than CUs leaves whole CUs to the kernels of another stream: the chain of single-workgroup leaves and
// few-tile products of a subtree runs next to it at its own pace (tools/experiments/overlap_bench.hip: 200 leaves
// 45.6 us each alone, 45.7 next to 255-workgroup launches that sustain 54 TF, 49 -- and the product at 25 TF -- next to
// 256).  WALK_ROWS only.
int launch_gemm_banded(dca_ctx* ctx, hipStream_t stream, GemmArgs g, int maxWGs)
{
    const int gx = (g.N + 127) / 128, gy = (g.M + 127) / 128;
    const int band = chol_band_rows(g.N, maxWGs);
    for (int r = 0; r < gy; r += band) {
        g.row0 = r;
        hipLaunchKernelGGL(gemm_nt_f64_dma_kernel<4>, dim3(gx, std::min(band, gy - r)), dim3(256), (size_t)6 * 128 * 16 * sizeof(double), stream, g);
    }
    HIP_TRY(hipGetLastError());
    return DCA_OK;
}

// The bound on the tiles of a 32 x 32 product (cholinv_plan.h): the block sweep lowers it for the launches it makes
thread_local int tl_small32_max = -1;
static int small32_max() { return tl_small32_max >= 0 ? tl_small32_max : kSmall32Max; }
static dim3 grid64(const GemmArgs& g) { return g.walk == WALK_COLUMNS_REVERSED ? dim3(g.M / BM, g.N / BN) : dim3(g.N / BN, g.M / BM); }

// both products on 32 x 32 tiles in ONE launch when each is small enough for that kernel; false: launch them one by one
bool launch_gemm_small_pair(dca_ctx* ctx, const GemmArgs& a, const GemmArgs& b)
{
    if (!chol_pair_fits(a.M, a.N, b.M, b.N, small32_max())) return false;
    const dim3 ga = grid64(a), gb = grid64(b);
    const size_t lds = (size_t)2 * (32 + 32) * (64 + 2) * sizeof(double);
    const dim3 grid(std::max(ga.x, gb.x) * 2, std::max(ga.y, gb.y) * 2, 2);
    hipLaunchKernelGGL(gemm_nt_f64_small_pair_kernel, grid, dim3(256), lds, ctx->stream, a, (int)ga.x * 2, (int)ga.y * 2, b, (int)gb.x * 2, (int)gb.y * 2);
    return true;
}

int launch_gemm_on(hipStream_t stream, const GemmArgs& g)
{
    const dim3 grid = grid64(g);
    const int gx = (int)(grid.x + 1) / 2, gy = (int)(grid.y + 1) / 2;
    switch (chol_product_form(g.M, g.N, g.maskA, g.maskB, g.lowerOnly, g.walk, small32_max())) {
    case CHOL_SMALL32: {
        dim3 g32(grid.x * 2, grid.y * 2);
        const size_t lds = (size_t)2 * (32 + 32) * (64 + 2) * sizeof(double);
        hipLaunchKernelGGL(gemm_nt_f64_small_kernel, g32, dim3(256), lds, stream, g);
        break;
    }
    case CHOL_DMA128x64:       // grid.y counts 128-row tiles
        hipLaunchKernelGGL((gemm_nt_f64_dma_kernel<4, 2>), dim3(grid.x, gy), dim3(256), (size_t)2 * (128 + 64) * 16 * sizeof(double), stream, g);
        break;
    case CHOL_DMA128: {
        dim3 grid128(gx, gy);
        if (g.walk == WALK_COLUMNS_REVERSED) grid128 = dim3((g.M + 127) / 128, (g.N + 127) / 128);
        hipLaunchKernelGGL(gemm_nt_f64_dma_kernel<4>, grid128, dim3(256), (size_t)4 * 128 * 16 * sizeof(double), stream, g);
        break;
    }
    default:
        hipLaunchKernelGGL(gemm_nt_f64_dma_kernel<2>, grid, dim3(256), (size_t)4 * 64 * 16 * sizeof(double), stream, g);
    }
    return DCA_OK;
}
int launch_gemm(dca_ctx* ctx, const GemmArgs& g) { return launch_gemm_on(ctx->stream, g); }

// Side streams: the fused recursion runs its top-level T^T on the first, the block sweep picks two of them (or of `extra`); the
// context's own stream carries the critical path.
constexpr int kSideDepths = DCA_SIDE_DEPTHS;
// Stream and event creation costs about a millisecond each -- more than the whole inverse of a small matrix -- so the sets are
// made once per process and device and lent to one inverse at a time (contexts of several host threads get a set each).
struct SideSet {
    hipStream_t s[kSideDepths] = {};
    // the sweep's two side streams, PROBED to run concurrently with the context's stream and with each other (see sweep_streams)
    std::vector<hipStream_t> extra;
    hipStream_t selFor = nullptr, selRest = nullptr, selSide = nullptr;
    int* probe = nullptr;             // pinned host memory: flag, result
    hipEvent_t fork = nullptr, join = nullptr;      // of the recursion's background product
    int device = -1;
    bool busy = false;
};
std::mutex g_sideMu;
std::vector<SideSet*> g_sideSets;          // never destroyed: the HIP runtime may be gone at exit

SideSet* side_set_acquire(int device)
{
    std::lock_guard<std::mutex> lk(g_sideMu);
    for (SideSet* S : g_sideSets)
        if (S->device == device && !S->busy) { S->busy = true; return S; }
    SideSet* S = new SideSet();
    S->device = device;
    // plain streams: with stream priorities (context stream highest, these lowest) the chain's few-tile products ran 3 - 10
    // times slower whenever a side stream had work (10-workgroup launches at depth 2 cost the inverse 10 ms)
    bool good = hipEventCreateWithFlags(&S->fork, hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&S->join, hipEventDisableTiming) == hipSuccess;
    for (int d = 0; d < kSideDepths && good; ++d) good = hipStreamCreateWithFlags(&S->s[d], hipStreamNonBlocking) == hipSuccess;
    if (!good) { delete S; return nullptr; }      // the products then run in line
    S->busy = true;
    g_sideSets.push_back(S);
    return S;
}
void side_set_release(SideSet* S)
{
    if (!S) return;
    std::lock_guard<std::mutex> lk(g_sideMu);
    S->busy = false;
}

// The fused recursion of the head of the file.  side: the set whose first stream takes this node's T^T (the top level of a
// whole matrix only: the nodes below and the sweep's pivot blocks pass none).
int cholinv_rec(dca_ctx* ctx, double* M, int ld, int n, int pivotBase, Arena& ws, int* dInfo, SideSet* side)
{
    if (chol_leaf(n) == 64) { hipLaunchKernelGGL(cholinv_leaf16_small_kernel<64>, dim3(1), dim3(512), leaf16_lds_bytes<64>(), ctx->stream, M, ld, pivotBase, dInfo); return DCA_OK; }
    if (chol_leaf(n) == 128) { hipLaunchKernelGGL(cholinv_leaf16_small_kernel<128>, dim3(1), dim3(512), leaf16_lds_bytes<128>(), ctx->stream, M, ld, pivotBase, dInfo); return DCA_OK; }
    const int n1 = chol_split(n), n2 = n - n1;
    double* M11 = M;
    double* M12 = M + n1;
    double* M21 = M + (size_t)n1 * ld;
    double* M22 = M + (size_t)n1 * ld + n1;
    DCA_TRY(cholinv_rec(ctx, M11, ld, n1, pivotBase, ws, dInfo, nullptr));
    const size_t mark = ws.top;
    double* L21 = ws.alloc((size_t)n2 * n1);
    double* Tt = ws.alloc((size_t)n1 * n2);
    if (!L21 || !Tt) { dca_set_error("cholinv workspace exhausted"); return DCA_ERR_NOMEM; }
    // L21 = A21 * X11^T : C[i][j] = sum_k A21[i][k] * X11[j][k],  X11 lower (k <= j)
    DCA_TRY(launch_gemm(ctx, GemmArgs{M21, ld, MASK_NONE, M11, ld, MASK_LOWER, L21, n1, nullptr, 0, n2, n1, n1, 1.0, 0.0, 0, WALK_COLUMNS_REVERSED}));
    // A22 -= L21 * L21^T (lower tiles); at the lower levels together with T^T in one launch
    const GemmArgs syrkArgs{L21, n1, MASK_NONE, L21, n1, MASK_NONE, M22, ld, nullptr, 0, n2, n2, n1, -1.0, 1.0, 1};
    const GemmArgs ttArgs{M11, ld, MASK_UPPER, L21, n1, MASK_NONE, Tt, n2, nullptr, 0, n1, n2, n1, 1.0, 0.0, 0};
    const bool paired = launch_gemm_small_pair(ctx, syrkArgs, ttArgs);
    // T^T[j][i] = sum_k X11^T[j][k] * L21[i][k];  X11^T rows are the mirrored upper part of M11 (k >= j).  It needs X11 and
    // L21 only, so at the top level it runs on a side stream NEXT TO the A22 subtree, whose chain of leaves and few-tile
    // products leaves the chip idle -- as launches of fewer workgroups than CUs (launch_gemm_banded), which is what makes the
    // overlap work: full-grid launches on a side stream (round 1) and CU-masked streams (round 2) had gained nothing.
    const bool onSide = chol_fork_side(paired, side != nullptr, n1);
    // Once the background product is in flight, NO path may leave this frame without joining it: it writes Tt in the
    // arena, and the caller hands the side set back and may reuse or free the workspace as soon as this returns.  On
    // an error below, the side stream is drained on the host before the error is passed on.
    bool inFlight = false;
    auto bail = [&](int rc) -> int {
        if (inFlight) hipStreamSynchronize(side->s[0]);
        ws.top = mark;
        return rc;
    };
    int rc = DCA_OK;
    if (onSide) {
        // the fork comes BEFORE the SYRK: that product's 820 lower 128 x 128 tiles fill 512 slots 1.6 times (47 TF), and the
        // background bands take what its ragged second round leaves idle
        auto fork_side = [&]() -> int {
            HIP_TRY(hipEventRecord(side->fork, ctx->stream));                  // L21 (and X11) are complete
            HIP_TRY(hipStreamWaitEvent(side->s[0], side->fork, 0));
            DCA_TRY(launch_gemm_banded(ctx, side->s[0], ttArgs, kSideWGs));
            inFlight = true;
            HIP_TRY(hipEventRecord(side->join, side->s[0]));
            return DCA_OK;
        };
        if ((rc = fork_side()) != DCA_OK) return bail(rc);
    }
    if (!paired && (rc = launch_gemm(ctx, syrkArgs)) != DCA_OK) return bail(rc);
    if ((rc = cholinv_rec(ctx, M22, ld, n2, pivotBase + n1, ws, dInfo, nullptr)) != DCA_OK) return bail(rc);
    if (onSide) {
        if (hipStreamWaitEvent(ctx->stream, side->join, 0) != hipSuccess) { dca_set_error("cholinv: join of the side stream failed"); return bail(DCA_ERR_HIP); }
    } else if (!paired) DCA_TRY(launch_gemm(ctx, ttArgs));
    // X21[i][j] = -sum_k X22[i][k] * T^T[j][k];  X22 lower (k <= i); mirrored into the (1,2) block
    DCA_TRY(launch_gemm(ctx, GemmArgs{M22, ld, MASK_LOWER, Tt, n2, MASK_NONE, M21, ld, M12, ld, n2, n1, n2, -1.0, 0.0, 0, WALK_ROWS_REVERSED}));
    ws.top = mark;
    return DCA_OK;
}

// Events of the block sweep's three streams, made as they are first asked for.
struct EventPool {
    std::vector<hipEvent_t> ev;
    hipEvent_t get(size_t i)
    {
        while (ev.size() <= i) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            ev.push_back(e);
        }
        return ev[i];
    }
};
std::mutex g_poolMu;
std::vector<std::pair<SideSet*, EventPool*>> g_eventPools;     // one pool per side set, never destroyed (as the sets)
EventPool* event_pool_of(SideSet* S)
{
    std::lock_guard<std::mutex> lk(g_poolMu);
    for (auto& p : g_eventPools) if (p.first == S) return p.second;
    g_eventPools.emplace_back(S, new EventPool());
    return g_eventPools.back().second;
}

// DCA_CHOLINV_TRACE=1 (measurement aid): timing events on the streams of the block sweep -- the kernel trace of the
// profiler serialises the queues, these do not.  Printed to stderr when the inverse has finished.
struct StepTrace {
    bool on = false;
    std::vector<std::pair<std::string, hipEvent_t>> marks;
    ~StepTrace() { for (auto& m : marks) hipEventDestroy(m.second); }      // an early return does not leak the events
    void mark(hipStream_t st, const char* what, int j)
    {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        hipEventRecord(e, st);
        marks.emplace_back(std::string(what) + " " + std::to_string(j), e);
    }
    void dump()
    {
        if (!on || marks.empty()) return;
        hipDeviceSynchronize();
        for (size_t i = 0; i < marks.size(); ++i) {
            float ms = 0.f;
            hipEventElapsedTime(&ms, marks[0].second, marks[i].second);
            fprintf(stderr, "cholinv trace %9.1f us  %s\n", ms * 1e3, marks[i].first.c_str());
        }
        for (auto& m : marks) hipEventDestroy(m.second);
        marks.clear();
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Round 6: the inverse as a symmetric BLOCK SWEEP (block Gauss-Jordan on an SPD matrix).
//
// The three-phase forms (factorisation, triangular inverse, X^T X: the fused recursion above, and round 5's look-ahead blocked
// factorisation) are serial phases of which the first and
// the second run out of parallel work at their ends (a deep update of the look-ahead factorisation was 100 - 250 tiles)
// -- 33 / 53 / 58 TF at n = 10 048 where the GEMM alone sustains 69.  The sweep does the same n^3 flop in ONE phase whose
// every step is the same rank-w update of the WHOLE matrix.  With M symmetric (both halves stored), J the next w pivot
// columns and P = inv(M_JJ):
//     W      = M[:, J] P                       n x w x w
//     M[i,j] -= W[i, :] M[j, J]^T              every tile with i, j outside J  (lower tiles, mirrored: (n - w)^2 w flop)
//     M[:, J] = W,  M[J, :] = W^T,  M[J, J] = -P
// and after the last panel M = -inv(A) -- the couplings themselves.  M_JJ at the time its panel is swept is the Schur
// complement of the panels before it, so the pivots met are EXACTLY the pivots of the Cholesky factorisation of A: P comes
// from the same leaves (X = inv(chol(M_JJ)) by the fused recursion on the w x w block, P = X^T X) and a matrix that is not
// positive definite is reported with the same pivot index as before.
// Two streams.  The CHAIN (context stream) owns the diagonal: from P_p it forms the next pivot block itself,
//     S' = M[J', J'] - (M[J', J] P_p) M[J', J]^T   (three few-tile products), then X', P' ...
// and never waits for the bulk of its own step.  The BULK stream does W, then the tiles that the chain of the NEXT steps
// reads (column panel J' and the diagonal block after it: `prio`), then the rest, as PERSISTENT launches of at most `cap`
// workgroups of 128 x 128 tiles (one per CU, whole CUs stay free for the chain's kernels), every workgroup walking the
// tile list with stride `cap`; the list is ordered in bands of four tile rows so that the 31 workgroups that share an
// XCD's L2 work on a 4 x 8 block of tiles at a time (12 operand panels instead of 62).
enum { SWEEP_REST = 0, SWEEP_PRIO = 1 };
struct SweepArgs {
    const double* W; int ldw;      // n x w: the scaled panel
    const double* Q; int ldq;      // n x w: the pivot panel's columns as they were before the step (compact copy, all rows)
    double* M; int ld;             // n x n: the lower triangle is kept up to date
    int n, c, w;                   // pivot columns [c, c + w)
    int nt;                        // tile rows of M (128 rows each, the last one may be short)
    int skip0, skipN;              // tile rows left out: the pivot panel and the panel after it
    int mode;
    int pr0, prN;                  // SWEEP_PRIO: tile rows of the next panel
    int dg0, dgN;                  // diagonal block of the panel after the next: its lower tiles belong to PRIO, not to REST
    int nTiles;                    // length of the tile list (entries that decode to no tile are passed over)
    int* ctr;                      // 8 zeroed counters: the list is cut into 8 chunks, chunk x is handed out to the workgroups of XCD x first
};

// tile list entry t -> tile (ti, tj), tj <= ti
__device__ __forceinline__ bool sweep_tile_of(const SweepArgs& g, int t, int& ti, int& tj)
{
    const int nR = g.nt - g.skipN;
    if (g.mode == SWEEP_REST) {
        // lower triangle over the nR remaining tile rows in bands of 4 rows, column by column inside a band; band k starts at 8 k^2 + 2 k
        int k = (int)((sqrtf(4.f + 32.f * (float)t) - 2.f) * (1.f / 16.f));
        while (8 * (k + 1) * (k + 1) + 2 * (k + 1) <= t) ++k;
        while (8 * k * k + 2 * k > t) --k;
        const int u = t - (8 * k * k + 2 * k);
        int a, b;
        if (u < 16 * k) { b = u >> 2; a = 4 * k + (u & 3); }
        else {
            const int v = u - 16 * k;                          // the band's own 4 x 4 triangle, column by column
            const int col = v < 4 ? 0 : v < 7 ? 1 : v < 9 ? 2 : 3;
            const int row = v < 4 ? v : v < 7 ? v - 3 : v < 9 ? v - 5 : 3;
            a = 4 * k + row; b = 4 * k + col;
        }
        if (a >= nR) return false;
        ti = a < g.skip0 ? a : a + g.skipN;
        tj = b < g.skip0 ? b : b + g.skipN;
        if (g.dgN > 0 && tj >= g.dg0 && ti < g.dg0 + g.dgN) return false;      // tj <= ti: both inside the block
        return true;
    }
    const int rect = g.prN * nR;
    if (t < rect) {
        const int cc = g.pr0 + t % g.prN;
        int r = t / g.prN;
        r = r < g.skip0 ? r : r + g.skipN;
        ti = max(r, cc); tj = min(r, cc);
        return true;
    }
    const int u = t - rect;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= u) ++a;
    ti = g.dg0 + a; tj = g.dg0 + u - a * (a + 1) / 2;
    return true;
}

// 128 x 128 tiles, operands by LDS-DMA as in gemm_nt_f64_dma_kernel<4>; no triangular operand.  The accumulators START as
// -M[tile] (fetched while the first operand tiles are on their way) and the tile is stored as -acc: the read half of the
// read-modify-write costs no registers and no pass of its own.
// NST operand stages in LDS (32 KB each), NST - 1 of them in flight: every k-tile of 16 is a NEW 128-byte line of every
// operand row, so each step waits for a fetch that nobody has made before (the workgroups of an XCD walk k together, the
// first to ask misses the L2), and one workgroup per CU has nothing else to run meanwhile: with two stages the step took
// 2.5 us against 0.85 us of matrix-core time (round 6, first measurement: 82 us per K = 512 tile).
#ifndef DCA_SWEEP_ABLATE
#define DCA_SWEEP_ABLATE 0        // tools/experiments/sweep_bench.hip, timing only: 1 no load of the tile, 4 no store
#endif
template <int NST>
__global__ __launch_bounds__(256, 2)
void sweep_update_kernel(SweepArgs g)
{
    constexpr int BK = 16, TW = 4, BM = 128, BN = 128;
    constexpr int PW = BM / 8 / 4;
    constexpr int OP = BM * BK * (int)sizeof(double);
    typedef double double2_t __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_gemm_smem[];   // [NST][A | B]
    unsigned char* const smem = dca_gemm_smem;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int fr = lane & 15, fg = lane >> 4, swz = (fr >> 1) & 7;
    const int nk = g.w / BK;
    __shared__ int s_tile;
    int q = (int)blockIdx.x % 8, tries = 0;                         // thread 0: the chunk it draws from, chunks found empty

    for (;;) {
        if (tid == 0) {
            int t = -1;
            while (tries < 8) {
                const int lo = (int)((long long)g.nTiles * q / 8), hi = (int)((long long)g.nTiles * (q + 1) / 8);
                const int v = lo + atomicAdd(&g.ctr[q], 1);
                if (v < hi) { t = v; break; }
                q = (q + 1) & 7; ++tries;                           // own chunk done: help the next XCD's
            }
            s_tile = t;
        }
        __syncthreads();
        const int t = s_tile;
        __syncthreads();
        if (t < 0) break;
        int ti, tj;
        if (!sweep_tile_of(g, t, ti, tj)) continue;                 // the same for the whole workgroup
        // the tile itself first (oldest in the memory queue: landed when the first operand stage has)
        double4_t acc[TW][TW];
        const int iBase = ti * BM + wm * 64 + (lane >> 4), jBase = tj * BN + wn * 64 + (lane & 15);
#pragma unroll
        for (int m = 0; m < TW; ++m)
#pragma unroll
            for (int n = 0; n < TW; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = min(iBase + m * 16 + 4 * r, g.n - 1), j = min(jBase + n * 16, g.n - 1);
                    acc[m][n][r] = (DCA_SWEEP_ABLATE & 1) ? 0.0 : -g.M[(size_t)i * g.ld + j];
                }
        const double* srcA[PW];
        const double* srcB[PW];
#pragma unroll
        for (int i = 0; i < PW; ++i) {
            const int R = 8 * (PW * wave + i) + (lane >> 3);
            const int piece = (lane & 7) ^ ((R >> 1) & 7);
            srcA[i] = g.W + (size_t)min(ti * BM + R, g.n - 1) * g.ldw + 2 * piece;
            srcB[i] = g.Q + (size_t)min(tj * BN + R, g.n - 1) * g.ldq + 2 * piece;
        }
        auto issue = [&](int st, int k0) {
#pragma unroll
            for (int i = 0; i < PW; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcA[i] + k0),
                                                 (__attribute__((address_space(3))) void*)(smem + st * 2 * OP + (PW * wave + i) * 1024), 16, 0, 0);
#pragma unroll
            for (int i = 0; i < PW; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(srcB[i] + k0),
                                                 (__attribute__((address_space(3))) void*)(smem + st * 2 * OP + OP + (PW * wave + i) * 1024), 16, 0, 0);
        };
        // wait until at most `tiles` operand stages of this wave are still in flight (2 PW loads each)
        auto wait_stages = [&](int tiles) {
            if (tiles >= 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(6 * PW) : "memory");
            else if (tiles == 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(4 * PW) : "memory");
            else if (tiles == 1) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * PW) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        auto mma_tile = [&](int st) {
            const unsigned char* as = smem + st * 2 * OP;
            const unsigned char* bs = as + OP;
#pragma unroll
            for (int kk = 0; kk < BK / 8; ++kk) {
                const int slot = (4 * kk + fg) ^ swz;
                double2_t a[TW], b[TW];
#pragma unroll
                for (int m = 0; m < TW; ++m) a[m] = *reinterpret_cast<const double2_t*>(as + (wm * 64 + 16 * m + fr) * 128 + slot * 16);
#pragma unroll
                for (int m = 0; m < TW; ++m) b[m] = *reinterpret_cast<const double2_t*>(bs + (wn * 64 + 16 * m + fr) * 128 + slot * 16);
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int m = 0; m < TW; ++m)
#pragma unroll
                        for (int n = 0; n < TW; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][h], b[n][h], acc[m][n], 0, 0, 0);
            }
        };
        const int ahead = min(NST - 1, nk);
        for (int s = 0; s < ahead; ++s) issue(s, s * BK);
        wait_stages(ahead - 1);
        __syncthreads();
        for (int kt = 0, st = 0; kt < nk; ++kt) {
            const int nxt = kt + NST - 1;                             // its stage is the one tile kt - 1 used
            if (nxt < nk) issue(st == 0 ? NST - 1 : st - 1, nxt * BK);
            mma_tile(st);
            wait_stages(min(NST - 2, nk - kt - 2));                   // tile kt + 1 has landed
            __syncthreads();
            st = st == NST - 1 ? 0 : st + 1;
        }
        const bool diag = ti == tj;
        if (!(DCA_SWEEP_ABLATE & 4)) {
#pragma unroll
            for (int m = 0; m < TW; ++m)
#pragma unroll
                for (int n = 0; n < TW; ++n)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = iBase + m * 16 + 4 * r, j = jBase + n * 16;
                        if (i >= g.n || j >= g.n) continue;
                        if (diag && j > i) continue;
                        const double v = -acc[m][n][r];
                        g.M[(size_t)i * g.ld + j] = v;
                    }
        } else if (acc[0][0][0] == 1.2345e-300) g.M[0] = 0.0;
    }
}

// The swept panel in the lower triangle: M[i][c .. c + w) <- W[i] for the rows below the pivot block, M[c .. c + w)[j] <- W[j]^T
// for the columns left of it, the pivot block itself <- -P (32 x 32 pieces)
__global__ __launch_bounds__(256)
void sweep_finalize_kernel(double* __restrict__ M, int ld, int c, int w, const double* __restrict__ W, int ldw, const double* __restrict__ P, int ldp)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    if (r0 >= c + w) {
#pragma unroll
        for (int s = 0; s < 4; ++s) M[(size_t)(r0 + ty + 8 * s) * ld + c + k0 + tx] = W[(size_t)(r0 + ty + 8 * s) * ldw + k0 + tx];
        return;
    }
    if (r0 >= c) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = r0 + ty + 8 * s;
            M[(size_t)r * ld + c + k0 + tx] = -P[(size_t)(r - c) * ldp + k0 + tx];
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) tile[ty + 8 * s][tx] = W[(size_t)(r0 + ty + 8 * s) * ldw + k0 + tx];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) M[(size_t)(c + k0 + ty + 8 * s) * ld + r0 + tx] = tile[tx][ty + 8 * s];
}

// Q[i][k] = M[i][c + k] as the symmetric matrix has it, read from the LOWER triangle only: rows below the panel's diagonal
// block as they stand, rows above it from the row panel left of the block (transposed through LDS).  The rows of the block
// itself are copied as they stand (nothing reads them).
__global__ __launch_bounds__(256)
void gather_panel_kernel(const double* __restrict__ M, int ld, int c, int w, double* __restrict__ Q, int ldq)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int k0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    if (r0 >= c) {
#pragma unroll
        for (int s = 0; s < 4; ++s) Q[(size_t)(r0 + ty + 8 * s) * ldq + k0 + tx] = M[(size_t)(r0 + ty + 8 * s) * ld + c + k0 + tx];
        return;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) tile[ty + 8 * s][tx] = M[(size_t)(c + k0 + ty + 8 * s) * ld + r0 + tx];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) Q[(size_t)(r0 + ty + 8 * s) * ldq + k0 + tx] = tile[tx][ty + 8 * s];
}

// upper triangle <- transposed lower triangle, 32 x 32 pieces (the sweep's last pass: the result is bit-symmetric)
__global__ __launch_bounds__(256)
void symmetrize_kernel(double* __restrict__ M, int ld, int nb)
{
    __shared__ double tile[32][33];
    // piece (bi, bj), bj < bi, from the linear index of the strict lower triangle of pieces
    const int t = blockIdx.x;
    int bi = (int)((sqrtf(8.f * (float)t + 1.f) + 1.f) * 0.5f);
    while (bi * (bi - 1) / 2 > t) --bi;
    while ((bi + 1) * bi / 2 <= t) ++bi;
    const int bj = t - bi * (bi - 1) / 2;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) tile[ty + 8 * s][tx] = M[(size_t)(32 * bi + ty + 8 * s) * ld + 32 * bj + tx];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) M[(size_t)(32 * bj + ty + 8 * s) * ld + 32 * bi + tx] = tile[tx][ty + 8 * s];
}
// ... and inside the diagonal pieces
__global__ __launch_bounds__(256)
void symmetrize_diag_kernel(double* __restrict__ M, int ld)
{
    const int b = blockIdx.x;
    for (int e = threadIdx.x; e < 32 * 32; e += 256) {
        const int r = e >> 5, cc = e & 31;
        if (cc > r) M[(size_t)(32 * b + r) * ld + 32 * b + cc] = M[(size_t)(32 * b + cc) * ld + 32 * b + r];
    }
}

__global__ __launch_bounds__(256)
void copy_block_kernel(double* __restrict__ dst, int ldd, const double* __restrict__ src, int lds, int rows, int cols)
{
    typedef double double2_t __attribute__((ext_vector_type(2)));
    const int perRow = cols / 2;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < rows * perRow; e += gridDim.x * blockDim.x) {
        const int r = e / perRow, k = 2 * (e % perRow);
        *reinterpret_cast<double2_t*>(dst + (size_t)r * ldd + k) = *reinterpret_cast<const double2_t*>(src + (size_t)r * lds + k);
    }
}

__global__ __launch_bounds__(256)
void scale_matrix_kernel(double* __restrict__ M, size_t count, double f)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x) M[e] *= f;
}

// HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and two streams on one queue run one after the
// other.  The sweep needs three streams that really overlap (measured at n = 10 048 inside the mfDCA chain, where the
// process holds a dozen streams: 26.0 ms with the sweep's streams sharing queues, 19.4 ms with them apart), so it PROBES:
// a kernel on stream a waits (at most 300 us) for a flag that a kernel enqueued afterwards on stream b sets.
__global__ void probe_wait_kernel(int* flag, int* result, long long ticks)
{
    const long long t0 = wall_clock64();
    int seen = 0;
    while (wall_clock64() - t0 < ticks) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) { seen = 1; break; }
        __builtin_amdgcn_s_sleep(8);
    }
    __hip_atomic_store(result, seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void probe_set_kernel(int* flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

static bool streams_overlap(SideSet* S, hipStream_t a, hipStream_t b)
{
    if (a == b) return false;
    // flag and result live in pinned host memory the kernels reach directly: no memset / copy calls around the two launches
    if (!S->probe && hipHostMalloc(reinterpret_cast<void**>(&S->probe), 2 * sizeof(int), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); S->probe = nullptr; return true; }
    volatile int* h = S->probe;
    h[0] = 0; h[1] = 0;
    hipLaunchKernelGGL(probe_wait_kernel, dim3(1), dim3(1), 0, a, S->probe, S->probe + 1, 30000LL);      // wall clock: 100 MHz
    hipLaunchKernelGGL(probe_set_kernel, dim3(1), dim3(1), 0, b, S->probe);
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return true;
    return h[1] != 0;
}
// two streams of the set that overlap with `chain` and with each other (cached per chain stream); the set's first two if none are found
static void sweep_streams(SideSet* S, hipStream_t chain, hipStream_t& rest, hipStream_t& side)
{
    rest = S->s[0]; side = S->s[1];
    if (S->selFor == chain && S->selRest) { rest = S->selRest; side = S->selSide; return; }
    if (hipStreamSynchronize(chain) != hipSuccess) return;              // the probe's kernel must be the stream's next
    std::vector<hipStream_t> cand(S->s, S->s + kSideDepths);
    cand.insert(cand.end(), S->extra.begin(), S->extra.end());
    std::vector<hipStream_t> good;                                      // overlap with the chain
    for (size_t i = 0; good.size() < 2 && i < 16; ++i) {
        if (i >= cand.size()) {
            hipStream_t ns = nullptr;
            if (hipStreamCreateWithFlags(&ns, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
            S->extra.push_back(ns);
            cand.push_back(ns);
        }
        if (!streams_overlap(S, chain, cand[i])) continue;            // (two streams on one queue fail in whichever order they are asked)
        if (good.size() == 1 && !streams_overlap(S, good[0], cand[i])) continue;
        good.push_back(cand[i]);
    }
    if (good.size() == 2) { rest = good[0]; side = good[1]; }
    S->selFor = chain; S->selRest = rest; S->selSide = side;
}

// The update kernel with two operand stages, 64 KB of LDS: two workgroups per CU.  (Three and four stages with one workgroup per
// CU were measured and not adopted.)
constexpr int kSweepPerCu = 2;
void sweep_update_launch(hipStream_t stream, int G, const SweepArgs& g)
{
    hipLaunchKernelGGL(sweep_update_kernel<2>, dim3(G), dim3(256), (size_t)2 * 2 * 128 * 16 * sizeof(double), stream, g);
}
static const SweepCfg& sweep_cfg()
{
    static const SweepCfg c = [] {
        SweepCfg v = sweep_cfg_defaults();
        // the knobs force the sweep and both of its forms onto test-sized matrices
        if (const char* e = getenv("DCA_SWEEP_PRIO_CAP")) v.prioCap = std::max(8, atoi(e) / 8 * 8);
        if (const char* e = getenv("DCA_SWEEP_FACTOR_MAX_N")) v.factorMaxN = atoi(e);       // below: next pivot block from X (F F^T), P on the side stream
        if (const char* e = getenv("DCA_SWEEP_MIN")) v.minN = atoi(e);
        if (const char* e = getenv("DCA_SWEEP")) if (atoi(e) == 0) v.minN = INT_MAX;
        if (const char* e = getenv("DCA_SWEEP_PANEL")) v.wide = v.narrow = std::max(128, atoi(e) / 128 * 128);
        if (const char* e = getenv("DCA_SWEEP_CAP")) v.cap = std::max(8, atoi(e) / 8 * 8);
        return v;
    }();
    return c;
}

int sweep_kernels_prepare(int device)
{
    static std::mutex mu;
    static std::vector<int> done;
    std::lock_guard<std::mutex> lk(mu);
    for (int d : done) if (d == device) return DCA_OK;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(sweep_update_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 6 * 128 * 16 * 8));
    done.push_back(device);
    return DCA_OK;
}

int cholinv_sweep(dca_ctx* ctx, double* A, int n, double* work, int* dInfo, SideSet* side)
{
    const SweepCfg& cfg = sweep_cfg();
    DCA_TRY(sweep_kernels_prepare(ctx->device));
    struct Bounds { Bounds(int n) { tl_small32_max = chol_small32_max_in_sweep(n); } ~Bounds() { tl_small32_max = -1; } } bounds(n);
    static const bool traceOn = getenv("DCA_CHOLINV_TRACE") && atoi(getenv("DCA_CHOLINV_TRACE")) != 0;
    StepTrace tr;
    tr.on = traceOn;
    const int ld = n;
    const int B = sweep_panel_width(n, cfg);
    const std::vector<int> b = sweep_panels(n, B);
    const int np = (int)b.size() - 1;
    const int nt = (n + 127) / 128;
    EventPool* pool = event_pool_of(side);
    // Three streams.  chain (the context's): pivot blocks.  rest: the bulk of every step's update, one persistent launch after the
    // other.  side: everything else of a step -- W, the swept panel, the tiles the next steps' pivots need (prio), the next
    // panel's copy -- next to the rest launch of the step before or of its own.
    hipStream_t chain = ctx->stream, rest, sd;
    sweep_streams(side, chain, rest, sd);
    const int capAll = kSweepPerCu * 256;
    const int capRest = cfg.cap > 0 ? cfg.cap : capAll * 3 / 4 / 8 * 8;     // the rest launch leaves room for the side stream's and the chain's kernels
    const int capPrio = cfg.prioCap;
    const bool factorForm = sweep_factor_form(n, cfg);
    // events of step p: 0 P is there (chain), 1 prio tiles done (side), 2 the chain has read the pivot panel in M (chain), 3 W is there
    // (side), 4 rest done (rest)
    constexpr int EV = 5;
    auto ev = [&](int kind, int p) { return pool->get((size_t)EV * p + kind); };
    if (!ev(EV - 1, np)) { dca_set_error("cholinv: event creation failed"); return DCA_ERR_HIP; }
    // workspace: W[2] | Q[2] | P[2] | S[2] | Wn | arena of the recursion on a pivot block | tile counters
    const size_t BB = (size_t)B * B, NB_ = (size_t)n * B;
    double* W[2] = {work, work + NB_};
    double* Q[2] = {work + 2 * NB_, work + 3 * NB_};
    double* P[2] = {work + 4 * NB_, work + 4 * NB_ + BB};
    double* S[2] = {P[1] + BB, P[1] + 2 * BB};
    double* Wn = S[1] + BB;
    Arena chainWs{Wn + BB, 2 * BB};
    int* ctr = reinterpret_cast<int*>(Wn + 3 * BB);                 // [np][2][8]
    if (!sweep_workspace_fits(n, B, np)) { dca_set_error("cholinv sweep: workspace too small"); return DCA_ERR_NOMEM; }
    HIP_TRY(hipMemsetAsync(ctr, 0, (size_t)np * 16 * sizeof(int), chain));
    bool sideInFlight = false;
    int rc = DCA_OK;
    auto copy_block = [&](double* dst, int ldd, const double* src, int rows, int cols) {
        hipLaunchKernelGGL(copy_block_kernel, dim3(std::min(256, (rows * cols / 2 + 255) / 256)), dim3(256), 0, chain, dst, ldd, src, ld, rows, cols);
    };
#define SWEEP_HIP(expr) if ((expr) != hipSuccess) { dca_set_error("cholinv sweep: %s failed", #expr); rc = DCA_ERR_HIP; break; }
    copy_block(S[0], B, A, b[1], b[1]);
    if (hipEventRecord(ev(0, np), chain) != hipSuccess || hipStreamWaitEvent(sd, ev(0, np), 0) != hipSuccess) { dca_set_error("cholinv sweep: fork failed"); return DCA_ERR_HIP; }
    hipLaunchKernelGGL(gather_panel_kernel, dim3(b[1] / 32, n / 32), dim3(256), 0, sd, A, ld, 0, b[1], Q[0], B);
    sideInFlight = true;
    for (int p = 0; p < np && rc == DCA_OK; ++p) {
        const int c = b[p], w = b[p + 1] - c;
        const bool last = p + 1 == np;
        const int c1 = last ? n : b[p + 1], w1 = last ? 0 : b[p + 2] - c1;
        const int c2 = c1 + w1, w2 = (last || p + 2 == np) ? 0 : b[p + 3] - c2;
        double* Sp = S[p & 1];
        double* Pp = P[p & 1];
        double* Wp = W[p & 1];
        double* Qp = Q[p & 1];
        // ---- chain: X = inv(chol(S)), P = X^T X
        tr.mark(chain, "chain: pivot block begins", p);
        if ((rc = cholinv_rec(ctx, Sp, B, w, c, chainWs, dInfo, nullptr)) != DCA_OK) break;
        // chain-bound sizes (factorForm): P = X^T X is the side stream's, the chain goes on from X itself
        const GemmArgs pArgs{Sp, B, MASK_UPPER, Sp, B, MASK_UPPER, Pp, B, Pp, B, w, w, w, 1.0, 0.0, 1};
        if (!factorForm && (rc = launch_gemm(ctx, pArgs)) != DCA_OK) break;
        tr.mark(chain, "chain: P done", p);
        SWEEP_HIP(hipEventRecord(ev(0, p), chain));
        if (!last) {
            // the next pivot block from this one: S' = M[J', J'] - (M[J', J] P) M[J', J]^T, or with F = M[J', J] X^T (X lower: half
            // the flop, one product less on the chain) S' = M[J', J'] - F F^T
            if (p >= 1) SWEEP_HIP(hipStreamWaitEvent(chain, ev(1, p - 1), 0));
            const double* MnJ = A + (size_t)c1 * ld + c;
            if (factorForm) rc = launch_gemm(ctx, GemmArgs{MnJ, ld, MASK_NONE, Sp, B, MASK_LOWER, Wn, B, nullptr, 0, w1, w, w, 1.0, 0.0, 0, WALK_COLUMNS_REVERSED});
            else rc = launch_gemm(ctx, GemmArgs{MnJ, ld, MASK_NONE, Pp, B, MASK_NONE, Wn, B, nullptr, 0, w1, w, w, 1.0, 0.0, 0});
            if (rc != DCA_OK) break;
            // (the addend comes straight from M: the block is not copied first ...
            GemmArgs sArgs{Wn, B, MASK_NONE, factorForm ? Wn : MnJ, factorForm ? B : ld, MASK_NONE, S[(p + 1) & 1], B, nullptr, 0, w1, w1, w, -1.0, 1.0, 1};
            // ... at the chain-bound sizes (n = 4032: 3.40 -> 3.31 with F, -> 3.20 ms without the copy kernel; at n = 10 048 the
            // copy-free form measured 0.3 ms SLOWER on the same box: 20.1 / 20.5 ms)
            if (!factorForm) copy_block(S[(p + 1) & 1], B, A + (size_t)c1 * ld + c1, w1, w1);
            else { sArgs.Cin = A + (size_t)c1 * ld + c1; sArgs.ldcin = ld; }
            if ((rc = launch_gemm(ctx, sArgs)) != DCA_OK) break;
            SWEEP_HIP(hipEventRecord(ev(2, p), chain));
            tr.mark(chain, "chain: next pivot block formed", p);
        }
        // ---- side: W = Q P (Q: this panel's copy, made at the end of the side stream's previous step), then the swept panel
        SWEEP_HIP(hipStreamWaitEvent(sd, ev(0, p), 0));
        tr.mark(sd, "side: step begins", p);
        if (factorForm && (rc = launch_gemm_on(sd, pArgs)) != DCA_OK) break;
        if ((rc = launch_gemm_on(sd, GemmArgs{Qp, B, MASK_NONE, Pp, B, MASK_NONE, Wp, B, nullptr, 0, n, w, w, 1.0, 0.0, 0})) != DCA_OK) break;
        SWEEP_HIP(hipEventRecord(ev(3, p), sd));
        tr.mark(sd, "side: W done", p);
        if (!last) SWEEP_HIP(hipStreamWaitEvent(sd, ev(2, p), 0));
        hipLaunchKernelGGL(sweep_finalize_kernel, dim3(w / 32, n / 32), dim3(256), 0, sd, A, ld, c, w, Wp, B, Pp, B);
        SweepArgs g{Wp, B, Qp, B, A, ld, n, c, w, nt, c / 128, (c1 + w1 + 127) / 128 - c / 128, SWEEP_REST, c1 / 128, (c1 + w1 + 127) / 128 - c1 / 128,
                    c2 / 128, w2 > 0 ? (c2 + w2 + 127) / 128 - c2 / 128 : 0, 0, nullptr};
        if (w1 == 0) { g.prN = 0; g.skipN = nt - g.skip0; }
        const int nR = nt - g.skipN;
        if (!last) {
            // ---- side: the next panel's tiles and the diagonal block after it (they were tiles of the rest launch one step ago), then the
            // next panel's copy
            if (p >= 1) SWEEP_HIP(hipStreamWaitEvent(sd, ev(4, p - 1), 0));
            tr.mark(sd, "side: prio begins", p);
            SweepArgs gp = g;
            gp.mode = SWEEP_PRIO;
            gp.nTiles = g.prN * nR + g.dgN * (g.dgN + 1) / 2;
            gp.ctr = ctr + (size_t)p * 16 + 8;
            if (gp.nTiles > 0) sweep_update_launch(sd, std::min(capPrio, (gp.nTiles + 7) / 8 * 8), gp);
            SWEEP_HIP(hipEventRecord(ev(1, p), sd));
            tr.mark(sd, "side: prio done", p);
            hipLaunchKernelGGL(gather_panel_kernel, dim3(w1 / 32, n / 32), dim3(256), 0, sd, A, ld, c1, w1, Q[(p + 1) & 1], B);
        }
        // ---- rest
        if (nR > 0) {
            SWEEP_HIP(hipStreamWaitEvent(rest, ev(3, p), 0));
            g.mode = SWEEP_REST;
            const int bands = (nR + 3) / 4;
            g.nTiles = 8 * bands * bands + 2 * bands;
            g.ctr = ctr + (size_t)p * 16;
            tr.mark(rest, "rest: begins", p);
            sweep_update_launch(rest, std::min(last ? capAll : capRest, (g.nTiles + 7) / 8 * 8), g);
            tr.mark(rest, "rest: done", p);
        }
        SWEEP_HIP(hipEventRecord(ev(4, p), rest));
        if (hipGetLastError() != hipSuccess) { dca_set_error("cholinv sweep: launch failed"); rc = DCA_ERR_HIP; }
    }
#undef SWEEP_HIP
    if (rc != DCA_OK) {
        if (sideInFlight) { hipStreamSynchronize(rest); hipStreamSynchronize(sd); }   // they write A and read the workspace: drain them before the caller may free either
        tr.dump();
        return rc;
    }
    // the lower triangle is the result: mirror it, once the last panel is written (side) and the last tiles are (rest)
    const int nb32 = n / 32;
    if (hipEventRecord(ev(1, np), sd) != hipSuccess || hipStreamWaitEvent(rest, ev(1, np), 0) != hipSuccess) {
        hipStreamSynchronize(rest); hipStreamSynchronize(sd);
        dca_set_error("cholinv sweep: join of the side stream failed");
        return DCA_ERR_HIP;
    }
    hipLaunchKernelGGL(symmetrize_kernel, dim3(nb32 * (nb32 - 1) / 2), dim3(256), 0, rest, A, ld, nb32);
    hipLaunchKernelGGL(symmetrize_diag_kernel, dim3(nb32), dim3(256), 0, rest, A, ld);
    if (hipEventRecord(ev(2, np), rest) != hipSuccess || hipStreamWaitEvent(chain, ev(2, np), 0) != hipSuccess) {
        hipStreamSynchronize(rest);
        dca_set_error("cholinv sweep: join of the rest stream failed");
        return DCA_ERR_HIP;
    }
    tr.mark(chain, "sweep done", np);
    tr.dump();
    return DCA_OK;
}

}  // namespace

int dca_spd_inverse_device(dca_ctx* ctx, double* dA, int n, double* dWork, int* info_out, double scale, double** result)
{
    if (n % 64 != 0 || n <= 0) { dca_set_error("dca_spd_inverse_device: n must be a positive multiple of 64"); return DCA_ERR_ARG; }
    DCA_TRY(gemm_kernels_prepare(ctx->device));
    ScopedKernelClock kc(ctx, "mf_inverse");
    DevBuf<int> dInfo;
    HIP_TRY(dInfo.alloc(1));
    HIP_TRY(hipMemsetAsync(dInfo, 0, sizeof(int), ctx->stream));
    Arena ws{dWork, (size_t)n * n};
    int rc;
    bool swept = false;
    {
        ScopedKernelClock kr(ctx, "mf_inverse_recursion");
        // n >= 2560: the block sweep; below it, or where no side set is to be had, the fused recursion.
        // A set of side streams only where one will be used (the sweep; the recursion's top level from n = 2048); everything they
        // run is joined into ctx->stream before either returns, so the set can go back as soon as the launches are enqueued
        const bool wantSweep = sweep_wanted(n, sweep_cfg());
        SideSet* side = chol_wants_side_set(n, wantSweep) ? side_set_acquire(ctx->device) : nullptr;
        if (wantSweep && side) {
            // -inv(A) in place
            rc = cholinv_sweep(ctx, dA, n, dWork, dInfo, side);
            swept = true;
        } else rc = cholinv_rec(ctx, dA, n, n, 0, ws, dInfo, side);
        side_set_release(side);
    }
    if (rc == DCA_OK && swept) {
        if (scale != -1.0) {
            hipLaunchKernelGGL(scale_matrix_kernel, dim3(2048), dim3(256), 0, ctx->stream, dA, (size_t)n * n, -scale);
            HIP_TRY(hipGetLastError());
        }
        *result = dA;
    } else if (rc == DCA_OK) {
        double* out = dWork + (size_t)n * n;
        // scale * inv(A)[i][j] = scale * sum_{k >= max(i,j)} X[k][i] X[k][j] = scale * sum_k Xt[i][k] Xt[j][k]
        ScopedKernelClock kx(ctx, "mf_inverse_xtx");
        rc = launch_gemm(ctx, GemmArgs{dA, n, MASK_UPPER, dA, n, MASK_UPPER, out, n, out, n, n, n, n, scale, 0.0, 1});
        *result = out;
    }
    int info = 0;
    HIP_TRY_AS(hipMemcpyAsync(&info, dInfo, sizeof(int), hipMemcpyDeviceToHost, ctx->stream), "cholinv");
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), "cholinv");
    if (info_out) *info_out = info;
    return rc;
}
