// Reduction kernels of the plmDCA optimiser (plm_engine.hip): the dot products of the line search and of the L-BFGS
// two-loop recursion, the recursion itself on the device, and the sums that finish fx.  The elementwise vector kernels and the
// double-double helpers are vec_kernels.h's.
#pragma once

#include "dca_internal.h"
#include "plm_plan.h"
#include "vec_kernels.h"

namespace {

// Dot-product accumulators of the optimiser.  float32 vectors: products and sums in double (already far more exact than the
// reference's float sums).  float64 vectors (the parity mode): the ROUNDED products are summed in double-double, like the
// objective -- a plain double sum of P = 5.5e7 products carries ~1e-13 of order-dependent rounding, g.d / y.s / y.y and the
// Gram entries steer the line search and scale the direction, and the optimisation amplifies such noise from iteration to
// iteration.  The float64 oracle compensates the same sums (Neumaier), so both see the sum of the
// same rounded products to the last bit or two, whatever the order.  Partials travel as (hi, lo) pairs in both cases.
template <bool DD> struct DotAcc;
template <> struct DotAcc<false> {
    double hi = 0.0;
    static constexpr double lo = 0.0;
    __device__ __forceinline__ void add(double a, double b) { hi += a * b; }
    __device__ __forceinline__ void wave_reduce() { for (int off = 32; off > 0; off >>= 1) hi += __shfl_down(hi, off); }
};
template <> struct DotAcc<true> {
    double hi = 0.0, lo = 0.0;
    __device__ __forceinline__ void add(double a, double b) { dd_add(hi, lo, __dmul_rn(a, b)); }
    __device__ __forceinline__ void wave_reduce() { dd_wave_reduce(hi, lo); }
};
// the workgroup's waves leave their (hi, lo) in red[wave][2 * v], [2 * v + 1]; thread v < nv adds them in wave order
template <int NV>
__device__ __forceinline__ void dot_block_store(double (*red)[2 * NV], int nv, double* __restrict__ partials, unsigned grid = 0)
{
    __syncthreads();
    if ((int)threadIdx.x < nv) {
        double hi = 0.0, lo = 0.0;
        for (int w = 0; w < (int)blockDim.x / 64; ++w) dd_add2(hi, lo, red[w][2 * threadIdx.x], red[w][2 * threadIdx.x + 1]);
        const size_t slot = (size_t)threadIdx.x * (grid ? grid : gridDim.x) + blockIdx.x;
        partials[2 * slot] = hi;
        partials[2 * slot + 1] = lo;
    }
}

// (hi, lo) partials [2 * (k*gridDim.x + block)] for k = 0..2 : a.b, c.c, a.a   (g.d, x.x, g.g)
template <typename T>
__global__ __launch_bounds__(kVecThreads)
void vec_dot3_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c, size_t n,
                     double* __restrict__ partials)
{
    __shared__ double red[kVecThreads / 64][6];
    DotAcc<sizeof(T) == 8> s0, s1, s2;
    DCA_VEC_LOOP(n, a,
        const Pack<T> pa = ldp(a, iv); const Pack<T> pb = ldp(b, iv); const Pack<T> pc = ldp(c, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) {
            const double av = pa.v[k]; const double bv = pb.v[k]; const double cv = pc.v[k];
            s0.add(av, bv); s1.add(cv, cv); s2.add(av, av);
        },
        { const double av = a[i]; const double bv = b[i]; const double cv = c[i]; s0.add(av, bv); s1.add(cv, cv); s2.add(av, av); })
    s0.wave_reduce(); s1.wave_reduce(); s2.wave_reduce();
    if ((threadIdx.x & 63) == 0) {
        double* r = red[threadIdx.x >> 6];
        r[0] = s0.hi; r[1] = s0.lo; r[2] = s1.hi; r[3] = s1.lo; r[4] = s2.hi; r[5] = s2.lo;
    }
    dot_block_store<3>(red, 3, partials);
}
// L-BFGS direction in one pass instead of 2m dependent dot/axpy rounds: every vector of the
// two-loop recursion (lbfgs.cpp:568-601) lies in span{g, s_k, y_k}, so the recursion can be run
// on 2m+1 coefficients once the Gram entries it needs are known: for the newest pair e and every
// slot k: s_k.g, y_k.g, s_e.y_k, y_e.s_k, y_e.y_k (25 dot products; the entries between older pairs are
// kept from earlier iterations).  vec_diff_gram_kernel below produces them in the pass that forms the pair.
struct VecPtrs5 { const void* s[5]; const void* y[5]; };
struct DirCoefs { double g; double s[5]; double y[5]; };

// Optimiser scalars that live on the device: dot products of the stored pairs and the coefficients of the current
// search direction in {g, s_k, y_k}.  The two-loop recursion runs here (one thread), so an iteration needs ONE host
// round trip -- the line search's decision after an evaluation -- instead of two.
struct LbfgsDev { double SY[5][5]; double YY[5][5]; double ys[5]; DirCoefs cf; };
constexpr int kSlotDginit = 30;      // dScal slot of g.d for the next line search

// lbfgs.cpp:568-601 on the coefficients; scal[1..2] = y.s, y.y of the newest pair e, scal[3..27] the 25 Gram entries
// [kind * 5 + k]: s_k.g, y_k.g, s_e.y_k, s_k.y_e, y_e.y_k; gg = g.g of the accepted point (the host has it).
__global__ void lbfgs_two_loop_kernel(double* __restrict__ scal, LbfgsDev* __restrict__ st, int e, int endNext, int bound, double gg)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    constexpr int M = 5;
    const double ys = scal[1], yy = scal[2];
    const double* G5 = scal + 3;
    double Sg[M], Yg[M], alpha[M];
    st->ys[e] = ys;
    for (int k2 = 0; k2 < M; ++k2) {
        Sg[k2] = G5[k2]; Yg[k2] = G5[5 + k2];
        st->SY[e][k2] = G5[10 + k2];            // s_e . y_k
        st->SY[k2][e] = G5[15 + k2];            // s_k . y_e
        st->YY[e][k2] = G5[20 + k2];
        st->YY[k2][e] = G5[20 + k2];
        alpha[k2] = 0.0;
    }
    st->SY[e][e] = ys; st->YY[e][e] = yy;
    DirCoefs cf;
    cf.g = -1.0;
    for (int k2 = 0; k2 < M; ++k2) cf.s[k2] = cf.y[k2] = 0.0;
    int j = endNext;
    for (int i = 0; i < bound; ++i) {
        j = (j + M - 1) % M;
        double sd = cf.g * Sg[j];
        for (int k2 = 0; k2 < M; ++k2) sd += cf.y[k2] * st->SY[j][k2];   // d has no s components yet
        alpha[j] = sd / st->ys[j];
        cf.y[j] -= alpha[j];
    }
    const double scale = ys / yy;
    cf.g *= scale;
    for (int k2 = 0; k2 < M; ++k2) cf.y[k2] *= scale;
    for (int i = 0; i < bound; ++i) {
        double yd = cf.g * Yg[j];
        for (int k2 = 0; k2 < M; ++k2) yd += cf.s[k2] * st->SY[k2][j] + cf.y[k2] * st->YY[j][k2];
        const double beta = yd / st->ys[j];
        cf.s[j] += alpha[j] - beta;
        j = (j + 1) % M;
    }
    st->cf = cf;
    // g.d for the next line search, from the same coefficients
    double gd = cf.g * gg;
    for (int k2 = 0; k2 < M; ++k2) gd += cf.s[k2] * Sg[k2] + cf.y[k2] * Yg[k2];
    scal[kSlotDginit] = gd;
}

// s_e = x - xp, y_e = g - gp (lbfgs.cpp:546-558) are formed, stored and used in one pass, so the newest pair is not
// read back and g is read once (14 vector passes; 19 as two kernels, 0.75 -> 0.6 ms at D).  partials[v * gridDim.x +
// block]: v = 0, 1 are y_e.s_e and y_e.y_e, v = 2 + kind * 5 + k the Gram entries (kinds in the order above).
template <typename T, int E>
__global__ __launch_bounds__(kVecThreads)
void vec_diff_gram_kernel(VecPtrs5 P, T* __restrict__ se, T* __restrict__ ye, const T* __restrict__ x, const T* __restrict__ xp,
                          const T* __restrict__ g, const T* __restrict__ gp, size_t n, double* __restrict__ partials)
{
    // E = slot of the newest pair, a template parameter: as a run-time value the test `k != e` stood in front of every pair's two
    // loads, which the compiler then issued and WAITED for pair by pair -- six round trips per pack with two to four loads in
    // flight (config D: 3.7 TB/s where the other vector kernels reach 5.3 - 6.4).  All twelve loads of a pack are issued before
    // the first store (the stores may alias the history for all the compiler knows).
    __shared__ double red[kVecThreads / 64][54];
    DotAcc<sizeof(T) == 8> acc[27];
    DCA_VEC_LOOP(n, se,
        const Pack<T> px = ldp(x, iv); const Pack<T> pxp = ldp(xp, iv); const Pack<T> pg = ldp(g, iv); const Pack<T> pgp = ldp(gp, iv);
        Pack<T> psk[5]; Pack<T> pyk[5];
        _Pragma("unroll") for (int k = 0; k < 5; ++k)
            if (k != E) { psk[k] = ldp(static_cast<const T*>(P.s[k]), iv); pyk[k] = ldp(static_cast<const T*>(P.y[k]), iv); }
        Pack<T> pse; Pack<T> pye;
        _Pragma("unroll") for (int u = 0; u < VEC; ++u) {
            pse.v[u] = px.v[u] - pxp.v[u]; pye.v[u] = pg.v[u] - pgp.v[u];
            acc[0].add((double)pye.v[u], (double)pse.v[u]); acc[1].add((double)pye.v[u], (double)pye.v[u]);
        }
        psk[E] = pse; pyk[E] = pye;
        stp(se, iv, pse); stp(ye, iv, pye);
        _Pragma("unroll") for (int k = 0; k < 5; ++k) {
            _Pragma("unroll") for (int u = 0; u < VEC; ++u) {
                const double gv = pg.v[u]; const double sev = pse.v[u]; const double yev = pye.v[u];
                const double sk = psk[k].v[u]; const double yk = pyk[k].v[u];
                acc[2 + k].add(sk, gv); acc[7 + k].add(yk, gv); acc[12 + k].add(sev, yk); acc[17 + k].add(yev, sk); acc[22 + k].add(yev, yk);
            }
        },
        { const T sev_ = x[i] - xp[i]; const T yev_ = g[i] - gp[i]; se[i] = sev_; ye[i] = yev_;
          const double gv = g[i]; const double sev = sev_; const double yev = yev_;
          acc[0].add(yev, sev); acc[1].add(yev, yev);
          _Pragma("unroll") for (int k = 0; k < 5; ++k) {
              const double sk = k == E ? sev : (double)static_cast<const T*>(P.s[k])[i]; const double yk = k == E ? yev : (double)static_cast<const T*>(P.y[k])[i];
              acc[2 + k].add(sk, gv); acc[7 + k].add(yk, gv); acc[12 + k].add(sev, yk); acc[17 + k].add(yev, sk); acc[22 + k].add(yev, yk);
          } })
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < 27; ++v) {
        acc[v].wave_reduce();
        if (lane == 0) { red[wv][2 * v] = acc[v].hi; red[wv][2 * v + 1] = acc[v].lo; }
    }
    dot_block_store<27>(red, 27, partials);
}

// d = c.g * g + sum_k c.s[k] * s_k + c.y[k] * y_k
template <typename T>
__global__ void vec_compose_kernel(T* __restrict__ d, const T* __restrict__ g, VecPtrs5 P, const DirCoefs* __restrict__ cp, size_t n)
{
    const DirCoefs c = *cp;
    DCA_VEC_LOOP(n, d,
        const Pack<T> pg = ldp(g, iv);
        double v[VEC];
        _Pragma("unroll") for (int u = 0; u < VEC; ++u) v[u] = c.g * (double)pg.v[u];
        _Pragma("unroll") for (int k = 0; k < 5; ++k) {
            const Pack<T> psk = ldp(static_cast<const T*>(P.s[k]), iv); const Pack<T> pyk = ldp(static_cast<const T*>(P.y[k]), iv);
            _Pragma("unroll") for (int u = 0; u < VEC; ++u) v[u] += c.s[k] * (double)psk.v[u] + c.y[k] * (double)pyk.v[u];
        }
        Pack<T> o;
        _Pragma("unroll") for (int u = 0; u < VEC; ++u) o.v[u] = (T)v[u];
        stp(d, iv, o);,
        { double v = c.g * (double)g[i];
          _Pragma("unroll") for (int k = 0; k < 5; ++k)
              v += c.s[k] * (double)static_cast<const T*>(P.s[k])[i] + c.y[k] * (double)static_cast<const T*>(P.y[k])[i];
          d[i] = (T)v; })
}
#undef ldp
#undef stp

// ---- direction, first trial point and coupling table in ONE pass (one GPU, plain path; PlmEngine::fused_step_ok)
// After the first iteration the line search's first trial step is 1, known when the direction is composed.  So, per element:
// d = vec_compose_kernel's expression, xt = vec_step_kernel's with step (T)1 on the accepted x and the rounded d, and W takes xt
// where plm_expand_kernel would put it -- 12 reads and 2 writes of the packed vector and one write of W, where the three kernels
// read 16, wrote 2 and wrote W in runs of q elements.  No sum is formed here: every element is a chain of its own, so the bits are
// those of the three kernels whatever the tiling.
// The pairs (i, j) are packed i-major.  A workgroup owns TI consecutive sites i (the columns of one 512-byte strip of W) x JC
// consecutive sites j: per i one contiguous piece of JC q^2 packed elements, read and written in 16-byte packs (the packs at a
// piece's two ends are shared with the neighbouring workgroup: both compute them, each stores its own elements).  xt goes through
// LDS as tile[ii][jj][a][b]; rows (i, a) of W then take runs of JC q elements, the transposed rows (j, b) runs of TI q.  The
// workgroups behind the pair blocks (their count rounded up to 64) do the fields, one element per thread.
__host__ __device__ constexpr int fused_step_ti(int q, int elemBytes) { return kRowBytes / elemBytes / q; }
// JC at q = 21: 42 KB of LDS, three workgroups of eight waves per CU.  Measured at config D (float32): JC 2 / 3 / 4 / 6 with 256 or
// 512 threads all lie within 2.5 % of each other, this one first
__host__ __device__ constexpr int fused_step_jc(int q) { return q == 21 ? 4 : 16; }
constexpr int kFusedStepThreads = 512;

template <typename T>
__device__ __forceinline__ T compose_elem(const DirCoefs& c, T gv, const T* sv, const T* yv)
{
    double v = c.g * (double)gv;
#pragma unroll
    for (int k = 0; k < 5; ++k) v += c.s[k] * (double)sv[k] + c.y[k] * (double)yv[k];
    return (T)v;
}

template <typename T, int Q>
__global__ __launch_bounds__(kFusedStepThreads)
void lbfgs_dir_trial_expand_kernel(T* __restrict__ d, T* __restrict__ xt, T* __restrict__ W, const T* __restrict__ x, const T* __restrict__ g,
                                   VecPtrs5 P, const DirCoefs* __restrict__ cp, int L, int Cs, int numJC, int pairBlocks)
{
    constexpr int VEC = 16 / (int)sizeof(T), TI = fused_step_ti(Q, (int)sizeof(T)), JC = fused_step_jc(Q), Q2 = Q * Q;
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];
    T* tile = reinterpret_cast<T*>(dca_smem);
    __shared__ size_t sLo[TI];          // first packed element of site ii's piece
    __shared__ int sCnt[TI];            // its elements
    __shared__ int sPre[TI + 1];        // packs of the pieces in front of it
    const DirCoefs c = *cp;
    const T one = (T)1.0;
    const int tid = threadIdx.x;
    const int padded = (pairBlocks + 63) / 64 * 64;
    if ((int)blockIdx.x >= padded) {
        const size_t e = (size_t)((int)blockIdx.x - padded) * kFusedStepThreads + tid;
        if (e < (size_t)L * Q) {
            T sv[5], yv[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { sv[k] = static_cast<const T*>(P.s[k])[e]; yv[k] = static_cast<const T*>(P.y[k])[e]; }
            const T dv = compose_elem(c, g[e], sv, yv);
            d[e] = dv;
            const T v = one * dv;
            xt[e] = x[e] + v;
        }
        return;
    }
    // Workgroups are dealt to the 8 XCDs in turn.  Of every 64 consecutive pair blocks, each XCD takes 8 consecutive ones: pieces
    // that are neighbours in memory share the cache lines at their ends (reads of the packed vectors, runs of W), and seven
    // of eight such ends then meet in one L2.  For speed only: nothing depends on where a workgroup runs.
    const int blk = ((int)blockIdx.x & ~63) | (((int)blockIdx.x & 7) << 3) | (((int)blockIdx.x >> 3) & 7);
    if (blk >= pairBlocks) return;
    const int i0 = (blk / numJC) * TI, j0 = (blk % numJC) * JC;
    const int j1 = min(j0 + JC, L);
    if (j1 <= i0 + 1) return;           // below the diagonal; uniform over the workgroup
    if (tid == 0) {
        int pre = 0;
        for (int ii = 0; ii < TI; ++ii) {
            const int i = i0 + ii, jlo = max(j0, i + 1);
            const int cnt = jlo < j1 ? (j1 - jlo) * Q2 : 0;
            const size_t before = (size_t)L * (L - 1) / 2 - (size_t)(L - i) * (L - i - 1) / 2;       // pairs whose first site is < i
            const size_t lo = cnt ? (size_t)L * Q + (before + (size_t)(jlo - i - 1)) * Q2 : 0;
            sLo[ii] = lo; sCnt[ii] = cnt; sPre[ii] = pre;
            pre += cnt ? (int)((lo + cnt + VEC - 1) / VEC - lo / VEC) : 0;
        }
        sPre[TI] = pre;
    }
    __syncthreads();
    const int total = sPre[TI];
    for (int idx = tid; idx < total; idx += kFusedStepThreads) {
        int ii = 0;
        while (idx >= sPre[ii + 1]) ++ii;
        const size_t lo = sLo[ii], hi = lo + (size_t)sCnt[ii];
        const size_t iv = lo / VEC + (size_t)(idx - sPre[ii]);
        // all twelve loads of the pack are issued before the first store
        const Pack<T> pg = ldp_at(g, iv); const Pack<T> px = ldp_at(x, iv);
        Pack<T> psk[5]; Pack<T> pyk[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { psk[k] = ldp_at(static_cast<const T*>(P.s[k]), iv); pyk[k] = ldp_at(static_cast<const T*>(P.y[k]), iv); }
        Pack<T> od, ox;
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            T sv[5], yv[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) { sv[k] = psk[k].v[u]; yv[k] = pyk[k].v[u]; }
            od.v[u] = compose_elem(c, pg.v[u], sv, yv);
            const T v = one * od.v[u];
            ox.v[u] = px.v[u] + v;
        }
        const size_t e0 = iv * VEC;
        // tile[ii][jj][a][b]: the piece starts at site max(j0, i + 1)
        T* const dst = tile + (size_t)(ii * JC + (max(j0, i0 + ii + 1) - j0)) * Q2;
        if (e0 >= lo && e0 + VEC <= hi) {
            stp_at(d, iv, od); stp_at(xt, iv, ox);
#pragma unroll
            for (int u = 0; u < VEC; ++u) dst[e0 + u - lo] = ox.v[u];
        } else {
#pragma unroll
            for (int u = 0; u < VEC; ++u) {
                const size_t e = e0 + u;
                if (e >= lo && e < hi) { d[e] = od.v[u]; xt[e] = ox.v[u]; dst[e - lo] = ox.v[u]; }
            }
        }
    }
    __syncthreads();
    // Both triangles are walked row by row of W, a thread stepping kFusedStepThreads elements at a time with its (row, column)
    // kept up by additions.  tile[(ii JC + jj) q^2 + a q + b] with row = ii q + a, col = jj q + b is
    // tile[row q + ii (JC - 1) q^2 + col + jj (q - 1) q].
    // rows (i, a), columns (j, b): runs over the workgroup's sites j
    {
        constexpr int WD = JC * Q;
        int row = tid / WD, col = tid % WD;
        while (row < TI * Q) {
            const int ii = row / Q, jj = col / Q;
            const int i = i0 + ii, j = j0 + jj;
            if (j > i && j < j1) W[(size_t)(i0 * Q + row) * Cs + j0 * Q + col] = tile[row * Q + ii * ((JC - 1) * Q2) + col + jj * ((Q - 1) * Q)];
            row += kFusedStepThreads / WD; col += kFusedStepThreads % WD;
            if (col >= WD) { col -= WD; ++row; }
        }
    }
    // rows (j, b), columns (i, a): runs over the tile's sites i
    {
        constexpr int WD = TI * Q;
        int row = tid / WD, col = tid % WD;
        while (row < JC * Q) {
            const int jj = row / Q, ii = col / Q;
            const int i = i0 + ii, j = j0 + jj;
            if (j > i && j < j1) W[(size_t)(j0 * Q + row) * Cs + i0 * Q + col] = tile[col * Q + ii * ((JC - 1) * Q2) + row + jj * ((Q - 1) * Q)];
            row += kFusedStepThreads / WD; col += kFusedStepThreads % WD;
            if (col >= WD) { col -= WD; ++row; }
        }
    }
}

// out[k] = sum_b of the (hi, lo) pairs partials[2 * (k*nb + b)], k < nk, rounded once; one block per k, fixed tree
__global__ __launch_bounds__(256)
void vec_final_kernel(const double* __restrict__ partials, int nb, int nk, double* __restrict__ out)
{
    __shared__ double redHi[256], redLo[256];
    const int k = blockIdx.x;
    double hi = 0.0, lo = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) dd_add2(hi, lo, partials[2 * ((size_t)k * nb + b)], partials[2 * ((size_t)k * nb + b) + 1]);
    dd_block_reduce(hi, lo, redHi, redLo);
    if (threadIdx.x == 0) out[k] = hi + lo;
}

// ---- sums of (hi, lo) pairs (the objective's partial sums), in two stages: kSumStageBlocks (plm_plan.h) first-stage blocks
// block b sums its contiguous chunk of the n pairs into pair b of out
__global__ __launch_bounds__(256)
void dd_sum_chunks_kernel(const double* __restrict__ parts, int n, double* __restrict__ out)
{
    __shared__ double redHi[256], redLo[256];
    const int chunk = (n + gridDim.x - 1) / gridDim.x;
    const int lo_ = blockIdx.x * chunk, hi_ = min(n, lo_ + chunk);
    double hi = 0.0, lo = 0.0;
    for (int b = lo_ + threadIdx.x; b < hi_; b += blockDim.x) dd_add2(hi, lo, parts[2 * (size_t)b], parts[2 * (size_t)b + 1]);
    dd_block_reduce(hi, lo, redHi, redLo);
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = hi; out[2 * blockIdx.x + 1] = lo; }
}
// out[0] = the sum of the nA pairs of A and the nB pairs of B, rounded once
__global__ __launch_bounds__(1024)
void dd_sum_final_kernel(const double* __restrict__ A, int nA, const double* __restrict__ B, int nB, double* __restrict__ out)
{
    __shared__ double redHi[1024], redLo[1024];
    double hi = 0.0, lo = 0.0;
    for (int b = threadIdx.x; b < nA; b += blockDim.x) dd_add2(hi, lo, A[2 * (size_t)b], A[2 * (size_t)b + 1]);
    for (int b = threadIdx.x; b < nB; b += blockDim.x) dd_add2(hi, lo, B[2 * (size_t)b], B[2 * (size_t)b + 1]);
    dd_block_reduce(hi, lo, redHi, redLo);
    if (threadIdx.x == 0) out[0] = hi + lo;
}

// The two reductions that end an evaluation of the optimiser -- fx from its per-pair / per-chunk partial sums (dd_sum_chunks_kernel,
// dd_sum_final_kernel) and the three dot products of the line search (vec_dot3_kernel, vec_final_kernel) -- as TWO launches instead
// of four: the workgroups behind the first kVecBlocks of the first launch sum the fx chunks, the workgroup behind the dot products'
// of the second finishes fx.  Every sum is formed by the same code over the same operands in the same order as in the separate
// kernels (the vector walk with its grid given, the 256-thread tree inside the 1024-thread workgroups), so the bits are theirs; what
// goes is two launch boundaries and ~11 us of two tiny kernels per evaluation (config C: 1.6 % of the step).
template <typename T>
__global__ __launch_bounds__(kVecThreads)
void vec_dot3_fx_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c, size_t n, double* __restrict__ partials,
                        const double* __restrict__ fxParts, int nFxParts, double* __restrict__ fxChunks)
{
    if (blockIdx.x >= (unsigned)kVecBlocks) {
        __shared__ double redHi[256], redLo[256];
        const int blk = (int)blockIdx.x - kVecBlocks;
        const int chunk = (nFxParts + kSumStageBlocks - 1) / kSumStageBlocks;
        const int lo_ = blk * chunk, hi_ = min(nFxParts, lo_ + chunk);
        double hi = 0.0, lo = 0.0;
        for (int p = lo_ + threadIdx.x; p < hi_; p += blockDim.x) dd_add2(hi, lo, fxParts[2 * (size_t)p], fxParts[2 * (size_t)p + 1]);
        dd_block_reduce(hi, lo, redHi, redLo);
        if (threadIdx.x == 0) { fxChunks[2 * blk] = hi; fxChunks[2 * blk + 1] = lo; }
        return;
    }
    __shared__ double red[kVecThreads / 64][6];
    DotAcc<sizeof(T) == 8> s0, s1, s2;
    DCA_VEC_LOOP_G(n, a, kVecBlocks,
        const Pack<T> pa = ldp_at(a + head_, iv); const Pack<T> pb = ldp_at(b + head_, iv); const Pack<T> pc = ldp_at(c + head_, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) {
            const double av = pa.v[k]; const double bv = pb.v[k]; const double cv = pc.v[k];
            s0.add(av, bv); s1.add(cv, cv); s2.add(av, av);
        },
        { const double av = a[i]; const double bv = b[i]; const double cv = c[i]; s0.add(av, bv); s1.add(cv, cv); s2.add(av, av); })
    s0.wave_reduce(); s1.wave_reduce(); s2.wave_reduce();
    if ((threadIdx.x & 63) == 0) {
        double* r = red[threadIdx.x >> 6];
        r[0] = s0.hi; r[1] = s0.lo; r[2] = s1.hi; r[3] = s1.lo; r[4] = s2.hi; r[5] = s2.lo;
    }
    dot_block_store<3>(red, 3, partials, kVecBlocks);
}
// 1024 threads per workgroup.  Workgroups 0 .. nk - 1: vec_final_kernel's sum of dot product k with its 256 threads (the others only
// keep the barriers company); workgroup nk: dd_sum_final_kernel's sum of fx with all 1024.
__global__ __launch_bounds__(1024)
void vec_final_fx_kernel(const double* __restrict__ partials, int nb, int nk, double* __restrict__ out,
                         const double* __restrict__ A, int nA, const double* __restrict__ B, int nB, double* __restrict__ fxOut)
{
    __shared__ double redHi[1024], redLo[1024];
    const int k = blockIdx.x;
    double hi = 0.0, lo = 0.0;
    if (k < nk) {
        constexpr int NT = 256;
        if ((int)threadIdx.x < NT) {
            for (int b = threadIdx.x; b < nb; b += NT) dd_add2(hi, lo, partials[2 * ((size_t)k * nb + b)], partials[2 * ((size_t)k * nb + b) + 1]);
            redHi[threadIdx.x] = hi;
            redLo[threadIdx.x] = lo;
        }
        __syncthreads();
        for (int st = NT / 2; st > 0; st >>= 1) {
            if ((int)threadIdx.x < st) dd_add2(redHi[threadIdx.x], redLo[threadIdx.x], redHi[threadIdx.x + st], redLo[threadIdx.x + st]);
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = redHi[0] + redLo[0];
        return;
    }
    for (int b = threadIdx.x; b < nA; b += blockDim.x) dd_add2(hi, lo, A[2 * (size_t)b], A[2 * (size_t)b + 1]);
    for (int b = threadIdx.x; b < nB; b += blockDim.x) dd_add2(hi, lo, B[2 * (size_t)b], B[2 * (size_t)b + 1]);
    dd_block_reduce(hi, lo, redHi, redLo);
    if (threadIdx.x == 0) fxOut[0] = hi + lo;
}

}  // namespace
