// Elementwise vector kernels of the L-BFGS optimisers (plm_engine.hip, ardca.hip).  Each is one rounded multiply or add per
// element (the build has -ffp-contract=off), so the results do not depend on the launch geometry.
#pragma once

#include "dca_internal.h"

namespace {

constexpr int kVecBlocks = 1024;
constexpr int kVecThreads = 256;

template <typename T> struct V16;
template <> struct V16<float> { using type = float4; };
template <> struct V16<double> { using type = double2; };

// All vector kernels stream 16 bytes per lane and load (4 floats / 2 doubles): with 4-byte loads a
// wave has too few bytes in flight to approach HBM bandwidth.  Element k of a pack is element
// iv*VEC + k; the n % VEC tail is handled by the first threads with scalar accesses.  The mapping
// of elements to threads is fixed, so every reduction is deterministic.
template <typename T> struct Pack { T v[16 / sizeof(T)]; };
template <typename T> __device__ __forceinline__ Pack<T> ldp_at(const T* p, size_t iv)
{
    using V = typename V16<T>::type;
    const V r = reinterpret_cast<const V*>(p)[iv];
    Pack<T> o;
    if constexpr (sizeof(T) == 4) { o.v[0] = r.x; o.v[1] = r.y; o.v[2] = r.z; o.v[3] = r.w; }
    else { o.v[0] = r.x; o.v[1] = r.y; }
    return o;
}
template <typename T> __device__ __forceinline__ void stp_at(T* p, size_t iv, const Pack<T>& o)
{
    using V = typename V16<T>::type;
    V r;
    if constexpr (sizeof(T) == 4) { r.x = o.v[0]; r.y = o.v[1]; r.z = o.v[2]; r.w = o.v[3]; }
    else { r.x = o.v[0]; r.y = o.v[1]; }
    reinterpret_cast<V*>(p)[iv] = r;
}
// The vectors of one call all start at the SAME element offset of 256-byte aligned allocations (base + vlo), so they share
// their misalignment.  With sequence sharding vlo is a multiple of four elements (set_slices); with column strips (exchange
// mode 4) it is the start of the rank's pair range, L q + pairs q^2 -- any parity.  ALIGNP names one of the vectors: the
// head_ elements in front of its first 16-byte boundary are handled with the tail, one element per thread, and the packs
// start at that boundary (ldp / stp inside the loop body index from there), so every 16-byte access is aligned.
#define ldp(p, iv) ldp_at((p) + head_, iv)
#define stp(p, iv, o) stp_at((p) + head_, iv, o)
#define DCA_VEC_LOOP(n, ALIGNP, BODY_PACK, BODY_TAIL) DCA_VEC_LOOP_G(n, ALIGNP, gridDim.x, BODY_PACK, BODY_TAIL)
/* GRID: the number of workgroups that walk the vector (a launch may carry other workgroups behind them) */
#define DCA_VEC_LOOP_G(n, ALIGNP, GRID, BODY_PACK, BODY_TAIL)                                             \
    {                                                                                                      \
        constexpr int VEC = 16 / (int)sizeof(T);                                                           \
        const size_t lead_ = ((16 - (reinterpret_cast<uintptr_t>(ALIGNP) & 15)) & 15) / sizeof(T);         \
        const size_t head_ = lead_ < (size_t)(n) ? lead_ : (size_t)(n);                                    \
        const size_t nv_ = ((n) - head_) / VEC, stride_ = (size_t)(GRID) * blockDim.x;                     \
        const size_t t0_ = blockIdx.x * (size_t)blockDim.x + threadIdx.x;                                  \
        for (size_t iv = t0_; iv < nv_; iv += stride_) { BODY_PACK }                                       \
        const size_t rest_ = (n) - nv_ * VEC;                     /* head_ + tail, fewer than 2 VEC */      \
        for (size_t r_ = t0_; r_ < rest_; r_ += stride_) {                                                 \
            const size_t i = r_ < head_ ? r_ : r_ + nv_ * VEC;                                             \
            BODY_TAIL                                                                                      \
        }                                                                                                  \
    }

template <typename T>
__global__ void vec_neg_kernel(T* __restrict__ d, const T* __restrict__ g, size_t n)
{
    DCA_VEC_LOOP(n, d,
        Pack<T> a = ldp(g, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) a.v[k] = -a.v[k];
        stp(d, iv, a);,
        d[i] = -g[i];)
}
template <typename T>
__global__ void vec_axpy_kernel(T* __restrict__ y, T a, const T* __restrict__ x, size_t n)
{
    DCA_VEC_LOOP(n, y,
        Pack<T> yy = ldp(y, iv); const Pack<T> xx = ldp(x, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) yy.v[k] += a * xx.v[k];
        stp(y, iv, yy);,
        y[i] += a * x[i];)
}
template <typename T>
__global__ void vec_scale_kernel(T* __restrict__ y, T a, size_t n)
{
    DCA_VEC_LOOP(n, y,
        Pack<T> yy = ldp(y, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) yy.v[k] *= a;
        stp(y, iv, yy);,
        y[i] *= a;)
}
// x = xp + stp*d, as lbfgs.cpp:902-903 (copy, then add the rounded product)
template <typename T>
__global__ void vec_step_kernel(T* __restrict__ x, const T* __restrict__ xp, T stpv, const T* __restrict__ d, size_t n)
{
    DCA_VEC_LOOP(n, x,
        const Pack<T> dd = ldp(d, iv); Pack<T> xx = ldp(xp, iv);
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) { const T v = stpv * dd.v[k]; xx.v[k] = xx.v[k] + v; }
        stp(x, iv, xx);,
        { const T v = stpv * d[i]; x[i] = xp[i] + v; })
}

// ------------------------------------------------------------------ double-double sums (plm_stages.h, lbfgs_kernels.h)
// The objective is summed in double-double (error-free TwoSum): N*L terms in whatever order the kernels meet them
// would otherwise leave ~1e-13 of rounding noise in fx, the line search interpolates on DIFFERENCES of fx, and over 100
// iterations of an optimisation that does not converge that noise grew to 6e-4 in the scores at config E
// (profiles/r03_e_sensitivity_cap100_plain_sums.json).  An (almost) exact sum does not depend on the order: chunked scan, serial
// chain, any sharding and the float64 oracle (Neumaier sums) then see the same fx to the last bit or two.
__device__ __forceinline__ void dd_add(double& hi, double& lo, double v)
{
    const double s = hi + v;
    const double bb = s - hi;
    lo += (hi - (s - bb)) + (v - bb);
    hi = s;
}
__device__ __forceinline__ void dd_add2(double& hi, double& lo, double vh, double vl) { dd_add(hi, lo, vh); lo += vl; }
__device__ __forceinline__ void dd_wave_reduce(double& hi, double& lo)       // fixed tree over the 64 lanes; lane 0 holds the sum
{
    for (int off = 32; off > 0; off >>= 1) {
        const double vh = __shfl_down(hi, off), vl = __shfl_down(lo, off);
        dd_add2(hi, lo, vh, vl);
    }
}

__device__ __forceinline__ void dd_block_reduce(double& hi, double& lo, double* redHi, double* redLo)      // result in thread 0
{
    redHi[threadIdx.x] = hi;
    redLo[threadIdx.x] = lo;
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) dd_add2(redHi[threadIdx.x], redLo[threadIdx.x], redHi[threadIdx.x + st], redLo[threadIdx.x + st]);
        __syncthreads();
    }
    hi = redHi[0];
    lo = redLo[0];
    __syncthreads();
}

}  // namespace
