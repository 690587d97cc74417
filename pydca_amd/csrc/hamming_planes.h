// The bit-plane builder of the Hamming kernels (distance.hip, redundancy.hip): rows in file order, no column permutation.
// The layout is that of weights.hip: per sequence and 32-site group PL dwords (5 for q <= 32, 3 for q <= 8), padded to the even
// PLP, dword p holding bit p of the 32 states.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

// rows of `stride` bytes, the first L of them codes -> planes P[(n * G + g) * PLP + p], sites past L as state 0 in every row
template <int PL>
__global__ __launch_bounds__(256)
void nn_bitplanes_kernel(const uint8_t* __restrict__ X, size_t stride, int L, uint32_t* __restrict__ P, int N, int G)
{
    constexpr int PLP = (PL + 1) & ~1;
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)N * G) return;
    const size_t n = idx / G;
    const int g = (int)(idx % G);
    const uint8_t* row = X + n * stride;
    uint32_t planes[PL];
#pragma unroll
    for (int p = 0; p < PL; ++p) planes[p] = 0;
    for (int k = 0; k < 32; ++k) {
        const int j = g * 32 + k;
        const uint32_t st = j < L ? row[j] : 0u;
#pragma unroll
        for (int p = 0; p < PL; ++p) planes[p] |= ((st >> p) & 1u) << k;
    }
#pragma unroll
    for (int p = 0; p < PLP; ++p) P[idx * PLP + p] = p < PL ? planes[p] : 0u;
}

}  // namespace
