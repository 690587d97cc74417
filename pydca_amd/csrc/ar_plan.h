// Launch geometry of the arDCA coupling gradient (ar_grad_kernel of ardca.hip): how many earlier sites one workgroup takes,
// its thread count and its LDS.  Host code only, no HIP header: a host compiler builds it, and tests/ar_plan_driver.cpp prints
// it for tests/test_ardca_eval_audit_host.py, which holds the audit's case table to these numbers.
#pragma once

#include <algorithm>
#include <cstddef>

constexpr int kGTile = 64;                         // sequences per staged tile of the coupling gradient
constexpr size_t kGBlockBudget = 56 * 1024;        // LDS of the gradient blocks of one workgroup
constexpr int kGMaxThreads = 512;

// earlier sites k per workgroup: their q x q blocks within kGBlockBudget, one thread per column of a block, 64 at most
inline int grad_chunk(int q)
{
    return std::max(1, std::min({64, (int)(kGBlockBudget / ((size_t)q * q * sizeof(double))), kGMaxThreads / q}));
}

// KC = grad_chunk(q); threads: KC q columns rounded up to whole waves (the rest idle); lds: KC q^2 + 64 q doubles (the blocks,
// one tile of residual rows), then KC x 64 code bytes
struct ArGradPlan { int KC, threads; size_t lds; };

inline ArGradPlan ar_grad_plan(int q)
{
    const int KC = grad_chunk(q);
    const int threads = (KC * q + 63) / 64 * 64;
    const size_t lds = ((size_t)KC * q * q + (size_t)kGTile * q) * sizeof(double) + (size_t)KC * kGTile;
    return {KC, threads, lds};
}
