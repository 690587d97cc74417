// Launch plan of the greedy ascent (ascent.hip): where a chain's local-field table lives, the LDS of both
// kernels and the block of chains that runs at once, each from (F, q, element size, max_steps) and the two environment caps alone.
// Host code only, no HIP header: a host compiler builds it, and tests/ascent_plan_driver.cpp prints it for
// tests/test_ascent_host.py.
#pragma once

#include "potts_plan.h"      // round_up, ceil_div, qm_of, sample_regs

constexpr int kAscThreads = 256;                        // 4 waves: one workgroup of the ascent = one chain
constexpr int kAscInitChains = 256;                     // chains per workgroup of the table pass (lane = chain)
constexpr size_t kAscLdsTotal = 159 * 1024;             // dynamic LDS of the ascent kernel at most: 160 KiB less its static words
constexpr size_t kAscScratchBudget = (size_t)1 << 30;   // the tables (and path records) of one block of chains
constexpr size_t kAscInitChunkBudget = 20 * 1024;       // LDS per J chunk buffer of the table pass (two of them)
constexpr int kAscMaxPass = 1 << 20;                    // chains per block at most

// chunk elements per thread of the table pass: every lane holds all QM accumulators there (as cond_field_regs)
constexpr int asc_init_regs(size_t elem) { return sample_regs(elem) / 2; }

struct AscentPlan {
    int QM, CJ;                 // the table pass: accumulators per lane, blocks per chunk
    size_t ldsInit;             // ... its dynamic LDS: two chunk buffers of CJ blocks of q x QM values
    size_t tableBytes;          // F * q doubles: one chain's table
    size_t sideBytes;           // beside the table in LDS: the site list (F ints) and the free sites' codes (F bytes, to 16)
    bool tableInLds;            // tableBytes <= ldsCap and table + side <= kAscLdsTotal
    size_t ldsAscent;           // dynamic LDS of the ascent kernel
    size_t perChain;            // scratch bytes per chain: the table and, with paths, max_steps records of 16 bytes
};

// ldsCap: the largest table in bytes that may sit in LDS (DCA_ASCENT_LDS; kAscLdsTotal when unset)
inline AscentPlan ascent_plan(int F, int q, size_t elem, size_t ldsCap, bool paths, int max_steps)
{
    AscentPlan p{};
    p.QM = qm_of(q);
    const size_t blkBytes = (size_t)q * p.QM * elem;
    const int R = asc_init_regs(elem);
    p.CJ = std::max(1, std::min((int)(kAscThreads * R / (q * q)), (int)(kAscInitChunkBudget / blkBytes)));
    p.ldsInit = round_up(2 * (size_t)p.CJ * blkBytes, 16);
    p.tableBytes = (size_t)F * q * sizeof(double);
    p.sideBytes = (size_t)F * sizeof(int) + round_up((size_t)F, 16);
    p.tableInLds = p.tableBytes <= ldsCap && p.tableBytes + p.sideBytes <= kAscLdsTotal;
    p.ldsAscent = (p.tableInLds ? p.tableBytes : 0) + p.sideBytes;
    p.perChain = std::max<size_t>(p.tableBytes, 8) + (paths ? (size_t)max_steps * 16 : 0);
    return p;
}

// chains per block: the scratch within kAscScratchBudget (one chain at least), capped by envCap (DCA_ASCENT_PASS; <= 0: unset)
// and by n
inline int ascent_pass_chains(int n, size_t perChain, long envCap)
{
    size_t cap = std::max<size_t>(1, kAscScratchBudget / perChain);
    cap = std::min<size_t>(cap, (size_t)kAscMaxPass);
    if (envCap > 0) cap = std::min(cap, (size_t)envCap);
    return (int)std::min(cap, (size_t)std::max(n, 1));
}
