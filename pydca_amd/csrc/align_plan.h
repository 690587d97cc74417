// Launch plan of the profile aligner (align.hip): the strip width T, the LDS image of the match table and
// whether it is staged whole or strip by strip, the scratch a query costs and the queries one pass may hold -- each from
// (Lp, A), the longest query, whether a traceback is wanted and DCA_ALIGN_PASS alone.
// Host code only, no HIP header: a host compiler builds it, and tests/align_plan_driver.cpp prints it for
// tests/test_profile_align_host.py.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr int kAlignWaves = 4;                          // waves per workgroup: they share the LDS image of the match table
constexpr int kAlignThreads = 64 * kAlignWaves;
constexpr int kAlignMaxLp = 8192;
constexpr int kAlignMaxA = 32;
constexpr int kAlignMaxLen = 32767;
constexpr int kAlignNeg = -(1 << 28);                   // "minus infinity" of the recurrence, as in the host aligner
constexpr size_t kAlignLdsWhole = 64u << 10;            // a whole table may take this much: two workgroups still share a CU
constexpr size_t kAlignLdsMax = 160u << 10;             // the CU's LDS
constexpr unsigned long long kAlignScratchMax = 1ull << 30;      // edge columns + pointer bits of one pass

struct AlignPlan {
    int T;                          // profile columns per register strip: 16 or 32
    int strips;                     // ceil(Lp / T)
    int LpPad;                      // strips * T
    bool whole;                     // the whole match table sits in LDS; otherwise one strip's slice at a time
    int ldsStride;                  // dwords between the rows (one per code) of the LDS image: = 4 mod 16, so 16 rows spread over all banks
    size_t ldsBytes;                // dynamic LDS of the DP kernel
    unsigned long long bytesPerResidue;     // scratch per query residue: 8 (edge column: H and D) + with traceback strips * T / 2 (4 bits per cell)
};

// T = 32 halves the edge-column traffic and the loop overhead per cell; below 64 columns its padding would waste more than that
inline AlignPlan align_plan(int Lp, int A, bool traceback)
{
    AlignPlan p{};
    p.T = Lp >= 64 ? 32 : 16;
    p.strips = (Lp + p.T - 1) / p.T;
    p.LpPad = p.strips * p.T;
    const size_t wholeBytes = (size_t)A * (p.LpPad + 4) * sizeof(int32_t);
    p.whole = wholeBytes <= kAlignLdsWhole;
    p.ldsStride = (p.whole ? p.LpPad : p.T) + 4;
    p.ldsBytes = (size_t)A * p.ldsStride * sizeof(int32_t);
    p.bytesPerResidue = 8ull + (traceback ? (unsigned long long)p.strips * p.T / 2 : 0ull);
    return p;
}

// scratch of one query in a wave whose longest query has maxLen residues (every lane of a wave owns maxLen slots)
inline unsigned long long align_bytes_per_query(const AlignPlan& p, int maxLen)
{
    return p.bytesPerResidue * (unsigned long long)std::max(maxLen, 1);
}

// queries of the next pass when the longest remaining query has maxLen residues.  envPass: DCA_ALIGN_PASS (<= 0: unset).
// Never less than 1: the largest single query (8192 columns x 32767 residues) takes 128.3 MiB.
inline long long align_queries_per_pass(const AlignPlan& p, int maxLen, long long envPass)
{
    long long q = (long long)(kAlignScratchMax / align_bytes_per_query(p, maxLen));
    q = std::min<long long>(q, 1ll << 24);                // 2^18 waves: far inside a grid's range
    if (envPass > 0) q = std::min(q, envPass);
    return std::max<long long>(q, 1);
}

// the argument check that keeps every partial sum away from kAlignNeg: (max|match| + max|penalty|) * (Lp + 32767) < 2^28
inline bool align_values_in_range(long long maxAbsMatch, long long maxAbsPenalty, int Lp)
{
    return (maxAbsMatch + maxAbsPenalty) * ((long long)Lp + kAlignMaxLen) < (1ll << 28);
}
