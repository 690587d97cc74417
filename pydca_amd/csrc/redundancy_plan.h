// Launch plan of the redundancy filter and the identity clusters (redundancy.hip): the block of rank
// positions the filter resolves at once, the tiles its launches cover in the worst case, the LDS of its kernels, and whether
// the clusters keep their similarity bits on the device -- each from (n, q) and the two environment values alone.
// Host code only, no HIP header: a host compiler builds it, and tests/redundancy_plan_driver.cpp prints it for
// tests/test_redundancy_host.py.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

constexpr int kRedTile = 64;                  // sequences per tile side (hamming_kernel's)
constexpr int kRedKG = 4;                     // 32-site groups per LDS stage
constexpr int kRedSuper = 32;                 // tiles per super-tile side of the 1-D tile walk
constexpr int kRedThreads = 256;              // 4 waves per tile, a 4 x 4 register block per lane
constexpr int kFilterBlockDefault = 2048;     // rank positions per block of the filter
constexpr int kFilterBlockMax = 8192;         // ... at most: the resolve pass keeps 4 bytes per position in LDS (32 KiB)
constexpr unsigned long long kClusterBitsMaxDefault = 8ull << 30;      // DCA_CLUSTER_BITS_MAX when unset

constexpr int red_planes(int q) { return q <= 8 ? 3 : 5; }
constexpr int red_planes_padded(int q) { return (red_planes(q) + 1) & ~1; }
// static LDS of a tile kernel: two staging buffers of 64 rows, row stride kRedKG * PLP + 2 dwords (8-byte reads, conflict free)
constexpr size_t red_tile_lds(int q) { return 2 * (size_t)kRedTile * (kRedKG * red_planes_padded(q) + 2) * sizeof(uint32_t); }

inline int red_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

struct FilterPlan {
    int B;                  // rank positions per block: a multiple of 64
    int blocks;             // ceil(n / B)
    int W;                  // dwords per row of a block's similarity bits: B / 32
    long long tilePairs;    // 64 x 64 tiles launched: per block its own tq^2 and the worst-case cover tq * ceil(p0 / 64)
    size_t ldsResolve;      // dynamic LDS of the resolve pass: 4 bytes per position
    size_t bitsBytes;       // the block's similarity bits
};

// envBlock: DCA_FILTER_BLOCK (<= 0: unset); rounded up to a multiple of 64, at most kFilterBlockMax and n rounded up to 64
inline FilterPlan filter_plan(int n, long envBlock)
{
    FilterPlan p{};
    long b = envBlock > 0 ? envBlock : kFilterBlockDefault;
    b = std::min<long>(b, kFilterBlockMax);
    b = (b + kRedTile - 1) / kRedTile * kRedTile;
    const long nUp = ((long)std::max(n, 1) + kRedTile - 1) / kRedTile * kRedTile;
    p.B = (int)std::min(b, nUp);
    p.blocks = red_ceil_div(std::max(n, 1), p.B);
    p.W = p.B / 32;
    for (long long p0 = 0; p0 < n; p0 += p.B) {
        const long long tq = red_ceil_div(std::min<long long>(p.B, n - p0), kRedTile);
        p.tilePairs += tq * tq + tq * red_ceil_div(p0, kRedTile);
    }
    p.ldsResolve = (size_t)p.B * sizeof(uint32_t);
    p.bitsBytes = (size_t)p.B * p.W * sizeof(uint32_t);
    return p;
}

struct ClusterPlan {
    int tiles;                      // ceil(n / 64)
    int W;                          // dwords per stored row: 2 * tiles (a tile owns whole dwords)
    unsigned long long bitsBytes;   // n * ceil(n / 32) * 4: what the cap is compared with
    unsigned long long allocDwords; // 64 * tiles * W: the rows padded to whole tiles
    bool stored;                    // bitsBytes <= cap
    unsigned long long units;       // (wave, 32-site group) units of one pass over all tile pairs, per group of the padded row
};

// cap: DCA_CLUSTER_BITS_MAX in bytes
inline ClusterPlan cluster_plan(int n, unsigned long long cap)
{
    ClusterPlan p{};
    p.tiles = red_ceil_div(std::max(n, 1), kRedTile);
    p.W = 2 * p.tiles;
    p.bitsBytes = (unsigned long long)n * (unsigned long long)red_ceil_div(n, 32) * 4ull;
    p.allocDwords = (unsigned long long)kRedTile * p.tiles * p.W;
    p.stored = p.bitsBytes <= cap;
    p.units = (unsigned long long)p.tiles * p.tiles * 4ull;
    return p;
}

// workgroups of the 1-D super-tile walk over tilesQ x tilesR tiles
inline unsigned long long red_walk_blocks(int tilesQ, int tilesR)
{
    return (unsigned long long)red_ceil_div(tilesQ, kRedSuper) * red_ceil_div(tilesR, kRedSuper) * kRedSuper * kRedSuper;
}
