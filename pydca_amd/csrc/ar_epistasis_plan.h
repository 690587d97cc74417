// Launch geometry of the tiled product kernel of the arDCA epistasis (epi_main_kernel of ar_epistasis.hip): the tile constants,
// the tiles that are launched and their order, a tile's first streamed site and step count, the values a thread stages per
// step and the dynamic LDS.  Host code only, no HIP header: a host compiler builds it, and tests/ar_epistasis_plan_driver.cpp
// prints it for tests/test_ar_epistasis_audit_host.py, which holds the audit's case table to these numbers.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

constexpr int kEpiThreads = 512;
constexpr int kEpiRows = 4, kEpiCols = 4;                 // elements per thread: rows tr * 4 + i, columns tc + 16 j
constexpr int kEpiTileR = kEpiThreads / 16 * kEpiRows;    // 128 flattened rows (k, a) per workgroup
constexpr int kEpiTileC = 16 * kEpiCols;                  // 64 flattened columns (l, b)
constexpr int kEpiRescale = 4;                            // steps between exponent splits (a power of two)

// values of one staged site (QM-wide rows of both runs) per thread: the registers of the prefetch
constexpr int epi_npre(int QM) { return ((kEpiTileR + kEpiTileC) * QM + kEpiThreads - 1) / kEpiThreads; }

// dynamic LDS: two buffers of (128 + 64) rows of q doubles
inline size_t epi_lds_bytes(int q) { return (size_t)2 * (kEpiTileR + kEpiTileC) * q * sizeof(double); }

// (row tile, column tile); the layout of the int2 the kernel reads
struct alignas(8) EpiTile { int x, y; };

// the first later site a column tile streams (the site after its first column's; a column joins once m > its own site) and the
// number of sites it streams (constexpr: the kernel calls them too)
constexpr int epi_mstart(int ct, int q) { return ct * kEpiTileC / q + 1; }
constexpr int epi_steps(int ct, int L, int q) { return L - epi_mstart(ct, q); }

// the tiles that hold a pair k < l, heaviest (most later sites to stream: the lowest column tile) first
inline std::vector<EpiTile> epistasis_tiles(int L, int q)
{
    const int Lq = L * q;
    std::vector<EpiTile> tiles;
    for (int ct = 0; ct * kEpiTileC < Lq; ++ct) {
        const int lmax = std::min(Lq - 1, ct * kEpiTileC + kEpiTileC - 1) / q;
        for (int rt = 0; rt * kEpiTileR < Lq && rt * kEpiTileR / q < lmax; ++rt) tiles.push_back(EpiTile{rt, ct});
    }
    return tiles;
}
