// Host arithmetic of the Hopfield-Potts fit (hopfield.hip): the launch geometry of the dense operator
// application and of the assembly, the block size of each end's subspace iteration, the likelihood gain and the selection rule.
// No HIP header: a host compiler builds it, tests/hopfield_plan_driver.cpp prints it and tests/test_hopfield_host.py holds it
// against tests/hopfield_reference.py.
#pragma once

#include <cmath>
#include <cstddef>

constexpr int kHpMaxPerEnd = 64;        // patterns per end: the host Jacobi's block k + 8 <= 72 (pca_host.h)
constexpr int kHpMaxStates = 32;        // (q - 1) <= 31: one diagonal block in LDS
constexpr int kHpTile = 16;             // the f64 matrix-core tile: 16 x 16 results from 16 x 4 and 4 x 16 operands
constexpr int kHpApplyRowTiles = 4;     // row tiles of A one wave keeps accumulators for: a workgroup owns 64 rows
constexpr int kHpApplyRows = kHpTile * kHpApplyRowTiles;
constexpr int kHpApplyWaves = 4;        // waves of a workgroup; wave w takes the 16-column steps s = w (mod 4) of the slab
constexpr int kHpApplySlab = 1024;      // columns of A per workgroup: the sums of the slabs are added in ascending order
constexpr int kHpMaxColTiles = 5;       // ceil(72 / 16)
constexpr int kHpAsmTile = 64;          // the assembly's workgroup tile of J: 64 x 64, one wave per 16 rows

struct HpApplyPlan {
    int col_tiles;      // 16-column tiles of V: the kernel instantiation
    int row_groups;     // grid.x
    int slabs;          // grid.y; > 1: partial products, then the ascending sum
    size_t part_doubles;    // doubles of the partial buffer (0 with one slab: the kernel writes Y itself)
};

// fixed by (n, b) alone -- never by the device -- so every sum has one order
inline HpApplyPlan hp_apply_plan(int n, int b)
{
    HpApplyPlan p;
    p.col_tiles = (b + kHpTile - 1) / kHpTile;
    p.row_groups = (n + kHpApplyRows - 1) / kHpApplyRows;
    p.slabs = (n + kHpApplySlab - 1) / kHpApplySlab;
    p.part_doubles = p.slabs > 1 ? (size_t)p.slabs * (size_t)n * (size_t)b : 0;
    return p;
}

// vectors of one end's block: the k wanted and 8 guards, at most the whole space
inline int hp_block(int n, int k) { return k <= 0 ? 0 : (n < k + 8 ? n : k + 8); }

// the likelihood gain of a pattern, Delta L = (lambda - 1 - ln lambda) / 2
inline double hp_gain(double lambda) { return 0.5 * (lambda - 1.0 - std::log(lambda)); }

// The p patterns of largest gain from the two ends of a spectrum: top[0 .. nt) descending eigenvalues (the largest), bot[0 .. nb)
// ascending (the smallest).  Equal gains go to the attractive side.  Writes how many are taken from each end and returns 0; -1
// when an end runs out before p are taken (the caller then holds too few eigenvalues of that end to know the answer).
inline int hp_select_likelihood(const double* top, int nt, const double* bot, int nb, int p, int* take_top, int* take_bot)
{
    int i = 0, j = 0;
    while (i + j < p) {
        if (i >= nt || j >= nb) return -1;
        if (hp_gain(top[i]) >= hp_gain(bot[j])) ++i; else ++j;
    }
    *take_top = i;
    *take_bot = j;
    return 0;
}
