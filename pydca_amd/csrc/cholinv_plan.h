// Launch decisions of the SPD inverse (cholinv.hip): which product kernel a launch takes, how the fused recursion splits and
// where it forks its side-stream product, when the block sweep runs, in which form and over which panels -- each from the
// sizes alone.
// Host code only, no HIP header: a host compiler builds it, and tests/cholinv_plan_driver.cpp prints every launch of one inverse
// for tests/spd_inverse_reference.py, whose case table and float64 restatement are held to these decisions.
#pragma once

#include <climits>
#include <cstddef>
#include <vector>

enum { MASK_NONE = 0, MASK_LOWER = 1 /* k <= row */, MASK_UPPER = 2 /* k >= row */ };

enum { WALK_ROWS = 0, WALK_ROWS_REVERSED = 1 /* lower triangular A */, WALK_COLUMNS_REVERSED = 2 /* lower triangular B; grid transposed */ };

// ---- the product kernels
enum CholForm {
    CHOL_SMALL32 = 0,      // gemm_nt_f64_small_kernel: 32 x 32 tiles, deep k
    CHOL_SMALL32_PAIR,     // gemm_nt_f64_small_pair_kernel: two such products in one launch
    CHOL_DMA64,            // gemm_nt_f64_dma_kernel<2>: 64 x 64 tiles
    CHOL_DMA128,           // gemm_nt_f64_dma_kernel<4>: 128 x 128 tiles
    CHOL_DMA128x64,        // gemm_nt_f64_dma_kernel<4, 2>: 128 x 64 tiles
    CHOL_DMA128_BANDED,    // gemm_nt_f64_dma_kernel<4> in bands of tile rows on the side stream (launch_gemm_banded)
    CHOL_FORMS
};
inline const char* chol_form_name(int f)
{
    static const char* const names[CHOL_FORMS] = {"small32", "small32pair", "dma64", "dma128", "dma128x64", "dma128banded"};
    return f >= 0 && f < CHOL_FORMS ? names[f] : "?";
}

// Products of at most kSmall32Max 64 x 64 tiles run on 32 x 32 tiles, the rest by LDS-DMA.  Inverse at n = 10 048 / 4000 by
// this bound: 0 -> 27.1 / 4.96 ms, 16 -> 25.8 / 4.36, 128 -> 24.7 / 4.08, 400 -> 24.2 / 3.95, 1200 -> 23.9 / 4.01,
// 1600 -> 24.8 / 3.99.
constexpr int kSmall32Max = 400;
// The block sweep's chain runs NEXT TO its update launches: there the few-tile products do better as fewer, larger workgroups
// (n = 10 048: 21.4 -> 20.6 ms with the bound at 16), so the sweep lowers the bound for the launches it makes
constexpr int kSweepSmall32Max = 16, kSweepSmall32MinN = 6000;
inline int chol_small32_max_in_sweep(int n) { return n >= kSweepSmall32MinN ? kSweepSmall32Max : kSmall32Max; }

// 64 x 64 tiles of a product's grid (all of them, also where lowerOnly leaves the upper ones idle)
inline long long chol_tiles64(int M, int N) { return (long long)(M / 64) * (N / 64); }

// both products on 32 x 32 tiles in ONE launch when each is small enough for that kernel
inline bool chol_pair_fits(int M0, int N0, int M1, int N1, int small32Max)
{
    return chol_tiles64(M0, N0) <= small32Max && chol_tiles64(M1, N1) <= small32Max;
}

// the kernel of one product launch (launch_gemm_on)
inline CholForm chol_product_form(int M, int N, int maskA, int maskB, int lowerOnly, int walk, int small32Max)
{
    // the launch grid: x counts tile columns, except in the transposed walk
    const long long gridX = walk == WALK_COLUMNS_REVERSED ? M / 64 : N / 64, gridY = walk == WALK_COLUMNS_REVERSED ? N / 64 : M / 64;
    if (gridX * gridY <= small32Max) return CHOL_SMALL32;       // far fewer tiles than CUs: 32 x 32 tiles on four times as many CUs
    // 128 x 128 tiles: 16 instead of 8 flop per operand byte (the 64 x 64 kernel sits at the L2 -> LDS fill limit), but a
    // quarter of the tiles on half of the slots: taken when the rounds of equal tiles still fill up
    const long long t64 = lowerOnly ? gridX * (gridX + 1) / 2 : gridX * gridY;
    const long long gx = (gridX + 1) / 2, gy = (gridY + 1) / 2;
    const long long t128 = lowerOnly ? gx * (gx + 1) / 2 : gx * gy;
    auto fill = [](long long t, long long slots) { return (double)t / (double)(((t + slots - 1) / slots) * slots); };
    // measured inside the inverse at n = 10 048 (kernel trace, 64 vs 128): SYRK 2.84 -> 2.61 ms, L21 / T^T 2.26 -> 2.19,
    // X21 2.40 -> 2.29, but X^T X (both operands triangular: the 128-tiles waste work along two diagonals) 6.10 -> 7.05
    const int masks = (maskA != MASK_NONE) + (maskB != MASK_NONE);
    bool use128 = false;
    if (masks == 0) use128 = t128 >= 512 && fill(t128, 512) * 66.0 > fill(t64, 1024) * 59.0;
    else if (masks == 1) use128 = t128 >= 1024;
    // two triangular operands: 128 x 64 tiles
    if (!use128 && walk != WALK_COLUMNS_REVERSED && masks == 2 && gridX * gridY >= 2048) return CHOL_DMA128x64;
    return use128 ? CHOL_DMA128 : CHOL_DMA64;
}

// ---- the fused recursion (cholinv_rec)
// 64 or 128: the node is a leaf of that size; 0: it splits
inline int chol_leaf(int n) { return n == 64 || n == 128 ? n : 0; }
// halves in multiples of 128 where possible, so that the recursion ends in 128-leaves (a 64-leaf only where n is an odd
// multiple of 64)
inline int chol_split(int n) { return n >= 256 ? (n / 128 / 2) * 128 : (n / 64 / 2) * 64; }

// Workgroups per launch of the background product and the smallest first half that forks one.  Measured at n = 10 048 (inverse,
// ms; 24.4 - 24.6 without): at the top level alone 40 / 80 / 120 / 240 workgroups 32.3 / 26.1 / 24.6 / 23.7 (a slow
// background product is waited for at the join); any background one or two levels down loses -- their subtrees are chains of
// few-tile products that share CUs with it (0,40,10: 36.0, 0,0,10: 25.5 without stream priorities) -- so only the top
// level overlaps: n = 8000: 14.7 -> 14.5, n = 6000: 7.6 -> 7.5, n = 4000: unchanged
constexpr int kSideWGs = 240, kSideMinN1 = 1024;
// a node's T^T goes to the side stream: not when it went out paired with the SYRK, only with a side set (the top level)
inline bool chol_fork_side(bool paired, bool haveSide, int n1) { return !paired && haveSide && n1 >= kSideMinN1; }
// the bands of launch_gemm_banded: 128-row tile rows per launch
inline int chol_band_rows(int N, int maxWGs) { const int gx = (N + 127) / 128, band = maxWGs / gx; return band > 1 ? band : 1; }
// a set of side streams is asked for where one will be used: the sweep, and the recursion's top level from here on
constexpr int kSideSetMinN = 2048;
inline bool chol_wants_side_set(int n, bool wantSweep) { return n >= kSideSetMinN || wantSweep; }

// ---- the block sweep (cholinv_sweep)
struct SweepCfg { int minN, wide, narrow, wideMinN, cap, prioCap, factorMaxN; };
// measured (ms, sweep / three-phase): n = 2048 1.43 / 1.30, 3072 2.16 / 2.31, 4032 3.41 / 3.55, 6016 6.46 / 7.54, 8000 12.25 / 13.25, 10 048 20.6 / 22.4, 12 032 34.0 / 34.9
inline SweepCfg sweep_cfg_defaults() { return SweepCfg{2560, 512, 256, 7000, 0, 64, 4500}; }

inline int sweep_panel_width(int n, const SweepCfg& c) { return n >= c.wideMinN ? c.wide : c.narrow; }
// doubles of the sweep's workspace against the 2 n^2 the caller provides: W[2] | Q[2] | P[2] | S[2] | Wn | arena of the
// recursion on a pivot block | tile counters
inline bool sweep_workspace_fits(int n, int B, int np) { return (size_t)4 * n * B + (size_t)7 * B * B + (size_t)np * 8 + 8 <= (size_t)2 * n * n; }
inline bool sweep_wanted(int n, const SweepCfg& c)
{
    const int B = sweep_panel_width(n, c);
    return n >= c.minN && n >= 2 * B && sweep_workspace_fits(n, B, n / B + 2);
}
// below factorMaxN (chain-bound sizes): the next pivot block from X (F F^T), P on the side stream
inline bool sweep_factor_form(int n, const SweepCfg& c) { return n < c.factorMaxN; }
// panel p holds the pivot columns [b[p], b[p + 1])
inline std::vector<int> sweep_panels(int n, int B)
{
    std::vector<int> b;
    for (int c = 0; c < n; c += B) b.push_back(c);
    b.push_back(n);
    return b;
}
