// TEST INFRASTRUCTURE ONLY: the launch decisions of the SPD inverse (pydca_amd/csrc/cholinv_plan.h, host code that cholinv.hip
// launches by) as a stand-alone program.  tests/spd_inverse_reference.py compiles it with the host compiler.
// cholinv_plan_driver n minN wide narrow wideMinN factorMaxN   (n: the padded size, a multiple of 64; the rest: SweepCfg)
// (cholinv_plan_driver forms  prints the names of all product forms of the header; cholinv_plan_driver defaults  prints
// sweep_cfg_defaults() as minN wide narrow wideMinN factorMaxN.)
// prints, in issue order, one line per launch of one inverse of that size:
//   inverse n swept B factorForm sideSet small32Max
//   panel p c w                                              a step of the block sweep begins: pivot columns [c, c + w)
//   leaf size buf off pivotBase stream                       X = inv(chol(.)) of buf[off : off + size, off : off + size]
//   gemm tag form buf off M N K maskA maskB lowerOnly walk stream cin
//   update kind p tiles stream                               the sweep's rank-w update: kind prio / rest, length of the tile list
// buf: A the matrix itself, S the sweep's copy of the pivot block (off is then relative to the block).  tag names the product:
// L21, SYRK, TT, X21 of the recursion node at off (tile counts n1 = K of L21, n2 = M of L21), XTX the final X^T X, and of a sweep
// step P, WN (the next pivot rows times P or X^T), S (the next pivot block), W.  stream: chain, side (the recursion's background
// product; the sweep's side stream), rest.  cin: the addend of a beta = 1 product is read from the matrix, not from the output.
#include "cholinv_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

static int g_small32 = kSmall32Max;

static void gemm(const char* tag, const char* buf, int off, int M, int N, int K, int maskA, int maskB, int lowerOnly, int walk, const char* stream,
                 int cin = 0, int forced = -1)
{
    const int form = forced >= 0 ? forced : (int)chol_product_form(M, N, maskA, maskB, lowerOnly, walk, g_small32);
    std::printf("gemm %s %s %s %d %d %d %d %d %d %d %d %s %d\n", tag, chol_form_name(form), buf, off, M, N, K, maskA, maskB, lowerOnly, walk, stream, cin);
}

// cholinv_rec on buf[off : off + n, off : off + n]
static void rec(const char* buf, int off, int n, int pivotBase, bool side)
{
    if (chol_leaf(n)) { std::printf("leaf %d %s %d %d chain\n", n, buf, off, pivotBase); return; }
    const int n1 = chol_split(n), n2 = n - n1;
    rec(buf, off, n1, pivotBase, false);
    gemm("L21", buf, off, n2, n1, n1, MASK_NONE, MASK_LOWER, 0, WALK_COLUMNS_REVERSED, "chain");
    const bool paired = chol_pair_fits(n2, n2, n1, n2, g_small32);
    if (paired) {
        gemm("SYRK", buf, off, n2, n2, n1, MASK_NONE, MASK_NONE, 1, WALK_ROWS, "chain", 0, CHOL_SMALL32_PAIR);
        gemm("TT", buf, off, n1, n2, n1, MASK_UPPER, MASK_NONE, 0, WALK_ROWS, "chain", 0, CHOL_SMALL32_PAIR);
    }
    const bool onSide = chol_fork_side(paired, side, n1);
    if (onSide) {
        // bands of launch_gemm_banded, one line each
        const int gy = (n1 + 127) / 128, band = chol_band_rows(n2, kSideWGs);
        for (int r = 0; r < gy; r += band)
            std::printf("gemm TT %s %s %d %d %d %d %d %d %d %d side 0\n", chol_form_name(CHOL_DMA128_BANDED), buf, off, std::min(band * 128, n1 - r * 128), n2, n1,
                        MASK_UPPER, MASK_NONE, 0, WALK_ROWS);
    }
    if (!paired) gemm("SYRK", buf, off, n2, n2, n1, MASK_NONE, MASK_NONE, 1, WALK_ROWS, "chain");
    rec(buf, off + n1, n2, pivotBase + n1, false);
    if (!onSide && !paired) gemm("TT", buf, off, n1, n2, n1, MASK_UPPER, MASK_NONE, 0, WALK_ROWS, "chain");
    gemm("X21", buf, off, n2, n1, n2, MASK_LOWER, MASK_NONE, 0, WALK_ROWS_REVERSED, "chain");
}

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "forms") {      // every form the header can return
        for (int f = 0; f < CHOL_FORMS; ++f) std::printf("%s\n", chol_form_name(f));
        return 0;
    }
    if (argc == 2 && std::string(argv[1]) == "defaults") {   // SweepCfg as the library starts from it, in the order of the arguments
        const SweepCfg d = sweep_cfg_defaults();
        std::printf("%d %d %d %d %d\n", d.minN, d.wide, d.narrow, d.wideMinN, d.factorMaxN);
        return 0;
    }
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s n minN wide narrow wideMinN factorMaxN\n", argv[0]);
        return 2;
    }
    const int n = std::atoi(argv[1]);
    SweepCfg cfg = sweep_cfg_defaults();
    cfg.minN = std::atoi(argv[2]); cfg.wide = std::atoi(argv[3]); cfg.narrow = std::atoi(argv[4]); cfg.wideMinN = std::atoi(argv[5]);
    cfg.factorMaxN = std::atoi(argv[6]);
    if (n <= 0 || n % 64 != 0 || cfg.wide < 128 || cfg.narrow < 128 || cfg.wide % 128 != 0 || cfg.narrow % 128 != 0) {
        std::fprintf(stderr, "need n a positive multiple of 64 and panels of multiples of 128 columns\n");
        return 2;
    }
    const bool swept = sweep_wanted(n, cfg);      // (a side set is always to be had here)
    const int B = sweep_panel_width(n, cfg);
    const bool factorForm = sweep_factor_form(n, cfg);
    if (swept) g_small32 = chol_small32_max_in_sweep(n);
    std::printf("inverse %d %d %d %d %d %d\n", n, swept ? 1 : 0, swept ? B : 0, swept && factorForm ? 1 : 0, chol_wants_side_set(n, swept) ? 1 : 0, g_small32);
    if (!swept) {
        rec("A", 0, n, 0, chol_wants_side_set(n, swept));
        gemm("XTX", "A", 0, n, n, n, MASK_UPPER, MASK_UPPER, 1, WALK_ROWS, "chain");
        return 0;
    }
    const std::vector<int> b = sweep_panels(n, B);
    const int np = (int)b.size() - 1, nt = (n + 127) / 128;
    if (!sweep_workspace_fits(n, B, np)) { std::printf("nomem\n"); return 0; }
    for (int p = 0; p < np; ++p) {
        const int c = b[p], w = b[p + 1] - c;
        const bool last = p + 1 == np;
        const int c1 = last ? n : b[p + 1], w1 = last ? 0 : b[p + 2] - c1;
        const int c2 = c1 + w1, w2 = (last || p + 2 == np) ? 0 : b[p + 3] - c2;
        std::printf("panel %d %d %d\n", p, c, w);
        rec("S", 0, w, c, false);
        if (!factorForm) gemm("P", "S", 0, w, w, w, MASK_UPPER, MASK_UPPER, 1, WALK_ROWS, "chain");
        if (!last) {
            if (factorForm) gemm("WN", "A", c1, w1, w, w, MASK_NONE, MASK_LOWER, 0, WALK_COLUMNS_REVERSED, "chain");
            else gemm("WN", "A", c1, w1, w, w, MASK_NONE, MASK_NONE, 0, WALK_ROWS, "chain");
            gemm("S", "A", c1, w1, w1, w, MASK_NONE, MASK_NONE, 1, WALK_ROWS, "chain", factorForm ? 1 : 0);
        }
        if (factorForm) gemm("P", "S", 0, w, w, w, MASK_UPPER, MASK_UPPER, 1, WALK_ROWS, "side");
        gemm("W", "A", c, n, w, w, MASK_NONE, MASK_NONE, 0, WALK_ROWS, "side");
        // the tile lists of sweep_update_kernel (cholinv_sweep)
        const int skip0 = c / 128;
        int skipN = (c1 + w1 + 127) / 128 - c / 128, prN = (c1 + w1 + 127) / 128 - c1 / 128;
        const int dgN = w2 > 0 ? (c2 + w2 + 127) / 128 - c2 / 128 : 0;
        if (w1 == 0) { prN = 0; skipN = nt - skip0; }
        const int nR = nt - skipN;
        if (!last) std::printf("update prio %d %d side\n", p, prN * nR + dgN * (dgN + 1) / 2);
        if (nR > 0) { const int bands = (nR + 3) / 4; std::printf("update rest %d %d rest\n", p, 8 * bands * bands + 2 * bands); }
    }
    return 0;
}
