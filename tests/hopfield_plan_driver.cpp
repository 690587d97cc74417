// TEST INFRASTRUCTURE ONLY: the host arithmetic of the Hopfield-Potts fit (pydca_amd/csrc/hopfield_plan.h, host code that
// hopfield.hip and mf_engine.hip run) as a stand-alone program.  tests/test_hopfield_host.py compiles it with the host compiler.
//   hopfield_plan_driver plan n b k [...]     one line of "key value" pairs per group of three:
//       n b k colTiles rowGroups slabs partDoubles block maxPerEnd maxBlock rows slab waves asmTile
//   hopfield_plan_driver gain lambda [...]    one line per eigenvalue: the likelihood gain with 17 significant digits
//   hopfield_plan_driver select p nt nb top[0] .. top[nt-1] bot[0] .. bot[nb-1]     prints "rc takeTop takeBot"
#include "hopfield_plan.h"
#include "pca_host.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char** argv)
{
    if (argc >= 5 && !std::strcmp(argv[1], "plan") && (argc - 2) % 3 == 0) {
        for (int i = 2; i < argc; i += 3) {
            const int n = std::atoi(argv[i]), b = std::atoi(argv[i + 1]), k = std::atoi(argv[i + 2]);
            const HpApplyPlan p = hp_apply_plan(n, b);
            std::printf("n %d b %d k %d colTiles %d rowGroups %d slabs %d partDoubles %zu block %d maxPerEnd %d maxBlock %d rows %d slab %d "
                        "waves %d asmTile %d\n", n, b, k, p.col_tiles, p.row_groups, p.slabs, p.part_doubles, hp_block(n, k), kHpMaxPerEnd,
                        kPcaMaxBlock, kHpApplyRows, kHpApplySlab, kHpApplyWaves, kHpAsmTile);
        }
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "gain")) {
        for (int i = 2; i < argc; ++i) std::printf("%.17g\n", hp_gain(std::atof(argv[i])));
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "select")) {
        const int p = std::atoi(argv[2]), nt = std::atoi(argv[3]), nb = std::atoi(argv[4]);
        if (nt < 0 || nb < 0 || argc != 5 + nt + nb) { std::fprintf(stderr, "select: %d values expected\n", nt + nb); return 2; }
        std::vector<double> top(nt), bot(nb);
        for (int i = 0; i < nt; ++i) top[i] = std::atof(argv[5 + i]);
        for (int i = 0; i < nb; ++i) bot[i] = std::atof(argv[5 + nt + i]);
        int a = -1, r = -1;
        const int rc = hp_select_likelihood(top.data(), nt, bot.data(), nb, p, &a, &r);
        std::printf("%d %d %d\n", rc, a, r);
        return 0;
    }
    std::fprintf(stderr, "usage: %s plan n b k [...] | gain lambda [...] | select p nt nb top.. bot..\n", argv[0]);
    return 2;
}
