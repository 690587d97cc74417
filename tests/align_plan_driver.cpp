// TEST INFRASTRUCTURE ONLY: the launch plan of the profile aligner (pydca_amd/csrc/align_plan.h, host code that align.hip runs)
// as a stand-alone program.  tests/test_profile_align_host.py compiles it with the host compiler.
// align_plan_driver Lp A traceback maxLen envPass [...] prints one line of "key value" pairs per group of five
// (envPass <= 0: DCA_ALIGN_PASS unset):
//   T strips LpPad whole ldsStride ldsBytes bytesPerResidue bytesPerQuery queriesPerPass passBytes waves ldsWhole ldsMax scratchMax
#include "align_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 6 || (argc - 1) % 5 != 0) {
        std::fprintf(stderr, "usage: %s Lp A traceback maxLen envPass [...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; i += 5) {
        const int Lp = std::atoi(argv[i]), A = std::atoi(argv[i + 1]), trace = std::atoi(argv[i + 2]), maxLen = std::atoi(argv[i + 3]);
        const long long envPass = std::atoll(argv[i + 4]);
        if (Lp < 1 || Lp > kAlignMaxLp || A < 2 || A > kAlignMaxA || maxLen < 0 || maxLen > kAlignMaxLen) {
            std::fprintf(stderr, "Lp in 1..8192, A in 2..32, maxLen in 0..32767\n");
            return 2;
        }
        const AlignPlan p = align_plan(Lp, A, trace != 0);
        const unsigned long long perQuery = align_bytes_per_query(p, maxLen);
        const long long perPass = align_queries_per_pass(p, maxLen, envPass);
        std::printf("Lp %d A %d T %d strips %d LpPad %d whole %d ldsStride %d ldsBytes %zu bytesPerResidue %llu bytesPerQuery %llu "
                    "queriesPerPass %lld passBytes %llu waves %d ldsWhole %zu ldsMax %zu scratchMax %llu\n",
                    Lp, A, p.T, p.strips, p.LpPad, (int)p.whole, p.ldsStride, p.ldsBytes, p.bytesPerResidue, perQuery, perPass,
                    perQuery * (unsigned long long)perPass, kAlignWaves, kAlignLdsWhole, kAlignLdsMax, kAlignScratchMax);
    }
    return 0;
}
