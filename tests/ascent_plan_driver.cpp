// TEST INFRASTRUCTURE ONLY: the launch plan of the greedy ascent (pydca_amd/csrc/ascent_plan.h, host code that ascent.hip runs)
// as a stand-alone program.  tests/test_ascent_host.py compiles it with the host compiler.
// ascent_plan_driver q elem F ldsCap maxSteps paths n envPass [...] prints one line of "key value" pairs per group of eight
// (elem: 4 | 8 bytes; ldsCap < 0: DCA_ASCENT_LDS unset; paths 0 | 1; envPass <= 0: DCA_ASCENT_PASS unset):
//   QM CJ chunkVals regVals ldsInit tableBytes sideBytes inLds ldsAscent perChain pass ldsTotal budget
#include "ascent_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 9 || (argc - 1) % 8 != 0) {
        std::fprintf(stderr, "usage: %s q elem F ldsCap maxSteps paths n envPass [...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; i += 8) {
        const int q = std::atoi(argv[i]), elem = std::atoi(argv[i + 1]), F = std::atoi(argv[i + 2]);
        const long cap = std::atol(argv[i + 3]);
        const int maxSteps = std::atoi(argv[i + 4]), paths = std::atoi(argv[i + 5]), n = std::atoi(argv[i + 6]);
        const long envPass = std::atol(argv[i + 7]);
        if (q < 2 || q > 32 || (elem != 4 && elem != 8) || F < 1 || maxSteps < 0 || n < 0) {
            std::fprintf(stderr, "q in 2..32, elem 4 or 8, F >= 1, maxSteps >= 0, n >= 0\n");
            return 2;
        }
        const size_t ldsCap = cap < 0 ? kAscLdsTotal : std::min((size_t)cap, kAscLdsTotal);
        const AscentPlan p = ascent_plan(F, q, (size_t)elem, ldsCap, paths != 0, maxSteps);
        std::printf("q %d elem %d F %d QM %d CJ %d chunkVals %d regVals %d ldsInit %zu tableBytes %zu sideBytes %zu inLds %d ldsAscent %zu "
                    "perChain %zu pass %d ldsTotal %zu budget %zu\n",
                    q, elem, F, p.QM, p.CJ, p.CJ * q * q, kAscInitChains * asc_init_regs((size_t)elem), p.ldsInit, p.tableBytes, p.sideBytes,
                    (int)p.tableInLds, p.ldsAscent, p.perChain, ascent_pass_chains(n, p.perChain, envPass), kAscLdsTotal, kAscScratchBudget);
    }
    return 0;
}
