// TEST INFRASTRUCTURE ONLY: the geometry of the arDCA coupling gradient (pydca_amd/csrc/ar_plan.h, host code that
// ArEngine::evaluate runs) as a stand-alone program.  tests/ardca_eval_reference.py compiles it with the host compiler.
// ar_plan_driver q [q ...] prints one line per q: q, KC, the thread count, the LDS bytes, then the constants kGTile,
// kGBlockBudget and kGMaxThreads.
#include "ar_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s q [q ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        const int q = std::atoi(argv[i]);
        if (q < 1) {
            std::fprintf(stderr, "q must be a positive integer, not '%s'\n", argv[i]);
            return 2;
        }
        const ArGradPlan p = ar_grad_plan(q);
        std::printf("%d %d %d %zu %d %zu %d\n", q, p.KC, p.threads, p.lds, kGTile, kGBlockBudget, kGMaxThreads);
    }
    return 0;
}
