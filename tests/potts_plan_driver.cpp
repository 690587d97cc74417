// TEST INFRASTRUCTURE ONLY: the launch geometry of the sequence-model kernels (pydca_amd/csrc/potts_plan.h, host code that
// energy.hip, pll.hip, sample.hip and boltzmann.hip run) as a stand-alone program.  tests/potts_audit_reference.py compiles it
// with the host compiler.
// potts_plan_driver q elem L [q elem L ...] prints one line of "key value" pairs per triple (elem: 4 | 8 bytes):
//   energies      TS nb ntiles tpg G eLds eBudget eSeqBlock eChunk
//   site kernel   QM CJ KPB CPT siteLds siteSeqBlock
//   sampler       sQM sCJ nch res chunkVals regVals sLds residentL
//   bmDCA         TB bmNb bmLds bmStatic
#include "potts_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 1) % 3 != 0) {
        std::fprintf(stderr, "usage: %s q elem L [q elem L ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; i += 3) {
        const int q = std::atoi(argv[i]), elem = std::atoi(argv[i + 1]), L = std::atoi(argv[i + 2]);
        if (q < 2 || q > 32 || (elem != 4 && elem != 8) || L < 1) {
            std::fprintf(stderr, "q in 2..32, elem 4 or 8, L >= 1; not '%s %s %s'\n", argv[i], argv[i + 1], argv[i + 2]);
            return 2;
        }
        const EnergyGeom e = energy_geometry(L, q, (size_t)elem);
        const SitePlan s = site_plan(q, (size_t)elem);
        const SampleGeom g = sample_geometry(L, q, (size_t)elem);
        const int tb = bm_tile(q);
        std::printf("q %d elem %d L %d TS %d nb %d ntiles %d tpg %d G %d eLds %zu eBudget %zu eSeqBlock %d eChunk %d "
                    "QM %d CJ %d KPB %d CPT %d siteLds %zu siteSeqBlock %d "
                    "sQM %d sCJ %d nch %d res %d chunkVals %d regVals %d sLds %zu residentL %d "
                    "TB %d bmNb %d bmLds %zu bmStatic %zu\n",
                    q, elem, L, e.TS, e.nb, e.ntiles, e.tpg, e.G, energy_lds(e.TS, q, (size_t)elem), kETileBudget, kESeqBlock, kEChunk,
                    s.QM, s.CJ, s.KPB, s.CPT, s.lds, kSiteSeqBlock,
                    g.QM, g.CJ, ceil_div(L, g.CJ), (int)g.res, g.CJ * q * q, kSThreads * sample_regs((size_t)elem), g.lds, kSResidentL,
                    tb, ceil_div(L, tb), bm_lds(tb, q), kBmStaticLds);
    }
    return 0;
}
