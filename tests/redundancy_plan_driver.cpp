// TEST INFRASTRUCTURE ONLY: the launch plan of the redundancy filter and the identity clusters (pydca_amd/csrc/redundancy_plan.h,
// host code that redundancy.hip runs) as a stand-alone program.  tests/test_redundancy_host.py compiles it with the host compiler.
// redundancy_plan_driver n q envBlock bitsCap [...] prints one line of "key value" pairs per group of four
// (envBlock <= 0: DCA_FILTER_BLOCK unset; bitsCap < 0: DCA_CLUSTER_BITS_MAX unset):
//   B blocks W tilePairs ldsResolve filterBits ldsTile tiles clusterW bitsBytes allocDwords stored units walkBlocks blockDefault blockMax capDefault
#include "redundancy_plan.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc < 5 || (argc - 1) % 4 != 0) {
        std::fprintf(stderr, "usage: %s n q envBlock bitsCap [...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; i += 4) {
        const int n = std::atoi(argv[i]), q = std::atoi(argv[i + 1]);
        const long envBlock = std::atol(argv[i + 2]);
        const long long cap = std::atoll(argv[i + 3]);
        if (n < 1 || q < 2 || q > 32) {
            std::fprintf(stderr, "n >= 1, q in 2..32\n");
            return 2;
        }
        const FilterPlan f = filter_plan(n, envBlock);
        const ClusterPlan c = cluster_plan(n, cap < 0 ? kClusterBitsMaxDefault : (unsigned long long)cap);
        std::printf("n %d q %d B %d blocks %d W %d tilePairs %lld ldsResolve %zu filterBits %zu ldsTile %zu tiles %d clusterW %d bitsBytes %llu "
                    "allocDwords %llu stored %d units %llu walkBlocks %llu blockDefault %d blockMax %d capDefault %llu\n",
                    n, q, f.B, f.blocks, f.W, f.tilePairs, f.ldsResolve, f.bitsBytes, red_tile_lds(q), c.tiles, c.W, c.bitsBytes, c.allocDwords,
                    (int)c.stored, c.units, red_walk_blocks(c.tiles, c.tiles), kFilterBlockDefault, kFilterBlockMax, kClusterBitsMaxDefault);
    }
    return 0;
}
