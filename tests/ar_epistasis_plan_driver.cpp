// TEST INFRASTRUCTURE ONLY: the geometry of the arDCA epistasis product kernel (pydca_amd/csrc/ar_epistasis_plan.h, host code
// that ar_epistasis.hip launches by) as a stand-alone program.  tests/ar_epistasis_reference.py compiles it with the host compiler.
// ar_epistasis_plan_driver L q prints
//   L q QM NPRE ldsBytes kEpiThreads kEpiRows kEpiCols kEpiTileR kEpiTileC kEpiRescale ntiles
// and then one line per tile in launch order:
//   rowTile columnTile mstart steps midSite liveRows liveColumns
// midSite: the tile's first column is not state 0 of its site (C0 % q != 0); live: rows / columns below L q.
#include "ar_epistasis_plan.h"
#include "potts_plan.h"      // qm_of

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s L q\n", argv[0]);
        return 2;
    }
    const int L = std::atoi(argv[1]), q = std::atoi(argv[2]);
    if (L < 2 || q < 1 || q > 32) {
        std::fprintf(stderr, "need L >= 2 and 1 <= q <= 32, not '%s' '%s'\n", argv[1], argv[2]);
        return 2;
    }
    const int QM = qm_of(q), Lq = L * q;
    const std::vector<EpiTile> tiles = epistasis_tiles(L, q);
    std::printf("%d %d %d %d %zu %d %d %d %d %d %d %zu\n", L, q, QM, epi_npre(QM), epi_lds_bytes(q), kEpiThreads, kEpiRows, kEpiCols,
                kEpiTileR, kEpiTileC, kEpiRescale, tiles.size());
    for (const EpiTile& t : tiles) {
        const int R0 = t.x * kEpiTileR, C0 = t.y * kEpiTileC;
        std::printf("%d %d %d %d %d %d %d\n", t.x, t.y, epi_mstart(t.y, q), epi_steps(t.y, L, q), C0 % q != 0 ? 1 : 0,
                    std::min(kEpiTileR, Lq - R0), std::min(kEpiTileC, Lq - C0));
    }
    return 0;
}
