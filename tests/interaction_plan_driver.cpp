// Prints the launch geometry of pydca_amd/csrc/interaction_plan.h as one JSON object, for tests/test_interaction_host.py and
// tests/test_interaction_energies.py.  Usage: interaction_plan_driver q LB [cnt ...]: cnt = the B-row count of each A-row of a
// block (the items of that block are listed, and its split into blocks under the current DCA_CROSS_PASS).
#include <cstdio>
#include <cstdlib>

#include "../pydca_amd/csrc/interaction_plan.h"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const int q = atoi(argv[1]), LB = atoi(argv[2]);
    std::vector<int32_t> cnt;
    for (int k = 3; k < argc; ++k) cnt.push_back(atoi(argv[k]));
    printf("{\"threads\": %d, \"qm\": %d, \"field_chunk\": %d, \"field_regs\": %d, \"field_lds\": %zu, \"slots\": %d, \"item_pairs\": %d, "
           "\"window\": %d, \"dense_rows\": %d, \"sparse_rows\": %d, \"phi_lds\": %zu, \"pass_budget\": %zu, ",
           kXThreads, cross_qm(q), cross_field_chunk(q), kXFieldRegs, cross_field_lds(q), kXSlots, kXItemPairs, kXWindow, kXDenseRows,
           kXSparseRows, kXPhiLds, kXPassBudget);
    // the largest LB an item of `rows` rows holds in one chunk
    printf("\"single_tile_dense\": %d, \"single_tile_sparse\": %d, \"chunk_dense\": %d, \"chunk_sparse\": %d, ",
           cross_chunk_sites(kXDenseRows, q, 1 << 30), cross_chunk_sites(kXSparseRows, q, 1 << 30), cross_chunk_sites(kXDenseRows, q, LB),
           cross_chunk_sites(kXSparseRows, q, LB));
    printf("\"items\": [");
    const std::vector<CrossItem> items = cross_items(cnt.data(), (int)cnt.size());
    for (size_t k = 0; k < items.size(); ++k)
        printf("%s[%d, %d, %d, %d]", k ? ", " : "", items[k].a0, items[k].na, items[k].k0, cross_chunk_sites(items[k].na, q, LB));
    printf("], \"blocks\": [");
    const int cap = cross_pass_cap();
    for (int m0 = 0, first = 1; m0 < (int)cnt.size(); first = 0) {
        const int rows = cross_pass_rows(cnt.data(), (int)cnt.size(), m0, LB, q, cap);
        printf("%s%d", first ? "" : ", ", rows);
        m0 += rows;
    }
    printf("]}\n");
    return 0;
}
