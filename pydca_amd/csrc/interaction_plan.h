// Launch geometry of the inter-protein energies (interaction.hip): the staging chunks of the field pass (cross_fields_kernel),
// the work items of the pair pass (cross_energy_kernel) and the blocks of A-sequences of a call.  Host code only, no HIP
// header: a host compiler builds it, and tests/interaction_plan_driver.cpp prints it for tests/test_interaction_host.py,
// which holds the GPU test's case table to these numbers.
//
// The pair pass works on items.  An item is a run of consecutive A-rows (they may belong to several groups) and a window
// [k0, k0 + kXWindow) over each row's own list of B-partners; its pairs are numbered row by row, pair p belongs to thread
// p % kXThreads, slot p / kXThreads, and a thread keeps one running sum per slot in registers.  The item's phi rows sit in LDS a
// chunk of jc sites at a time, jc = cross_chunk_sites(rows, q, LB).
//   a group with more than kXWindow B-rows: items of up to kXDenseRows of its A-rows times one window each;
//   the other groups: their A-rows are packed in order into items of up to kXSparseRows rows and kXItemPairs pairs, so that
//     many small groups share one workgroup (a 5 x 5 species takes 25 of an item's 4096 pairs).
// None of this enters a value: E(m, n) is one sequential sum over j whatever the item, the chunk or the block.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

// ---- cross_fields_kernel<S, QM>
constexpr int kXThreads = 256;                       // both kernels: 4 waves
constexpr int kXFieldRegs = 8;                       // staged block elements per thread at most
constexpr int kXFieldMaxCJ = 16;                     // A-sites per staging chunk at most
constexpr size_t kXFieldChunkBudget = 16 * 1024;     // LDS per chunk buffer (two of them), blocks of q x QM doubles

inline int cross_qm(int q) { return q <= 8 ? 8 : q <= 24 ? 24 : 32; }        // qm_of (potts_plan.h)

// A-sites per staging chunk: within the buffer, within the registers that carry the next chunk, at most kXFieldMaxCJ
inline int cross_field_chunk(int q)
{
    const int byLds = (int)(kXFieldChunkBudget / ((size_t)q * cross_qm(q) * sizeof(double)));
    const int byRegs = kXThreads * kXFieldRegs / (q * q);
    return std::max(1, std::min(kXFieldMaxCJ, std::min(byLds, byRegs)));
}

// dynamic LDS of the field pass: two chunk buffers, then per staged block r(a), c(b) (q each) and m for the zero-sum shift
inline size_t cross_field_lds(int q)
{
    const int cj = cross_field_chunk(q);
    return 2 * (size_t)cj * q * cross_qm(q) * sizeof(double) + (size_t)cj * (2 * q + 1) * sizeof(double);
}

// ---- cross_energy_kernel
constexpr int kXSlots = 16;                          // running sums per thread
constexpr int kXItemPairs = kXThreads * kXSlots;     // pairs per item at most
constexpr int kXWindow = 256;                        // B-rows of one A-row per item at most
constexpr int kXDenseRows = kXItemPairs / kXWindow;  // A-rows per item of a group with more than kXWindow B-rows
constexpr int kXSparseRows = 32;                     // A-rows per item at most (small groups packed together)
constexpr size_t kXPhiLds = 64 * 1024;               // LDS for the item's phi chunk: two workgroups per CU (160 KiB)
static_assert(kXDenseRows <= kXSparseRows, "the item's row tables hold kXSparseRows rows");

// sites per phi chunk of an item of `rows` A-rows: all LB of them when they fit (the single-tile case)
inline int cross_chunk_sites(int rows, int q, int LB)
{
    const int fit = (int)(kXPhiLds / ((size_t)rows * q * sizeof(double)));
    return std::max(1, std::min(LB, fit));
}

struct CrossItem { int32_t a0, na, k0, pad; };       // rows a0 .. a0 + na - 1 of the block, window starting at k0

// the items of the A-rows [0, n) of a block; cnt[m]: B-rows of row m's group
inline std::vector<CrossItem> cross_items(const int32_t* cnt, int n)
{
    std::vector<CrossItem> items;
    int m = 0;
    while (m < n) {
        if (cnt[m] <= 0) { ++m; continue; }
        if (cnt[m] > kXWindow) {                     // rows of one large group: equal counts, consecutive
            int na = 1;
            while (na < kXDenseRows && m + na < n && cnt[m + na] == cnt[m]) ++na;
            for (int k0 = 0; k0 < cnt[m]; k0 += kXWindow) items.push_back({m, na, k0, 0});
            m += na;
            continue;
        }
        int na = 0, pairs = 0;
        while (m + na < n && na < kXSparseRows && cnt[m + na] <= kXWindow && pairs + std::max(cnt[m + na], 0) <= kXItemPairs) {
            pairs += std::max(cnt[m + na], 0);
            ++na;
        }
        items.push_back({m, na, 0, 0});
        m += na;
    }
    return items;
}

// ---- the blocks of A-rows of a call: phi (LB * q doubles per row) and the device output (cnt[m] doubles per row) of a block
// both stay within kXPassBudget; the environment variable DCA_CROSS_PASS (a positive row count) caps a block; a block has at
// least one row
constexpr size_t kXPassBudget = (size_t)1 << 30;

inline int cross_pass_cap()
{
    const char* v = getenv("DCA_CROSS_PASS");
    return v && atol(v) > 0 ? (int)std::min<long>(atol(v), 1 << 30) : 1 << 30;
}

// rows of the block that starts at row m0
inline int cross_pass_rows(const int32_t* cnt, int n, int m0, int LB, int q, int cap)
{
    const size_t perRow = (size_t)LB * q * sizeof(double);
    size_t phi = 0, out = 0;
    int rows = 0;
    while (m0 + rows < n && rows < cap) {
        const size_t o = (size_t)std::max(cnt[m0 + rows], 0) * sizeof(double);
        if (rows > 0 && (phi + perRow > kXPassBudget || out + o > kXPassBudget)) break;
        phi += perRow; out += o; ++rows;
    }
    return rows;
}
