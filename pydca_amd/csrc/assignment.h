// Maximum-weight assignment with gaps (dca_assign_partners).  Host code only, no HIP header: capi.cpp includes it and
// tests/assignment_driver.cpp compiles it alone.
//
// The matching: size min(nr, nc), maximum total of E, by shortest augmenting paths on the costs -E with row and column
// potentials (Hungarian / Jonker-Volgenant, O(n^2 m) for n = min(nr, nc), m = max(nr, nc)); with nr > nc the transposed
// problem is solved, so every row of the problem solved is matched.  Under exact ties any optimal matching may come back;
// the total and the gaps do not depend on which.
//
// The gaps, one augmentation per forbidden pair from the optimal potentials (u, v), v <= 0 and 0 on free columns, reduced
// costs c'(i, j) = c(i, j) - u(i) - v(j) >= 0 and 0 on the matching M.  With m - n dummy rows of cost 0 (potential 0; they
// hold the free columns) M is a perfect matching, and a best perfect matching that avoids (r, c) differs from it by one
// alternating cycle through (r, c): gap = the distance in reduced costs from row r to column c with the pair forbidden.
// One dense Dijkstra over the columns per assigned row, O(m^2) each, O(n m^2) in all; the dummy rows are alike, so they
// are entered once, from the nearest free column, and reach column j at -v(j).  +inf when column c cannot be reached (a
// 1 x 1 block).  The gap itself is total - (the total of the matching that cycle gives), both summed over the rows in ascending
// order: it does not carry the rounding of the potentials, and two pairs of a block whose best alternative is the same matching
// (two rows that would swap partners) get the same bits.
//
// Deterministic (ties in the searches go to the smallest index), no threads, no device.  Returns 0, or -1 (the caller's
// DCA_ERR_ARG) for a negative size, a NULL array that is needed or a non-finite entry.
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

inline int assign_partners_host(const double* E, int nr, int nc, int32_t* col_of_row, double* total_out, double* gap_out)
{
    if (nr < 0 || nc < 0) return -1;
    if (total_out) *total_out = 0.0;
    if (nr > 0 && !col_of_row) return -1;
    for (int r = 0; r < nr; ++r) {
        col_of_row[r] = -1;
        if (gap_out) gap_out[r] = 0.0;
    }
    if (nr == 0 || nc == 0) return 0;
    if (!E) return -1;
    for (size_t k = 0; k < (size_t)nr * nc; ++k)
        if (!std::isfinite(E[k])) return -1;

    const bool tr = nr > nc;                         // solve with n <= m
    const int n = tr ? nc : nr, m = tr ? nr : nc;
    auto cost = [&](int i, int j) { return tr ? -E[(size_t)j * nc + i] : -E[(size_t)i * nc + j]; };
    const double inf = std::numeric_limits<double>::infinity();

    // rows and columns 1-based, 0 the sentinel; p[j]: the row matched to column j
    std::vector<double> u((size_t)n + 1, 0.0), v((size_t)m + 1, 0.0), minv((size_t)m + 1);
    std::vector<int> p((size_t)m + 1, 0), way((size_t)m + 1, 0);
    std::vector<char> used((size_t)m + 1);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        std::fill(minv.begin(), minv.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = inf;
            int j1 = 0;
            for (int j = 1; j <= m; ++j) {
                if (used[j]) continue;
                const double cur = cost(i0 - 1, j - 1) - u[i0] - v[j];
                if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
                if (minv[j] < delta) { delta = minv[j]; j1 = j; }
            }
            for (int j = 0; j <= m; ++j) {
                if (used[j]) { u[p[j]] += delta; v[j] -= delta; }
                else minv[j] -= delta;
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }

    std::vector<int> colOf((size_t)n + 1, 0);
    for (int j = 1; j <= m; ++j)
        if (p[j]) colOf[p[j]] = j;
    if (tr) { for (int j = 1; j <= m; ++j) if (p[j]) col_of_row[j - 1] = p[j] - 1; }
    else for (int i = 1; i <= n; ++i) col_of_row[i - 1] = colOf[i] - 1;
    double total = 0.0;                              // over the original rows in ascending order, from 0.0
    for (int r = 0; r < nr; ++r)
        if (col_of_row[r] >= 0) total += E[(size_t)r * nc + col_of_row[r]];
    if (total_out) *total_out = total;
    if (!gap_out) return 0;

    // the total of a matching given as the solver's colOf, summed over the ORIGINAL rows in ascending order from 0.0 (as `total`
    // above): two forbidden pairs with the same best alternative get the same bits
    auto total_of = [&](const std::vector<int>& cOf) {
        double t = 0.0;
        if (!tr) { for (int i = 1; i <= n; ++i) t += E[(size_t)(i - 1) * nc + (cOf[i] - 1)]; return t; }
        std::vector<int> rowOfCol((size_t)m + 1, 0);                 // original row (solver column) -> its solver row
        for (int i = 1; i <= n; ++i) rowOfCol[cOf[i]] = i;
        for (int j = 1; j <= m; ++j) if (rowOfCol[j]) t += E[(size_t)(j - 1) * nc + (rowOfCol[j] - 1)];
        return t;
    };
    std::vector<double> d((size_t)m + 1);
    std::vector<int> prev((size_t)m + 1), cNew;
    const int kDummy = -1;
    for (int r = 1; r <= n; ++r) {
        const int c = colOf[r];
        std::fill(d.begin(), d.end(), inf);
        std::fill(used.begin(), used.end(), 0);
        // d(j) <- min(d(j), base + c'(i0, j)) over the open columns; the forbidden pair is never relaxed
        auto relax = [&](int i0, double base) {
            for (int j = 1; j <= m; ++j) {
                if (used[j] || (i0 == r && j == c)) continue;
                double w = cost(i0 - 1, j - 1) - u[i0] - v[j];
                if (w < 0.0) w = 0.0;                // rounding of the potentials
                if (base + w < d[j]) { d[j] = base + w; prev[j] = i0; }
            }
        };
        bool found = false;
        int jfree = 0;                               // the free column through which the dummy rows were entered
        relax(r, 0.0);
        for (;;) {
            int j1 = 0;
            double dj = inf;
            for (int j = 1; j <= m; ++j)
                if (!used[j] && d[j] < dj) { dj = d[j]; j1 = j; }
            if (j1 == 0) break;
            used[j1] = 1;
            if (j1 == c) { found = true; break; }
            if (p[j1] != 0) { relax(p[j1], dj); continue; }
            if (jfree) continue;                     // a later free column is no nearer to the dummy rows
            jfree = j1;
            for (int j = 1; j <= m; ++j)
                if (!used[j] && dj - v[j] < d[j]) { d[j] = dj - v[j]; prev[j] = kDummy; }
        }
        double best = inf;
        if (found) {                                 // the alternative matching, walked back from column c to row r
            cNew = colOf;
            for (int col = c;;) {
                const int i = prev[col];
                if (i == kDummy) { col = jfree; continue; }      // `col` goes free, the dummy row gives up jfree
                const int old = colOf[i];
                cNew[i] = col;
                if (i == r) break;
                col = old;
            }
            best = total - total_of(cNew);
        }
        if (best < 0.0) best = 0.0;
        gap_out[tr ? c - 1 : r - 1] = best;          // the original row of the pair
    }
    return 0;
}
