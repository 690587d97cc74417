// Stand-alone driver of pydca_amd/csrc/assignment.h for tests/test_interaction_host.py: reads problems from stdin
// ("nr nc" and nr * nc entries as hexadecimal doubles, until end of input) and prints for each
// "rc total" and the lines "col gap" of its rows (total and gaps as hexadecimal doubles).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pydca_amd/csrc/assignment.h"

int main()
{
    int nr, nc;
    while (scanf("%d %d", &nr, &nc) == 2) {
        const size_t cells = nr > 0 && nc > 0 ? (size_t)nr * nc : 0;
        std::vector<double> E(cells);
        char tok[64];
        for (size_t k = 0; k < cells; ++k) {
            if (scanf("%63s", tok) != 1) return 2;
            E[k] = strtod(tok, nullptr);
        }
        std::vector<int32_t> col(nr > 0 ? nr : 0);
        std::vector<double> gap(nr > 0 ? nr : 0);
        double total = 0.0;
        const int rc = assign_partners_host(E.data(), nr, nc, col.data(), &total, gap.data());
        printf("%d %a\n", rc, total);
        if (rc == 0)
            for (int r = 0; r < nr; ++r) printf("%d %a\n", (int)col[r], gap[r]);
    }
    return 0;
}
