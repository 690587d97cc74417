// TEST INFRASTRUCTURE ONLY: the product's line search (pydca_amd/csrc/more_thuente.h) behind the call shape of the oracle's
// oracle_mt_search_f64, with the oracle's constants (oracle/plm_oracle.c: plmDCA's).  tests/test_more_thuente_host.py
// compiles it with the host compiler.  deferred != 0: g.s of the starting point is handed over the way plmDCA's engine
// does it, with the first evaluation.
#include <cstddef>

#include "more_thuente.h"

typedef double (*eval_fn)(void* ctx, const double* x, double* g, size_t n);

extern "C" int mt_search_driver(size_t n, double* x, double* f, double* g, const double* s, double* stp, const double* xp,
                                eval_fn eval, void* ctx, int* nevals, int deferred)
{
    const MtParams params{1e-4, 0.9, 1.0e-16, 1e-20, 1e20, 5};
    auto gs = [&] { double v = 0.0; for (size_t i = 0; i < n; ++i) v += g[i] * s[i]; return v; };
    const double slope = gs();
    double dginit = deferred ? 0.0 : slope;
    int rc = 0;
    return mt_line_search(params, stp, f, &dginit, deferred != 0, [&](double t, double* ft, double* dgt) {
        dginit = slope;
        for (size_t i = 0; i < n; ++i) { x[i] = xp[i]; x[i] += t * s[i]; }
        *ft = eval(ctx, x, g, n);
        ++*nevals;
        *dgt = gs();
        return 0;
    }, &rc);
}
