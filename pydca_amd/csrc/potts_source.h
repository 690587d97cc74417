// The fitted Potts model as its consumers see it (energy.hip, pll.hip, sample.hip, sample_conditional.hip, ascent.hip,
// ais.hip, boltzmann.hip): one host-side description, PottsSource, and one typed device view, PottsView<S>, which alone knows the two
// parameter layouts.
//   kind 0: the packed plm vector x of element type `dtype` (DCA_F32 / DCA_F64): fields L*q first, then the upper-triangle
//           q x q blocks in pair order (pair_index); mfh and ld unused;
//   kind 1: the dense mf couplings -inv(C) (double, leading dimension ld, (q-1) x (q-1) blocks) with the mf fields mfh
//           (device, L*(q-1) doubles); both zero on the gap state q-1.
// Included from dca_internal.h.
#pragma once

struct dca_ctx;

struct PottsSource {
    const void* src;          // device
    int kind, dtype;
    const double* mfh;        // device, kind 1 only
    int L, q, ld;
};

__host__ __device__ __forceinline__ size_t pair_index(int L, int i, int j)
{
    return (size_t)L * (L - 1) / 2 - (size_t)(L - i) * (L - i - 1) / 2 + (size_t)(j - i - 1);
}

// floor(e / d) for e * d < 2^32: m = floor(2^32 / d) + 1
__device__ __forceinline__ int fast_div(int e, uint32_t m) { return (int)__umulhi((uint32_t)e, m); }

// The two layouts.  Free functions for the kernels that keep the view's members as __restrict__ scalar parameters
// (energy_pairs_kernel, gibbs_sweep_kernel: at their register limit the allocator's result moved when they read a struct)
// and for the row staging of the other lane = chain kernels (potts_rows.h).
template <typename S>
__device__ __forceinline__ double potts_field(const S* src, const double* mfh, int kind, int q, int i, int a)
{
    if (kind == 0) return (double)src[(size_t)i * q + a];
    return a == q - 1 ? 0.0 : mfh[(size_t)i * (q - 1) + a];
}

// J_ij(a, b) for i < j, widened to double
template <typename S>
__device__ __forceinline__ double potts_coupling(const S* src, int kind, int L, int q, int ld, int i, int j, int a, int b)
{
    if (kind == 0) return (double)src[(size_t)L * q + pair_index(L, i, j) * (size_t)q * q + (size_t)a * q + b];
    const int qm = q - 1;
    if (a == qm || b == qm) return 0.0;
    return (double)src[(size_t)(i * qm + a) * ld + (size_t)j * qm + b];
}

template <typename S>
struct PottsView {
    const S* src;
    const double* mfh;
    int kind, L, q, ld;
    explicit PottsView(const PottsSource& ps) : src(static_cast<const S*>(ps.src)), mfh(ps.mfh), kind(ps.kind), L(ps.L), q(ps.q), ld(ps.ld) {}
    __device__ __forceinline__ double field(int i, int a) const { return potts_field(src, mfh, kind, q, i, a); }
    __device__ __forceinline__ double coupling(int i, int j, int a, int b) const { return potts_coupling(src, kind, L, q, ld, i, j, a, b); }
};

// f(PottsView<float>) or f(PottsView<double>), by ps.dtype
template <typename F>
auto with_source_type(const PottsSource& ps, F&& f)
{
    if (ps.dtype == DCA_F32) return f(PottsView<float>(ps));
    return f(PottsView<double>(ps));
}

// sample.hip: rows (n x L device bytes; row stride ld going in, L coming out) <-> site-major codes st[s * nS + c] (zero past n),
// on ctx->stream
hipError_t dca_rows_to_sites(dca_ctx* ctx, const uint8_t* dRows, size_t ld, int n, int L, int nS, uint8_t* dSites);
hipError_t dca_sites_to_rows(dca_ctx* ctx, const uint8_t* dSites, int n, int L, int nS, uint8_t* dRows);

// energy.hip: DCA_ERR_ARG with "<what>code %d >= q at element %zu" for the first host code >= q
int dca_check_codes(const uint8_t* codes, size_t count, int q, const char* what);
