// Principal components of the reweighted one-hot alignment and projections of sequence sets (dca_pca_fit, dca_pca_project;
// DESIGN.md section 21).  With X the N x L q one-hot alignment, f the weighted site frequencies and w the context's weights,
//   C V = (X - 1 f^T)^T diag(w) (X - 1 f^T) V / Meff
// is two passes over the code bytes, so the L q x L q matrix is never formed:
//   pca_project_kernel   P[n][m] = sum_i V[(i q + s_ni)][m] - c_m, one double chain over the sites in ascending order and one
//                        subtraction (lane = sequence, a tile of V rows in LDS, kProjCols columns in registers); with weights
//                        it writes w_n P[n][m].  It is the whole of dca_pca_project.
//   pca_back_kernel      lanes own (state, column) pairs of kBackSites sites; a workgroup walks its slab of DCA_PCA_SLAB
//                        sequences in ascending order with a predicated add; pca_back_reduce_kernel adds the slabs ascending,
//                        divides by Meff and subtracts f(i,a) t_m, t_m = sum_n w_n P[n][m] / Meff (pca_colsum_kernel, same slabs).
//   pca_gram_kernel      b x b products of two L q x b blocks: chunks of kGramRows rows, each summed in ascending row order,
//                        the chunks added ascending by pca_sum_kernel.
//   pca_rotate_kernel    V <- A T1 (+ B T2), ascending over the inner index.
// No floating atomics anywhere: the order of every sum is fixed by (N, L, q, b).
// The fit is block subspace iteration with Rayleigh-Ritz on b = min(L q, k + 8) vectors; the b x b eigenproblems and the rules
// of the contract are host code (pca_host.h).
#include "dca_internal.h"
#include "pca_host.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int kSlab = DCA_PCA_SLAB;      // sequences per slab of the back-projection
constexpr int kThreads = 256;
constexpr int kProjCols = 10;            // columns of V one lane of pca_project_kernel accumulates in registers
constexpr int kProjLds = 6144;           // doubles of LDS per V tile (48 KiB): q = 21, 10 columns -> 29 sites
constexpr int kBackSites = 8;            // sites per workgroup of pca_back_kernel: one aligned 8-byte load of codes per sequence
constexpr int kGramRows = 128;           // rows per chunk of pca_gram_kernel
constexpr int kGramTile = 16;            // rows staged in LDS at a time
constexpr uint32_t kPcaTag = 4;          // Philox tag of the start block (0..3 belong to the samplers)

static_assert(kBackSites == 8, "pca_back_kernel reads the codes of its sites as one uint64");

// XT[i * Ns + s] = X[s * Ls + i]; grid (ceil(n / 64), ceil(L / 64)), 256 threads: 64 sequences x 4 groups of 16 sites
__global__ __launch_bounds__(kThreads)
void pca_transpose_kernel(const uint8_t* __restrict__ X, int Ls, int n, int L, int Ns, uint8_t* __restrict__ XT)
{
    const int s = blockIdx.x * 64 + (threadIdx.x & 63), ig = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
    if (s >= n) return;
    for (int u = 0; u < 16; ++u) {
        const int i = ig + u;
        if (i < L) XT[(size_t)i * Ns + s] = X[(size_t)s * Ls + i];
    }
}

// the start block: element (r, m) is a function of (seed, r, m) alone
__global__ __launch_bounds__(kThreads)
void pca_init_kernel(double* __restrict__ V, int rows, int b, uint64_t seed)
{
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (size_t)rows * b) return;
    const int r = (int)(e / b), m = (int)(e - (size_t)r * b);
    V[e] = 2.0 * philox_uniform(seed, (uint64_t)r, (uint64_t)m, 0, kPcaTag) - 1.0;
}

// grid (ceil(n / 256), ceil(ncols / kProjCols)); dynamic LDS ts * q * kProjCols doubles.  V: rows x ldv, columns m0.. of it.
// out[s * ldo + m] = (W ? W[s] : 1) * (sum_i V[(i q + XT[i][s])][m] - c[m])
__global__ __launch_bounds__(kThreads)
void pca_project_kernel(const uint8_t* __restrict__ XT, int Ns, int n, int L, int q, const double* __restrict__ V, int ldv, int ncols,
                        const double* __restrict__ c, const double* __restrict__ W, double* __restrict__ out, int ldo, int ts)
{
    extern __shared__ double tile[];
    const int t = threadIdx.x, s = blockIdx.x * kThreads + t, m0 = blockIdx.y * kProjCols;
    const int g = min(kProjCols, ncols - m0);
    double acc[kProjCols];
#pragma unroll
    for (int mm = 0; mm < kProjCols; ++mm) acc[mm] = 0.0;
    for (int i0 = 0; i0 < L; i0 += ts) {
        const int nt = min(ts, L - i0), cells = nt * q * kProjCols;
        __syncthreads();                                   // the previous tile has been read
        for (int e = t; e < cells; e += kThreads) {
            const int row = e / kProjCols, mm = e - row * kProjCols;
            tile[e] = mm < g ? V[((size_t)i0 * q + row) * ldv + m0 + mm] : 0.0;
        }
        __syncthreads();
        if (s < n) {
            for (int u = 0; u < nt; ++u) {
                const int code = XT[(size_t)(i0 + u) * Ns + s];
                const double* tr = tile + (u * q + code) * kProjCols;
#pragma unroll
                for (int mm = 0; mm < kProjCols; ++mm) acc[mm] += tr[mm];
            }
        }
    }
    if (s >= n) return;
    const double w = W ? W[s] : 1.0;
#pragma unroll
    for (int mm = 0; mm < kProjCols; ++mm) {
        if (mm >= g) continue;
        const double p = acc[mm] - c[m0 + mm];
        out[(size_t)s * ldo + m0 + mm] = W ? w * p : p;
    }
}

// Tpart[slab * b + m] = sum of WP[n][m] over the slab's sequences, ascending; grid (slabs), 128 threads
__global__ __launch_bounds__(128)
void pca_colsum_kernel(const double* __restrict__ WP, int N, int b, double* __restrict__ Tpart)
{
    const int m = threadIdx.x, slab = blockIdx.x;
    if (m >= b) return;
    const int n0 = slab * kSlab, n1 = min(N, n0 + kSlab);
    double acc = 0.0;
    for (int n = n0; n < n1; ++n) acc += WP[(size_t)n * b + m];
    Tpart[(size_t)slab * b + m] = acc;
}

// grid (ceil(L / 8), slabs, ceil(q b / 256)); thread = pair p = a * b + m of the sites i0 .. i0 + 7.
// Ypart[(slab * L + i) * q b + p] = sum over the slab's sequences with s_ni == a of WP[n][m], ascending n
__global__ __launch_bounds__(kThreads)
void pca_back_kernel(const uint8_t* __restrict__ X, int Ls, int N, int L, int q, int b, const double* __restrict__ WP,
                     double* __restrict__ Ypart)
{
    const int i0 = blockIdx.x * kBackSites, slab = blockIdx.y, qb = q * b;
    const int p = blockIdx.z * kThreads + threadIdx.x;
    if (p >= qb) return;
    const int a = p / b, m = p - a * b;
    const int n0 = slab * kSlab, n1 = min(N, n0 + kSlab);
    double acc[kBackSites];
#pragma unroll
    for (int u = 0; u < kBackSites; ++u) acc[u] = 0.0;
#pragma unroll 4
    for (int n = n0; n < n1; ++n) {
        // i0 is a multiple of 8 below L <= Ls and Ls a multiple of 128: inside the zero-padded row, aligned
        const uint64_t cw = *reinterpret_cast<const uint64_t*>(X + (size_t)n * Ls + i0);
        const double wp = WP[(size_t)n * b + m];
#pragma unroll
        for (int u = 0; u < kBackSites; ++u) acc[u] += (int)((cw >> (8 * u)) & 0xffu) == a ? wp : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kBackSites; ++u)
        if (i0 + u < L) Ypart[((size_t)slab * L + i0 + u) * qb + p] = acc[u];
}

// Y[e] = (sum of the slabs, ascending) / meff - F[row] * (sum of Tpart's slabs, ascending) / meff; F == NULL: no second term
__global__ __launch_bounds__(kThreads)
void pca_back_reduce_kernel(const double* __restrict__ Ypart, int slabs, size_t cells, int b, const double* __restrict__ Tpart,
                            const double* __restrict__ F, double meff, double* __restrict__ Y)
{
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= cells) return;
    double acc = 0.0;
    for (int s = 0; s < slabs; ++s) acc += Ypart[(size_t)s * cells + e];
    double y = acc / meff;
    if (F) {
        const size_t r = e / b;
        const int m = (int)(e - r * b);
        double t = 0.0;
        for (int s = 0; s < slabs; ++s) t += Tpart[(size_t)s * b + m];
        y = y - F[r] * (t / meff);
    }
    Y[e] = y;
}

// part[chunk * pairs + p] = sum over the chunk's rows, ascending, of A[r][pa] * B[r][pb]; p = pa * bb + pb, or with diag
// (ba == bb) p = pa = pb.  grid (chunks, ceil(pairs / 256))
__global__ __launch_bounds__(kThreads)
void pca_gram_kernel(const double* __restrict__ A, int ba, const double* __restrict__ B, int bb, int rows, int diag,
                     double* __restrict__ part)
{
    __shared__ double tA[kGramTile * kPcaMaxBlock], tB[kGramTile * kPcaMaxBlock];
    const int t = threadIdx.x, chunk = blockIdx.x, pairs = diag ? ba : ba * bb;
    const int p = blockIdx.y * kThreads + t;
    const int pa = diag ? p : p / bb, pb = diag ? p : p - pa * bb;
    const int r0 = chunk * kGramRows, r1 = min(rows, r0 + kGramRows);
    double acc = 0.0;
    for (int t0 = r0; t0 < r1; t0 += kGramTile) {
        const int nt = min(kGramTile, r1 - t0);
        __syncthreads();
        for (int e = t; e < nt * ba; e += kThreads) tA[e] = A[(size_t)t0 * ba + e];
        for (int e = t; e < nt * bb; e += kThreads) tB[e] = B[(size_t)t0 * bb + e];
        __syncthreads();
        if (p < pairs)
            for (int r = 0; r < nt; ++r) acc += tA[r * ba + pa] * tB[r * bb + pb];
    }
    if (p < pairs) part[(size_t)chunk * pairs + p] = acc;
}

__global__ __launch_bounds__(kThreads)
void pca_sum_kernel(const double* __restrict__ part, int chunks, int len, double* __restrict__ out)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * len + e];
    out[e] = acc;
}

// out[r][m] = sum_j A[r][j] T1[j][m] (ascending j), then + sum_j B[r][j] T2[j][m] when B is given.  out is neither A nor B.
__global__ __launch_bounds__(kThreads)
void pca_rotate_kernel(const double* __restrict__ A, const double* __restrict__ T1, const double* __restrict__ B,
                       const double* __restrict__ T2, int rows, int b, double* __restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (size_t)rows * b) return;
    const size_t r = e / b;
    const int m = (int)(e - r * b);
    double acc = 0.0;
    for (int j = 0; j < b; ++j) acc += A[r * b + j] * T1[(size_t)j * b + m];
    if (B) {
        double acc2 = 0.0;
        for (int j = 0; j < b; ++j) acc2 += B[r * b + j] * T2[(size_t)j * b + m];
        acc += acc2;
    }
    out[e] = acc;
}

#define PCA_ALLOC(buf, count) HIP_TRY_AS_NOMEM((buf).alloc(std::max<size_t>(count, 1), false), who)

int proj_tile_sites(int L, int q) { return std::max(1, std::min(L, kProjLds / (q * kProjCols))); }

// rows (n x L codes at stride Ls on the device) -> XT (L x Ns)
int transpose_rows(dca_ctx* ctx, const char* who, const uint8_t* dRows, int Ls, int n, int L, int Ns, uint8_t* dXT)
{
    hipLaunchKernelGGL(pca_transpose_kernel, dim3(ceil_div(n, 64), ceil_div(L, 64)), dim3(kThreads), 0, ctx->stream, dRows, Ls, n, L,
                       Ns, dXT);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}

int launch_project(dca_ctx* ctx, const char* who, const uint8_t* dXT, int Ns, int n, int L, int q, const double* dV, int ldv, int ncols,
                   const double* dC, const double* dW, double* dOut, int ldo)
{
    const int ts = proj_tile_sites(L, q);
    ScopedKernelClock kc(ctx, "pca_project");
    hipLaunchKernelGGL(pca_project_kernel, dim3(ceil_div(n, kThreads), ceil_div(ncols, kProjCols)), dim3(kThreads),
                       (size_t)ts * q * kProjCols * sizeof(double), ctx->stream, dXT, Ns, n, L, q, dV, ldv, ncols, dC, dW, dOut, ldo, ts);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}

// host -> device on the context's stream; returns once the host buffer may change
int upload(dca_ctx* ctx, const char* who, void* dst, const void* src, size_t bytes)
{
    HIP_TRY_AS(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}
int download(dca_ctx* ctx, const char* who, void* dst, const void* src, size_t bytes)
{
    HIP_TRY_AS(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream), who);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    return DCA_OK;
}

struct PcaFit {
    dca_ctx* ctx;
    const char* who;
    int N, L, q, Ls, rows, b, slabs, chunks, Ns;
    double meff;
    DevBuf<uint8_t> dXT;
    DevBuf<double> dF, dV, dY, dR, dWP, dYpart, dTpart, dGpart, dSmall, dT1, dT2, dC;

    // Y = C Z for a block of nb columns; with dFreq == NULL it is the plain weighted histogram of WP / meff (the frequencies)
    int back(const double* dWPin, int nb, const double* dFreq, double* dOut)
    {
        ScopedKernelClock kc(ctx, "pca_back");
        if (dFreq) hipLaunchKernelGGL(pca_colsum_kernel, dim3(slabs), dim3(128), 0, ctx->stream, dWPin, N, nb, dTpart.get());
        hipLaunchKernelGGL(pca_back_kernel, dim3(ceil_div(L, kBackSites), slabs, ceil_div(q * nb, kThreads)), dim3(kThreads), 0,
                           ctx->stream, ctx->dX, Ls, N, L, q, nb, dWPin, dYpart.get());
        const size_t cells = (size_t)rows * nb;
        hipLaunchKernelGGL(pca_back_reduce_kernel, dim3((unsigned)((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                           dYpart.get(), slabs, cells, nb, dTpart.get(), dFreq, meff, dOut);
        HIP_TRY_AS(hipGetLastError(), who);
        return DCA_OK;
    }
    // dOut (ba x bb, or ba with diag) = A^T B on the device; the launches are dca_pca_small_gram / _rotate below
    int gram(const double* dA, int ba, const double* dB, int bb, bool diag, double* dOut)
    {
        return dca_pca_small_gram(ctx, who, dA, ba, dB, bb, rows, diag, dGpart.get(), dOut);
    }
    int rotate(const double* dA, const double* dTa, const double* dB, const double* dTb, double* dOut)
    {
        return dca_pca_small_rotate(ctx, who, dA, dTa, dB, dTb, rows, b, dOut);
    }
    // dV <- orthonormalised dV, through the Gram matrix, twice; dR is the scratch block
    int orthonormalise(std::vector<double>& G, std::vector<double>& T)
    {
        for (int pass = 0; pass < 2; ++pass) {
            DCA_TRY(gram(dV, b, dV, b, false, dSmall));
            DCA_TRY(download(ctx, who, G.data(), dSmall, (size_t)b * b * sizeof(double)));
            pca_orth_transform(b, G.data(), T.data());
            DCA_TRY(upload(ctx, who, dT1, T.data(), (size_t)b * b * sizeof(double)));
            DCA_TRY(rotate(dV, dT1, nullptr, nullptr, dR));
            dV.swap(dR);
        }
        return DCA_OK;
    }
};

}  // namespace

// The small block algebra, for the fit above (PcaFit::gram, ::rotate and the start block) and for hopfield.hip
int dca_pca_small_chunks(int rows) { return ceil_div(rows, kGramRows); }
int dca_pca_small_init(dca_ctx* ctx, const char* who, double* dV, int rows, int b, uint64_t seed)
{
    hipLaunchKernelGGL(pca_init_kernel, dim3((unsigned)(((size_t)rows * b + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, dV,
                       rows, b, seed);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}
int dca_pca_small_gram(dca_ctx* ctx, const char* who, const double* dA, int ba, const double* dB, int bb, int rows, bool diag,
                       double* dGpart, double* dOut)
{
    const int pairs = diag ? ba : ba * bb, chunks = ceil_div(rows, kGramRows);
    ScopedKernelClock kc(ctx, "pca_small");
    hipLaunchKernelGGL(pca_gram_kernel, dim3(chunks, ceil_div(pairs, kThreads)), dim3(kThreads), 0, ctx->stream, dA, ba, dB, bb, rows,
                       diag ? 1 : 0, dGpart);
    hipLaunchKernelGGL(pca_sum_kernel, dim3(ceil_div(pairs, kThreads)), dim3(kThreads), 0, ctx->stream, (const double*)dGpart, chunks, pairs,
                       dOut);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}
int dca_pca_small_rotate(dca_ctx* ctx, const char* who, const double* dA, const double* dT1, const double* dB, const double* dT2, int rows,
                         int b, double* dOut)
{
    ScopedKernelClock kc(ctx, "pca_small");
    hipLaunchKernelGGL(pca_rotate_kernel, dim3((unsigned)(((size_t)rows * b + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream, dA,
                       dT1, dB, dT2, rows, b, dOut);
    HIP_TRY_AS(hipGetLastError(), who);
    return DCA_OK;
}

int dca_pca_fit_impl(dca_ctx* ctx, int k, double tol, int max_iterations, uint64_t seed, double* eigenvalues_out,
                     double* components_out, double* offsets_out, double* residuals_out, double* total_variance_out,
                     int* iterations_out, int* converged_out)
{
    static const char* who = "dca_pca_fit";
    PcaFit S;
    S.ctx = ctx; S.who = who;
    const int N = S.N = ctx->N, L = S.L = ctx->L, q = S.q = ctx->q;
    S.Ls = ctx->Ls;
    const int rows = S.rows = L * q, b = S.b = std::min(rows, k + 8);
    S.slabs = ceil_div(N, kSlab);
    S.chunks = ceil_div(rows, kGramRows);
    S.Ns = (int)round_up((size_t)N, 64);

    // Meff = sum_n w_n, ascending, on the host
    std::vector<double> w(N);
    HIP_TRY_AS(hipStreamSynchronize(ctx->stream), who);
    DCA_TRY(download(ctx, who, w.data(), ctx->dWd, (size_t)N * sizeof(double)));
    double meff = 0.0;
    for (int n = 0; n < N; ++n) {
        if (!(w[n] >= 0.0) || !std::isfinite(w[n])) { dca_set_error("%s: weight %g of sequence %d is negative or not finite", who, w[n], n); return DCA_ERR_ARG; }
        meff += w[n];
    }
    if (!(meff > 0.0)) { dca_set_error("%s: the weights sum to zero", who); return DCA_ERR_ARG; }
    S.meff = meff;

    PCA_ALLOC(S.dXT, (size_t)L * S.Ns);
    PCA_ALLOC(S.dF, (size_t)rows);
    PCA_ALLOC(S.dV, (size_t)rows * b);
    PCA_ALLOC(S.dY, (size_t)rows * b);
    PCA_ALLOC(S.dR, (size_t)rows * b);
    PCA_ALLOC(S.dWP, (size_t)N * b);
    PCA_ALLOC(S.dYpart, (size_t)S.slabs * rows * b);
    PCA_ALLOC(S.dTpart, (size_t)S.slabs * b);
    PCA_ALLOC(S.dGpart, (size_t)S.chunks * b * b);
    PCA_ALLOC(S.dSmall, (size_t)b * b);
    PCA_ALLOC(S.dT1, (size_t)b * b);
    PCA_ALLOC(S.dT2, (size_t)b * b);
    PCA_ALLOC(S.dC, (size_t)b);
    DCA_TRY(transpose_rows(ctx, who, ctx->dX, S.Ls, N, L, S.Ns, S.dXT));

    // f(i,a): the back-projection of the one column w
    DCA_TRY(S.back(ctx->dWd, 1, nullptr, S.dF));
    std::vector<double> f(rows);
    DCA_TRY(download(ctx, who, f.data(), S.dF, (size_t)rows * sizeof(double)));
    double total = 0.0;
    for (int i = 0; i < L; ++i) {
        double s2 = 0.0;
        for (int a = 0; a < q; ++a) s2 += f[(size_t)i * q + a] * f[(size_t)i * q + a];
        total += 1.0 - s2;
    }
    if (total_variance_out) *total_variance_out = total;

    std::vector<double> theta(b, 0.0), res(b, 0.0), U((size_t)b * b), H((size_t)b * b), T((size_t)b * b);
    int it = 0, converged = 0;
    // a trace at the rounding level of its own L sums: C is zero (one sequence, a constant alignment); every component is null
    const bool zero = !(total > 4.0 * (double)L * 0x1.0p-52);
    if (zero) {
        converged = 1;
        HIP_TRY_AS(hipMemsetAsync(S.dV, 0, (size_t)rows * b * sizeof(double), ctx->stream), who);
    } else {
        DCA_TRY(dca_pca_small_init(ctx, who, S.dV.get(), rows, b, seed));
        DCA_TRY(S.orthonormalise(H, T));
    }
    while (!zero) {
        ++it;
        DCA_TRY(S.gram(S.dV, b, S.dF, 1, false, S.dC));                                   // c = V^T f
        DCA_TRY(launch_project(ctx, who, S.dXT, S.Ns, N, L, q, S.dV, b, b, S.dC, ctx->dWd, S.dWP, b));
        DCA_TRY(S.back(S.dWP, b, S.dF, S.dY));                                            // Y = C V
        DCA_TRY(S.gram(S.dV, b, S.dY, b, false, S.dSmall));                               // H = V^T Y
        DCA_TRY(download(ctx, who, H.data(), S.dSmall, (size_t)b * b * sizeof(double)));
        pca_sym_eigh(b, H.data(), U.data(), theta.data());
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) T[(size_t)i * b + j] = -(U[(size_t)i * b + j] * theta[j]);
        DCA_TRY(upload(ctx, who, S.dT1, U.data(), (size_t)b * b * sizeof(double)));
        DCA_TRY(upload(ctx, who, S.dT2, T.data(), (size_t)b * b * sizeof(double)));
        DCA_TRY(S.rotate(S.dY, S.dT1, S.dV, S.dT2, S.dR));                                // R = Y U - V U Theta
        DCA_TRY(S.gram(S.dR, b, S.dR, b, true, S.dSmall));
        DCA_TRY(download(ctx, who, res.data(), S.dSmall, (size_t)b * sizeof(double)));
        converged = 1;
        for (int m = 0; m < b; ++m) {
            res[m] = std::sqrt(res[m]);
            if (m < k && !(res[m] <= tol * theta[0])) converged = 0;
        }
        if (converged || it >= max_iterations) {
            DCA_TRY(S.rotate(S.dV, S.dT1, nullptr, nullptr, S.dR));                       // the Ritz vectors V U
            S.dV.swap(S.dR);
            break;
        }
        DCA_TRY(S.rotate(S.dY, S.dT1, nullptr, nullptr, S.dR));                           // the next block: orth(Y U)
        S.dV.swap(S.dR);
        DCA_TRY(S.orthonormalise(H, T));
    }

    std::vector<double> Vh((size_t)rows * b);
    DCA_TRY(download(ctx, who, Vh.data(), S.dV, (size_t)rows * b * sizeof(double)));
    for (int m = 0; m < k; ++m) {
        double* v = components_out + (size_t)m * rows;
        const bool null = zero || pca_is_null(theta[m], theta[0], tol);
        for (int r = 0; r < rows; ++r) v[r] = null ? 0.0 : Vh[(size_t)r * b + m];
        pca_fix_sign((size_t)rows, v);
        double c = 0.0;
        for (int r = 0; r < rows; ++r) c += f[r] * v[r];               // ascending (i, a), one chain
        eigenvalues_out[m] = null ? 0.0 : theta[m];
        offsets_out[m] = null ? 0.0 : c;
        if (residuals_out) residuals_out[m] = res[m];
    }
    if (iterations_out) *iterations_out = it;
    *converged_out = converged;
    return DCA_OK;
}

int dca_pca_project_impl(dca_ctx* ctx, const uint8_t* Q, int nq, int k, const double* components, const double* offsets,
                         double* proj_out)
{
    static const char* who = "dca_pca_project";
    const int L = ctx->L, q = ctx->q, Ls = ctx->Ls, rows = L * q;
    if (Q) DCA_TRY(dca_check_codes(Q, (size_t)nq * L, q, "dca_pca_project: "));
    const int n = Q ? nq : ctx->N;
    const int pass = Q ? std::min(n, dca_nn_pass_size()) : n;
    const int Ns = (int)round_up((size_t)pass, 64);

    std::vector<double> Vh((size_t)rows * k);                          // row (i, a), column m
    for (int m = 0; m < k; ++m)
        for (int r = 0; r < rows; ++r) Vh[(size_t)r * k + m] = components[(size_t)m * rows + r];
    DevBuf<double> dV, dC, dP;
    DevBuf<uint8_t> dRows, dXT;
    PCA_ALLOC(dV, (size_t)rows * k);
    PCA_ALLOC(dC, (size_t)k);
    PCA_ALLOC(dP, (size_t)pass * k);
    PCA_ALLOC(dXT, (size_t)L * Ns);
    if (Q) PCA_ALLOC(dRows, (size_t)pass * Ls);
    DCA_TRY(upload(ctx, who, dV, Vh.data(), (size_t)rows * k * sizeof(double)));
    DCA_TRY(upload(ctx, who, dC, offsets, (size_t)k * sizeof(double)));
    for (int first = 0; first < n; first += pass) {
        const int m = std::min(pass, n - first);
        const uint8_t* src = ctx->dX;
        if (Q) {
            HIP_TRY_AS(hipMemsetAsync(dRows, 0, (size_t)m * Ls, ctx->stream), who);
            HIP_TRY_AS(hipMemcpy2DAsync(dRows, (size_t)Ls, Q + (size_t)first * L, (size_t)L, (size_t)L, (size_t)m, hipMemcpyHostToDevice,
                                        ctx->stream), who);
            src = dRows;
        }
        DCA_TRY(transpose_rows(ctx, who, src, Ls, m, L, Ns, dXT));
        DCA_TRY(launch_project(ctx, who, dXT, Ns, m, L, q, dV, k, k, dC, nullptr, dP, k));
        DCA_TRY(download(ctx, who, proj_out + (size_t)first * k, dP, (size_t)m * k * sizeof(double)));
    }
    return DCA_OK;
}
