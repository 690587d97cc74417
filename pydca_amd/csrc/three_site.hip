// Three-site connected correlations of the alignment or of a sequence set (dca_three_site_values, dca_three_site_scan;
// DESIGN.md section 20).  Everything that is summed is an integer: sequence n carries the weight wq_n = llrint(w_n 2^40) (the
// alignment) or 1 (a set), every count is a uint64 sum of wq over the matching sequences, the denominator is M = sum_n wq_n, a
// frequency is (double)count / (double)M and
//   c_ijk(a,b,c) = f_ijk - f_ij(a,b) f_k(c) - f_ik(a,c) f_j(b) - f_jk(b,c) f_i(a) + 2.0 f_i(a) f_j(b) f_k(c)
// is formed in double, left to right, without contraction.  No float atomics: the results do not depend on the launch geometry,
// the order of the atomics or the pass split.
//   ts_site_kernel / ts_pair_kernel   the frequency tables F1 (L q) and F2 (pairs q^2) of a call, from LDS integer histograms
//   ts_scan_kernel                    persistent workgroups; one work item = (site i, state a, TB x TB tile of later sites (j, k)).
//                                     The item walks the list of the sequences with s_i = a once (4 or 8 code bytes per tile side
//                                     in one load from the row-major rows), adds wq into TB^2 q^2 uint64 LDS cells with LDS
//                                     atomics, then turns its own cells into c_ijk.  Mode 0 bins |c| into a 1024-bin LDS histogram
//                                     that is flushed once per workgroup; mode 1 appends the elements at or above an edge.
//   ts_values_*                       T listed elements: one workgroup per site triple counts its one- and two-site tables in LDS
//                                     and its elements' cells (binary search of the sequence's (a, b, c) among the triple's sorted
//                                     keys) through 64-bit integer atomics.
// Selection of the top K (host, exact, memory O(K)): histogram pass -> the edge bin that holds the K-th largest |c| -> at most one
// refinement of that bin on lower bits -> append pass into a buffer whose size the histogram gave -> sort by (|c| descending,
// linear index ascending).  The appended SET fixes the result, never its order.
#include "dca_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace {

constexpr int kScanThreads = 512;
constexpr int kBins = 1024;
constexpr int kThreads = 256;
constexpr int kPairChunk = 4;                     // later sites per workgroup of ts_pair_kernel
constexpr uint64_t kCandCapBase = 1ull << 20;     // cap of the append buffer: 16 K + 2^20 records

struct TsRecord { uint64_t idx; double c; uint64_t count; };

// ---------------------------------------------------------------- tables
__global__ __launch_bounds__(kThreads)
void ts_site_kernel(const uint8_t* __restrict__ X, const uint64_t* __restrict__ W, int n, int Ls, int q, double Md,
                    double* __restrict__ F1)
{
    __shared__ unsigned long long cells[32];
    const int i = blockIdx.x, t = threadIdx.x;
    if (t < 32) cells[t] = 0ull;
    __syncthreads();
    for (int s = t; s < n; s += kThreads) atomicAdd(&cells[X[(size_t)s * Ls + i]], W ? (unsigned long long)W[s] : 1ull);
    __syncthreads();
    if (t < q) F1[(size_t)i * q + t] = (double)cells[t] / Md;
}

// grid (ceil(L / 4), L): site i = blockIdx.y against the sites j = 4 blockIdx.x .. + 3 that lie behind it
__global__ __launch_bounds__(kThreads)
void ts_pair_kernel(const uint8_t* __restrict__ X, const uint64_t* __restrict__ W, int n, int L, int Ls, int q, double Md,
                    double* __restrict__ F2)
{
    extern __shared__ unsigned long long pcells[];             // kPairChunk * q * q
    const int i = blockIdx.y, j0 = blockIdx.x * kPairChunk, t = threadIdx.x, qq = q * q;
    if (j0 + kPairChunk - 1 <= i) return;
    for (int e = t; e < kPairChunk * qq; e += kThreads) pcells[e] = 0ull;
    __syncthreads();
    for (int s = t; s < n; s += kThreads) {
        const uint8_t* row = X + (size_t)s * Ls;
        const unsigned long long w = W ? (unsigned long long)W[s] : 1ull;
        const int a = row[i];
        const uint32_t jw = *reinterpret_cast<const uint32_t*>(row + j0);      // Ls is a multiple of 128: in the row, aligned
#pragma unroll
        for (int u = 0; u < kPairChunk; ++u) {
            const int j = j0 + u;
            if (j > i && j < L) atomicAdd(&pcells[u * qq + a * q + (int)((jw >> (8 * u)) & 0xffu)], w);
        }
    }
    __syncthreads();
    for (int e = t; e < kPairChunk * qq; e += kThreads) {
        const int u = e / qq, j = j0 + u;
        if (j > i && j < L) F2[pair_index(L, i, j) * qq + (e - u * qq)] = (double)pcells[e] / Md;
    }
}

// ---------------------------------------------------------------- scan
struct TsScanArgs {
    const uint8_t* X; const uint64_t* W; const int32_t* perm; const int32_t* off; const int2* tiles;
    const double* F1; const double* F2;
    int n, L, Ls, q, nT, skip;
    unsigned long long items;
    double Md;
    int mode;                                  // 0: histogram, 1: append
    unsigned long long flo, fhi, lo; int sh;   // mode 0: elements with flo <= bits < fhi, key = clamp((bits >> sh) - lo, 0, 1023)
    unsigned long long* hist;                  // mode 0: kBins global bins
    unsigned long long edge, cap;              // mode 1: elements with bits >= edge
    unsigned long long* cursor; TsRecord* rec;
};

template <int TB> struct TileWord;
template <> struct TileWord<2> { typedef uint16_t type; };
template <> struct TileWord<4> { typedef uint32_t type; };
template <> struct TileWord<8> { typedef uint64_t type; };

template <int TB>
__global__ __launch_bounds__(kScanThreads)
void ts_scan_kernel(const TsScanArgs A)
{
    extern __shared__ unsigned long long lds[];
    typedef typename TileWord<TB>::type word_t;
    const int t = threadIdx.x, q = A.q, qq = q * q, L = A.L, ncell = TB * TB * qq;
    unsigned long long* cells = lds;
    unsigned long long* lhist = lds + ncell;
    if (A.mode == 0) {
        for (int b = t; b < kBins; b += kScanThreads) lhist[b] = 0ull;
    }
    for (unsigned long long item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int ia = (int)(item / (unsigned long long)A.nT), tl = (int)(item - (unsigned long long)ia * A.nT);
        const int i = ia / q, a = ia - i * q;
        const int2 jk = A.tiles[tl];
        const int j0 = jk.x * TB, k0 = jk.y * TB;
        // uniform over the workgroup: nothing of this tile lies behind site i, or the state is left out
        if (a == A.skip || j0 + TB - 1 <= i || k0 + TB - 1 <= i + 1) continue;
        __syncthreads();                                   // the previous item's cells have been read
        for (int e = t; e < ncell; e += kScanThreads) cells[e] = 0ull;
        __syncthreads();
        const int lb = A.off[i * (q + 1) + a], le = A.off[i * (q + 1) + a + 1];
        const int32_t* list = A.perm + (size_t)i * A.n;
        for (int x = lb + t; x < le; x += kScanThreads) {
            const int s = list[x];
            const unsigned long long w = A.W ? (unsigned long long)A.W[s] : 1ull;
            const uint8_t* row = A.X + (size_t)s * A.Ls;
            const word_t jw = *reinterpret_cast<const word_t*>(row + j0);      // tile starts are multiples of TB, Ls of 128
            const word_t kw = *reinterpret_cast<const word_t*>(row + k0);
#pragma unroll
            for (int u = 0; u < TB; ++u) {
                const int j = j0 + u, b = (int)((jw >> (8 * u)) & 0xffu);
                if (j <= i) continue;
#pragma unroll
                for (int v = 0; v < TB; ++v) {
                    const int k = k0 + v;
                    if (k > j && k < L) atomicAdd(&cells[(u * TB + v) * qq + b * q + (int)((kw >> (8 * v)) & 0xffu)], w);
                }
            }
        }
        __syncthreads();
        const double fi = A.F1[(size_t)i * q + a];
        for (int e = t; e < ncell; e += kScanThreads) {
            const int p = e / qq, bc = e - p * qq;
            const int u = p / TB, v = p - u * TB, j = j0 + u, k = k0 + v;
            if (j <= i || k <= j || k >= L) continue;
            const int b = bc / q, c = bc - b * q;
            if (b == A.skip || c == A.skip) continue;
            const unsigned long long cnt = cells[e];
            const double f3 = (double)cnt / A.Md;
            const double fj = A.F1[(size_t)j * q + b], fk = A.F1[(size_t)k * q + c];
            const double fij = A.F2[pair_index(L, i, j) * qq + a * q + b];
            const double fik = A.F2[pair_index(L, i, k) * qq + a * q + c];
            const double fjk = A.F2[pair_index(L, j, k) * qq + b * q + c];
            const double c3 = f3 - fij * fk - fik * fj - fjk * fi + 2.0 * fi * fj * fk;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(fabs(c3));
            if (A.mode == 0) {
                if (bits < A.flo || bits >= A.fhi) continue;
                const unsigned long long kv = bits >> A.sh;
                const unsigned long long key = kv > A.lo ? kv - A.lo : 0ull;
                atomicAdd(&lhist[key < (unsigned long long)(kBins - 1) ? key : (unsigned long long)(kBins - 1)], 1ull);
            } else if (bits >= A.edge) {
                const unsigned long long pos = atomicAdd(A.cursor, 1ull);
                if (pos < A.cap) {
                    TsRecord r;
                    r.idx = (((((unsigned long long)i * L + j) * L + k) * q + a) * q + b) * q + c;
                    r.c = c3; r.count = cnt;
                    A.rec[pos] = r;
                }
            }
        }
    }
    if (A.mode == 0) {
        __syncthreads();
        for (int b = t; b < kBins; b += kScanThreads)
            if (lhist[b]) atomicAdd(&A.hist[b], lhist[b]);
    }
}

// ---------------------------------------------------------------- values
// tables of group g at gtab + g * (3 q + 3 q^2): n_i, n_j, n_k, then n_ij, n_ik, n_jk
__global__ __launch_bounds__(kThreads)
void ts_values_count_kernel(const uint8_t* __restrict__ X, const uint64_t* __restrict__ W, int n, int Ls, int q,
                            const int32_t* __restrict__ tri, const int32_t* __restrict__ goff, const int32_t* __restrict__ keys,
                            unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ gtab)
{
    __shared__ unsigned long long tab[3 * 32 + 3 * 32 * 32];
    const int g = blockIdx.x, t = threadIdx.x, qq = q * q, nt = 3 * q + 3 * qq;
    const int i = tri[3 * g], j = tri[3 * g + 1], k = tri[3 * g + 2];
    const int e0 = goff[g], e1 = goff[g + 1];
    for (int e = t; e < nt; e += kThreads) tab[e] = 0ull;
    __syncthreads();
    for (int s = t; s < n; s += kThreads) {
        const uint8_t* row = X + (size_t)s * Ls;
        const unsigned long long w = W ? (unsigned long long)W[s] : 1ull;
        const int a = row[i], b = row[j], c = row[k];
        atomicAdd(&tab[a], w); atomicAdd(&tab[q + b], w); atomicAdd(&tab[2 * q + c], w);
        atomicAdd(&tab[3 * q + a * q + b], w); atomicAdd(&tab[3 * q + qq + a * q + c], w); atomicAdd(&tab[3 * q + 2 * qq + b * q + c], w);
        const int key = (a * q + b) * q + c;
        int lo = e0, hi = e1;                   // first position with keys[pos] >= key
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < e1 && keys[lo] == key) atomicAdd(&cnt[lo], w);
    }
    __syncthreads();
    // one workgroup per group and the passes follow one another on the stream: a plain add
    for (int e = t; e < nt; e += kThreads) gtab[(size_t)g * nt + e] += tab[e];
}

__global__ __launch_bounds__(kThreads)
void ts_values_final_kernel(int U, int q, double Md, const int32_t* __restrict__ grp, const int32_t* __restrict__ keys,
                            const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ gtab,
                            double* __restrict__ f3_out, double* __restrict__ c3_out)
{
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= U) return;
    const int qq = q * q, nt = 3 * q + 3 * qq;
    const unsigned long long* tab = gtab + (size_t)grp[u] * nt;
    const int key = keys[u], a = key / qq, b = (key - a * qq) / q, c = key - a * qq - b * q;
    const double f3 = (double)cnt[u] / Md;
    const double fi = (double)tab[a] / Md, fj = (double)tab[q + b] / Md, fk = (double)tab[2 * q + c] / Md;
    const double fij = (double)tab[3 * q + a * q + b] / Md, fik = (double)tab[3 * q + qq + a * q + c] / Md;
    const double fjk = (double)tab[3 * q + 2 * qq + b * q + c] / Md;
    f3_out[u] = f3;
    c3_out[u] = f3 - fij * fk - fik * fj - fjk * fi + 2.0 * fi * fj * fk;
}

// ---------------------------------------------------------------- host side
// the context's weights as integers on the device; *M = their sum
int ts_alignment_weights(dca_ctx* ctx, const char* who, DevBuf<uint64_t>* dW, uint64_t* M)
{
    const int N = ctx->N;
    if (N > (1 << 23)) { dca_set_error("%s: %d sequences are more than the 2^23 the integer sums allow", who, N); return DCA_ERR_ARG; }
    std::vector<double> w(N);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(w.data(), ctx->dWd, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<uint64_t> wq(N);
    uint64_t sum = 0;
    for (int s = 0; s < N; ++s) {
        const long long v = llrint(w[s] * 0x1.0p40);
        if (!(w[s] >= 0.0) || v < 0 || v > (1ll << 40)) { dca_set_error("%s: weight %g of sequence %d is outside [0, 1]", who, w[s], s); return DCA_ERR_ARG; }
        wq[s] = (uint64_t)v;
        sum += (uint64_t)v;
    }
    if (sum == 0) { dca_set_error("%s: the weights sum to zero", who); return DCA_ERR_ARG; }
    if (dW->alloc((size_t)N, false) != hipSuccess) {
        dca_set_error("%s: out of device memory", who);
        return DCA_ERR_NOMEM;
    }
    HIP_TRY(hipMemcpy(dW->get(), wq.data(), (size_t)N * sizeof(uint64_t), hipMemcpyHostToDevice));
    *M = sum;
    return DCA_OK;
}

// rows n x L (tight) -> a device block of n rows of stride Ls, zero padded
int ts_upload_rows(const uint8_t* rows, int n, int L, int Ls, uint8_t* dst)
{
    HIP_TRY(hipMemset(dst, 0, (size_t)n * Ls));
    HIP_TRY(hipMemcpy2D(dst, (size_t)Ls, rows, (size_t)L, (size_t)L, (size_t)n, hipMemcpyHostToDevice));
    return DCA_OK;
}

int tile_side(int q)        // the largest of 8, 4, 2 whose TB^2 q^2 uint64 cells fit 56 KiB of LDS (q = 21: 4, q = 5: 8, q = 32: 2)
{
    for (int tb = 8; tb > 2; tb >>= 1)
        if (tb * tb * q * q <= 7168) return tb;
    return 2;
}

hipError_t launch_scan(dca_ctx* ctx, int TB, int grid, const TsScanArgs& A)
{
    const size_t lds = ((size_t)TB * TB * A.q * A.q + kBins) * sizeof(unsigned long long);
    ScopedKernelClock kc(ctx, "three_site_scan");
    if (TB == 8) hipLaunchKernelGGL(ts_scan_kernel<8>, dim3(grid), dim3(kScanThreads), lds, ctx->stream, A);
    else if (TB == 4) hipLaunchKernelGGL(ts_scan_kernel<4>, dim3(grid), dim3(kScanThreads), lds, ctx->stream, A);
    else hipLaunchKernelGGL(ts_scan_kernel<2>, dim3(grid), dim3(kScanThreads), lds, ctx->stream, A);
    return hipGetLastError();
}

// a buffer of max(count, 1) elements, not zeroed; out of memory is DCA_ERR_NOMEM
#define TS_ALLOC(buf, count) HIP_TRY_AS_NOMEM((buf).alloc(std::max<size_t>(count, 1), false), who)

}  // namespace

int dca_three_site_values_impl(dca_ctx* ctx, const uint8_t* Q, int nq, const int32_t* elements, int T, uint64_t* count_out,
                               uint64_t* denom_out, double* f3_out, double* c3_out)
{
    static const char* who = "dca_three_site_values";
    const int L = ctx->L, q = ctx->q, Ls = ctx->Ls, qq = q * q;
    for (int e = 0; e < T; ++e) {
        const int32_t* r = elements + (size_t)6 * e;
        if (!(0 <= r[0] && r[0] < r[1] && r[1] < r[2] && r[2] < L)) {
            dca_set_error("%s: element %d names the sites (%d, %d, %d); they must satisfy 0 <= i < j < k < %d", who, e, r[0], r[1], r[2], L);
            return DCA_ERR_ARG;
        }
        for (int s = 3; s < 6; ++s)
            if (r[s] < 0 || r[s] >= q) { dca_set_error("%s: element %d names the state %d; states are 0 .. %d", who, e, r[s], q - 1); return DCA_ERR_ARG; }
    }
    if (Q) DCA_TRY(dca_check_codes(Q, (size_t)nq * L, q, "dca_three_site_values: "));

    // the elements sorted by (triple, key) without duplicates: slot u; the triples' groups
    std::vector<int> ord(T);
    for (int e = 0; e < T; ++e) ord[e] = e;
    auto el_less = [&](int x, int y) {
        const int32_t *a = elements + (size_t)6 * x, *b = elements + (size_t)6 * y;
        return std::lexicographical_compare(a, a + 6, b, b + 6);
    };
    std::sort(ord.begin(), ord.end(), el_less);
    std::vector<int32_t> slot(T), keys, grp, tri, goff;
    for (int x = 0; x < T; ++x) {
        const int32_t* r = elements + (size_t)6 * ord[x];
        const bool same_el = x > 0 && std::equal(r, r + 6, elements + (size_t)6 * ord[x - 1]);
        if (!same_el) {
            const bool same_tri = x > 0 && std::equal(r, r + 3, elements + (size_t)6 * ord[x - 1]);
            if (!same_tri) { goff.push_back((int32_t)keys.size()); tri.insert(tri.end(), r, r + 3); }
            keys.push_back((r[3] * q + r[4]) * q + r[5]);
            grp.push_back((int32_t)goff.size() - 1);
        }
        slot[ord[x]] = (int32_t)keys.size() - 1;
    }
    goff.push_back((int32_t)keys.size());
    const int U = (int)keys.size(), G = (int)goff.size() - 1, nt = 3 * q + 3 * qq;

    DevBuf<uint64_t> dW;
    uint64_t M = (uint64_t)nq;
    if (!Q) DCA_TRY(ts_alignment_weights(ctx, who, &dW, &M));
    DevBuf<int32_t> dTri, dGoff, dKeys, dGrp;
    DevBuf<unsigned long long> dCnt, dTab;
    DevBuf<double> dF3, dC3;
    DevBuf<uint8_t> dRows;
    TS_ALLOC(dTri, tri.size());
    TS_ALLOC(dGoff, goff.size());
    TS_ALLOC(dKeys, keys.size());
    TS_ALLOC(dGrp, grp.size());
    TS_ALLOC(dCnt, (size_t)U);
    HIP_TRY_AS_NOMEM(hipMemsetAsync(dCnt, 0, std::max<size_t>(U, 1) * sizeof(unsigned long long), ctx->stream), who);
    TS_ALLOC(dTab, (size_t)G * nt);
    HIP_TRY_AS_NOMEM(hipMemsetAsync(dTab, 0, std::max<size_t>((size_t)G * nt, 1) * sizeof(unsigned long long), ctx->stream), who);
    TS_ALLOC(dF3, (size_t)U);
    TS_ALLOC(dC3, (size_t)U);
    const int pass = Q ? std::min(nq, dca_nn_pass_size()) : 0;
    if (Q) TS_ALLOC(dRows, (size_t)pass * Ls);
    HIP_TRY_AS_NOMEM(hipMemcpyAsync(dTri, tri.data(), tri.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS_NOMEM(hipMemcpyAsync(dGoff, goff.data(), goff.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS_NOMEM(hipMemcpyAsync(dKeys, keys.data(), keys.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS_NOMEM(hipMemcpyAsync(dGrp, grp.data(), grp.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), who);
    HIP_TRY_AS_NOMEM(hipStreamSynchronize(ctx->stream), who);
    if (!Q) {
        ScopedKernelClock kc(ctx, "three_site_values");
        hipLaunchKernelGGL(ts_values_count_kernel, dim3(G), dim3(kThreads), 0, ctx->stream, ctx->dX, dW, ctx->N, Ls, q, dTri, dGoff,
                           dKeys, dCnt, dTab);
        HIP_TRY_AS_NOMEM(hipGetLastError(), who);
    } else {
        for (int first = 0; first < nq; first += pass) {
            const int m = std::min(pass, nq - first);
            HIP_TRY_AS_NOMEM(hipStreamSynchronize(ctx->stream), who);          // the previous pass has read the rows
            DCA_TRY(ts_upload_rows(Q + (size_t)first * L, m, L, Ls, dRows));
            ScopedKernelClock kc(ctx, "three_site_values");
            hipLaunchKernelGGL(ts_values_count_kernel, dim3(G), dim3(kThreads), 0, ctx->stream, dRows, (const uint64_t*)nullptr, m, Ls,
                               q, dTri, dGoff, dKeys, dCnt, dTab);
            HIP_TRY_AS_NOMEM(hipGetLastError(), who);
        }
    }
    {
        ScopedKernelClock kc(ctx, "three_site_values");
        hipLaunchKernelGGL(ts_values_final_kernel, dim3(ceil_div(U, kThreads)), dim3(kThreads), 0, ctx->stream, U, q, (double)M, dGrp,
                           dKeys, dCnt, dTab, dF3, dC3);
        HIP_TRY_AS_NOMEM(hipGetLastError(), who);
    }
    HIP_TRY_AS_NOMEM(hipStreamSynchronize(ctx->stream), who);
    std::vector<uint64_t> hc(count_out ? U : 0);
    std::vector<double> hf(f3_out ? U : 0), hcc(c3_out ? U : 0);
    if (count_out) HIP_TRY_AS_NOMEM(hipMemcpy(hc.data(), dCnt, (size_t)U * sizeof(uint64_t), hipMemcpyDeviceToHost), who);
    if (f3_out) HIP_TRY_AS_NOMEM(hipMemcpy(hf.data(), dF3, (size_t)U * sizeof(double), hipMemcpyDeviceToHost), who);
    if (c3_out) HIP_TRY_AS_NOMEM(hipMemcpy(hcc.data(), dC3, (size_t)U * sizeof(double), hipMemcpyDeviceToHost), who);
    for (int e = 0; e < T; ++e) {
        if (count_out) count_out[e] = hc[slot[e]];
        if (f3_out) f3_out[e] = hf[slot[e]];
        if (c3_out) c3_out[e] = hcc[slot[e]];
    }
    if (denom_out) *denom_out = M;
    return DCA_OK;
}

int dca_three_site_scan_impl(dca_ctx* ctx, const uint8_t* Q, int nq, int K, int skip_state, int32_t* elements_out, double* c3_out,
                             double* f3_out, int* found)
{
    static const char* who = "dca_three_site_scan";
    const int L = ctx->L, q = ctx->q, Ls = ctx->Ls, qq = q * q;
    const int n = Q ? nq : ctx->N;
    const size_t pairs = (size_t)L * (L - 1) / 2;
    if (Q) DCA_TRY(dca_check_codes(Q, (size_t)nq * L, q, "dca_three_site_scan: "));
    const uint8_t* rows = Q ? Q : dca_host_msa(ctx);
    if (!rows) { dca_set_error("%s: cannot read the alignment back", who); return DCA_ERR_HIP; }
    const int skip = skip_state >= 0 && skip_state < q ? skip_state : -1;

    DevBuf<uint64_t> dW;
    uint64_t M = (uint64_t)nq;
    if (!Q) DCA_TRY(ts_alignment_weights(ctx, who, &dW, &M));
    // the sequences of every (site, state), the layout of the mean-field counting lists: perm[i * n + off[i][a] .. off[i][a + 1])
    std::vector<int32_t> off((size_t)L * (q + 1), 0), perm((size_t)L * n);
    for (int s = 0; s < n; ++s)
        for (int i = 0; i < L; ++i) off[(size_t)i * (q + 1) + rows[(size_t)s * L + i] + 1] += 1;
    for (int i = 0; i < L; ++i)
        for (int a = 0; a < q; ++a) off[(size_t)i * (q + 1) + a + 1] += off[(size_t)i * (q + 1) + a];
    {
        std::vector<int32_t> cur((size_t)L * q);
        for (int i = 0; i < L; ++i)
            for (int a = 0; a < q; ++a) cur[(size_t)i * q + a] = off[(size_t)i * (q + 1) + a];
        for (int s = 0; s < n; ++s)
            for (int i = 0; i < L; ++i) perm[(size_t)i * n + cur[(size_t)i * q + rows[(size_t)s * L + i]]++] = s;
    }
    const int TB = tile_side(q), nt1 = ceil_div(L, TB);
    std::vector<int2> tiles;
    for (int jt = 0; jt < nt1; ++jt)
        for (int kt = jt; kt < nt1; ++kt) tiles.push_back(make_int2(jt, kt));
    const int nT = (int)tiles.size();

    DevBuf<uint8_t> dRows;
    DevBuf<int32_t> dPerm, dOff;
    DevBuf<int2> dTiles;
    DevBuf<double> dF1, dF2;
    DevBuf<unsigned long long> dHist, dCursor;
    DevBuf<TsRecord> dRec;
    if (Q) {
        TS_ALLOC(dRows, (size_t)n * Ls);
        DCA_TRY(ts_upload_rows(Q, n, L, Ls, dRows));
    }
    const uint8_t* dX = Q ? dRows.get() : ctx->dX;
    TS_ALLOC(dPerm, perm.size());
    TS_ALLOC(dOff, off.size());
    TS_ALLOC(dTiles, tiles.size());
    TS_ALLOC(dF1, (size_t)L * q);
    TS_ALLOC(dF2, pairs * qq);
    TS_ALLOC(dHist, (size_t)kBins);
    TS_ALLOC(dCursor, (size_t)1);
    HIP_TRY_AS_NOMEM(hipMemsetAsync(dCursor, 0, sizeof(unsigned long long), ctx->stream), who);
    HIP_TRY_AS_NOMEM(hipMemcpy(dPerm, perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice), who);
    HIP_TRY_AS_NOMEM(hipMemcpy(dOff, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice), who);
    HIP_TRY_AS_NOMEM(hipMemcpy(dTiles, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice), who);

    const double Md = (double)M;
    hipLaunchKernelGGL(ts_site_kernel, dim3(L), dim3(kThreads), 0, ctx->stream, dX, dW, n, Ls, q, Md, dF1);
    hipLaunchKernelGGL(ts_pair_kernel, dim3(ceil_div(L, kPairChunk), L), dim3(kThreads), (size_t)kPairChunk * qq * sizeof(unsigned long long),
                       ctx->stream, dX, dW, n, L, Ls, q, Md, dF2);
    HIP_TRY_AS_NOMEM(hipGetLastError(), who);

    hipDeviceProp_t prop;
    HIP_TRY_AS_NOMEM(hipGetDeviceProperties(&prop, ctx->device), who);
    TsScanArgs A{};
    A.X = dX; A.W = dW; A.perm = dPerm; A.off = dOff; A.tiles = dTiles; A.F1 = dF1; A.F2 = dF2;
    A.n = n; A.L = L; A.Ls = Ls; A.q = q; A.nT = nT; A.skip = skip;
    A.items = (unsigned long long)L * q * nT;
    A.Md = Md;
    A.hist = dHist; A.cursor = dCursor;
    // two workgroups of 64 KiB LDS per CU
    const int grid = (int)std::min<unsigned long long>(A.items, (unsigned long long)std::max(1, prop.multiProcessorCount) * 2);

    std::vector<unsigned long long> hist(kBins);
    auto hist_pass = [&](unsigned long long flo, unsigned long long fhi, unsigned long long lo, int sh) -> int {
        A.mode = 0; A.flo = flo; A.fhi = fhi; A.lo = lo; A.sh = sh;
        HIP_TRY_AS_NOMEM(hipMemsetAsync(dHist, 0, kBins * sizeof(unsigned long long), ctx->stream), who);
        HIP_TRY_AS_NOMEM(launch_scan(ctx, TB, grid, A), who);
        HIP_TRY_AS_NOMEM(hipStreamSynchronize(ctx->stream), who);
        HIP_TRY_AS_NOMEM(hipMemcpy(hist.data(), dHist, kBins * sizeof(unsigned long long), hipMemcpyDeviceToHost), who);
        return DCA_OK;
    };
    // level 1: the exponent and 4 mantissa bits of |c|, the 64 binades below 4.0; everything smaller (0 included) in bin 0
    const unsigned long long lo1 = 15376ull;        // (1024 << 4 | 15) + 1 - 1024
    DCA_TRY(hist_pass(0ull, ~0ull, lo1, 48));
    unsigned long long total = 0;
    for (int b = 0; b < kBins; ++b) total += hist[b];
    const unsigned long long want = std::min<unsigned long long>((unsigned long long)K, total);
    *found = (int)want;
    if (want == 0) return DCA_OK;
    auto pick = [&](unsigned long long above, int* bin, unsigned long long* reach) {     // the bin that holds the want-th largest
        unsigned long long acc = above;
        int b = kBins - 1;
        for (; b > 0; --b) {
            if (acc + hist[b] >= want) break;
            acc += hist[b];
        }
        *bin = b; *reach = acc + hist[b];
        return acc;
    };
    const char* cap_env = getenv("DCA_THREE_SITE_CAP");         // a positive count replaces the cap (the tests reach the refinement with it)
    const long long cap_v = cap_env ? atoll(cap_env) : 0;
    const unsigned long long cap = cap_v > 0 ? (unsigned long long)cap_v : 16ull * (unsigned long long)K + kCandCapBase;
    int b1 = 0;
    unsigned long long ncand = 0;
    const unsigned long long above1 = pick(0ull, &b1, &ncand);
    unsigned long long edge = b1 > 0 ? (lo1 + b1) << 48 : 0ull;
    if (ncand > cap) {
        // ties or a crowded bin: once more inside it, on the next 10 mantissa bits (bin 0: on the exponent)
        unsigned long long flo, fhi, lo2; int sh;
        if (b1 > 0) { flo = (lo1 + b1) << 48; fhi = b1 == kBins - 1 ? ~0ull : (lo1 + b1 + 1) << 48; lo2 = (lo1 + b1) << 10; sh = 38; }
        else { flo = 0ull; fhi = (lo1 + 1) << 48; lo2 = 0ull; sh = 52; }
        DCA_TRY(hist_pass(flo, fhi, lo2, sh));
        int b2 = 0;
        pick(above1, &b2, &ncand);
        edge = (b1 > 0 || b2 > 0) ? (lo2 + b2) << sh : 0ull;
        if (ncand > cap) {
            dca_set_error("%s: %llu elements tie with the K-th largest |c| within the resolution of the selection; more than the %llu "
                          "candidates K = %d allows", who, ncand, cap, K);
            return DCA_ERR_ARG;
        }
    }
    TS_ALLOC(dRec, (size_t)ncand);
    A.mode = 1; A.edge = edge; A.cap = ncand; A.rec = dRec;
    HIP_TRY_AS_NOMEM(launch_scan(ctx, TB, grid, A), who);
    HIP_TRY_AS_NOMEM(hipStreamSynchronize(ctx->stream), who);
    unsigned long long appended = 0;
    HIP_TRY_AS_NOMEM(hipMemcpy(&appended, dCursor, sizeof(appended), hipMemcpyDeviceToHost), who);
    if (appended != ncand) {
        dca_set_error("%s: the append pass found %llu elements where the histogram counted %llu", who, appended, ncand);
        return DCA_ERR_HIP;
    }
    std::vector<TsRecord> rec((size_t)ncand);
    HIP_TRY_AS_NOMEM(hipMemcpy(rec.data(), dRec, (size_t)ncand * sizeof(TsRecord), hipMemcpyDeviceToHost), who);
    std::sort(rec.begin(), rec.end(), [](const TsRecord& x, const TsRecord& y) {
        const double ax = std::fabs(x.c), ay = std::fabs(y.c);
        return ax != ay ? ax > ay : x.idx < y.idx;
    });
    for (unsigned long long r = 0; r < want; ++r) {
        unsigned long long v = rec[r].idx;
        int32_t* e = elements_out + 6 * r;
        e[5] = (int32_t)(v % q); v /= q;
        e[4] = (int32_t)(v % q); v /= q;
        e[3] = (int32_t)(v % q); v /= q;
        e[2] = (int32_t)(v % L); v /= L;
        e[1] = (int32_t)(v % L); v /= L;
        e[0] = (int32_t)v;
        if (c3_out) c3_out[r] = rec[r].c;
        if (f3_out) f3_out[r] = (double)rec[r].count / Md;
    }
    return DCA_OK;
}
