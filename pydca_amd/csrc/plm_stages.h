// Stage kernels of one plmDCA evaluation (plm_engine.hip launches them; the stages are listed in its header comment): expand,
// logits, softmax scan, scatter, slab and column sums, the column-strip copies and the fold.  The inner blocks of the two
// gathers are generated assembly (tools/gen_plm_asm.py).  Included by plm_engine.hip only: one translation unit holds all of
// the engine's device code.
#pragma once

#include "dca_internal.h"
#include "plm_plan.h"
#include "vec_kernels.h"

namespace {

#ifdef DCA_FAST_EXP
__device__ __forceinline__ float t_exp(float v) { return __expf(v); }
#else
__device__ __forceinline__ float t_exp(float v) { return expf(v); }
#endif
__device__ __forceinline__ double t_exp(double v) { return exp(v); }
__device__ __forceinline__ float t_log(float v) { return logf(v); }
__device__ __forceinline__ double t_log(double v) { return log(v); }

// block (i<j) from linear pair index (host side builds the table once)
struct PairIJ { uint16_t i, j; };

// ------------------------------------------------------------------ expand
// W[(j,b)][(i,a)] = W[(i,a)][(j,b)] = J_ij(a,b); diagonal blocks and padding stay 0.
// One workgroup per site pair; the q x q block goes through LDS so that both
// writes are runs of q contiguous elements.
// Column window [s0, s1) of sites (the whole alignment unless the column-strip decomposition is on): W, S, R and G hold the
// columns of those sites only, re-based to column 0; their rows always cover all sites.
template <typename T>
__global__ void plm_expand_kernel(const T* __restrict__ x, T* __restrict__ W, const PairIJ* __restrict__ pairs,
                                  int L, int q, int Cs, int s0, int s1)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];
    T* tile = reinterpret_cast<T*>(dca_smem);
    const int p = blockIdx.x;
    const int i = pairs[p].i, j = pairs[p].j;
    const bool iIn = i >= s0 && i < s1, jIn = j >= s0 && j < s1;
    if (!iIn && !jIn) return;                    // uniform over the workgroup
    const int q2 = q * q;
    const T* src = x + (size_t)L * q + (size_t)p * q2;
    for (int t = threadIdx.x; t < q2; t += blockDim.x) tile[t] = src[t];   // tile[a*q+b]
    __syncthreads();
    for (int t = threadIdx.x; t < q2; t += blockDim.x) {
        const int r = t / q, c = t % q;
        // row (i,a=r), columns (j,b=c): contiguous in b
        if (jIn) W[(size_t)(i * q + r) * Cs + (j - s0) * q + c] = tile[r * q + c];
        // row (j,b=r), columns (i,a=c): contiguous in a
        if (iIn) W[(size_t)(j * q + r) * Cs + (i - s0) * q + c] = tile[c * q + r];
    }
}

// ------------------------------------------------------------------ logits
// S[n][c] = sum_j W[j*q + x_nj][c].  The transpose of the scatter kernel: a workgroup owns a block
// of sequences (NS per wave) and one 512-byte column strip (lane = 8 bytes of a row) and walks the
// sites in tiles of JT = 128/q sites whose q rows each are double-buffered in LDS by LDS-DMA.
// For one site a wave pulls the q rows into q register pairs (ds_read_b64, immediate offsets) and
// then adds, for each of its NS sequences, the row of that sequence's state: the SOURCE register
// is selected with the VGPR index mode (M0 = 0x2000 | 2 x state, src1 relative), so a
// (sequence, site) pair costs one SALU write of M0 and one packed add; the NS running sums are
// fixed registers.  No per-lane LDS addresses, hence no bank conflicts and no row permutation.
// Inner block: generated assembly (tools/gen_plm_asm.py -> logits_gather_asm.inc), accumulator and
// row registers pinned.  Workgroup shape per q (generator LOGITS_CFG): q=21 runs 8 waves x 96
// sequences on 256 VGPRs (768 sequences share one staged tile; the fixed per-site cost of fetching
// the q rows is spread over 96 adds; the site's 48 state dwords live in ONE SGPR set refilled in
// place, in thirds, see the generator), q=5 runs 16 waves x 48 sequences on 128.
typedef float dca_v32f __attribute__((ext_vector_type(32)));
typedef float dca_v16f __attribute__((ext_vector_type(16)));
typedef float dca_v8f __attribute__((ext_vector_type(8)));
typedef float dca_v2f __attribute__((ext_vector_type(2)));
typedef uint32_t dca_v4u __attribute__((ext_vector_type(4)));

#include "logits_gather_asm.inc"

// "q = 25" in the helpers and kernel templates below is the SITE-PAIR ALPHABET of q = 5 (float32 only, round 5): the unit a
// gather block walks is a pair of neighbouring sites (2 jp, 2 jp + 1) with the combined state 5 x1 + x2.  Logits: the 25
// sums W[(j1, b1)] + W[(j2, b2)] are formed once per wave and pair in registers (10 row reads + 25 packed adds), after which
// a sequence costs ONE M0 write and ONE indexed add per PAIR of sites -- (25 + 80) adds per 160 (sequence, site) units.
// Scatter: 25 accumulators per pair selected by the combined state, one add per row and pair, marginalised to 5 + 5 sums
// when the workgroup stores.  An odd L pairs its last site with a padding site (state 0; its rows of W are zero, its rows
// of G lie in the padding of the allocation).  The sums are re-associated, so this is a float32 formulation; the
// float64 (parity) mode keeps the per-site blocks.
__host__ __device__ constexpr int logits_waves(int q) { return q == 21 ? DCA_LOGITS_WAVES_Q21 : q == kPairQ ? DCA_LOGITS_WAVES_Q25 : DCA_LOGITS_WAVES_Q5; }
__host__ __device__ constexpr int logits_nseq(int q) { return q == 21 ? DCA_LOGITS_NSEQ_Q21 : q == kPairQ ? DCA_LOGITS_NSEQ_Q25 : DCA_LOGITS_NSEQ_Q5; }   // per wave
__host__ __device__ constexpr int logits_seq_per_wg(int q) { return logits_waves(q) * logits_nseq(q); }
// 64-byte lines that the 2*nseq bytes of one wave's state words of one site can span (their offset
// is a multiple of 2*nseq)
__host__ __device__ constexpr int logits_lines_per_site(int nseq)
{
    const int bytes = 2 * nseq;
    const int g = (bytes & -bytes) > 64 ? 64 : (bytes & -bytes);
    return (64 - g + bytes + 63) / 64;
}
__host__ __device__ constexpr int logits_jt(int q) { return q == 21 ? 6 : q == kPairQ ? 12 : 25; }   // sites (q = 25: site pairs) per LDS tile (<= 128 rows)
__host__ __device__ constexpr int logits_tile_rows(int q) { return q == kPairQ ? 12 * 2 * 5 : logits_jt(q) * q; }

// XL[j][n] = 0x2000 | 2 * x_nj (M0 image: src1-relative + register-pair offset); state 0 past N and for
// the padding sites j >= L of the last tile (their rows of W are zero)
__global__ void plm_build_logit_states_kernel(const uint8_t* __restrict__ X, uint16_t* __restrict__ XL, int N, int Npad,
                                              int L, int Ls)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (n >= Npad) return;
    XL[(size_t)j * Npad + n] = (uint16_t)(0x2000u | ((n < N && j < L) ? 2u * X[(size_t)n * Ls + j] : 0u));
}

// site-pair alphabet (q = 5): the same M0 images over the combined state 5 x_{n,2jp} + x_{n,2jp+1}; `tag` = 0x2000 for the
// logits kernel (row stride Npad, sequences from 0), 0x9000 for the scatter kernel (row stride NT, owned sequences from halo);
// state 0 past N, for the padding pairs of the last tile and for the padding site that an odd L pairs its last site with
__global__ void plm_build_pair_states_kernel(const uint8_t* __restrict__ X, uint16_t* __restrict__ XP, int N, int stride, int L, int Ls,
                                             int first, uint32_t tag)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int jp = blockIdx.y;
    if (k >= stride) return;
    const int n = first + k;
    uint32_t st = 0;
    if (n < N && 2 * jp < L) {
        const uint8_t* row = X + (size_t)n * Ls;
        st = 5u * row[2 * jp] + (2 * jp + 1 < L ? (uint32_t)row[2 * jp + 1] : 0u);
    }
    XP[(size_t)jp * stride + k] = (uint16_t)(tag | 2u * st);
}

template <int NP>
struct LogitsAcc { dca_v16f p[NP]; };          // sequence s of the wave: p[s / 8][2 * (s % 8) .. +1]

template <int NSEQ, int S = 0>
__device__ __forceinline__ void logits_store(const LogitsAcc<NSEQ / 8>& acc, unsigned char* rowBase, size_t rowStrideBytes, int rowsLeft)
{
    if constexpr (S < NSEQ) {
        if (S < rowsLeft)
            *reinterpret_cast<dca_v2f*>(rowBase + (size_t)S * rowStrideBytes) =
                dca_v2f{acc.p[S / 8][2 * (S % 8)], acc.p[S / 8][2 * (S % 8) + 1]};
        logits_store<NSEQ, S + 1>(acc, rowBase, rowStrideBytes, rowsLeft);
    }
}

// timing experiments only (results are wrong when set): compile with -DDCA_LOGITS_ABLATE=<bits> /
// -DDCA_SCATTER_ABLATE=<bits> -- 1 no per-tile barrier, 2 / 8 no staging of the next tile, 4 no wait for the landed pieces
#ifndef DCA_LOGITS_ABLATE
#define DCA_LOGITS_ABLATE 0
#endif
#ifndef DCA_SCATTER_ABLATE
#define DCA_SCATTER_ABLATE 0
#endif

// JTV (site-pair alphabet only): site pairs per LDS tile, 12 (0), 11 or 10 -- the engine takes the count that pads ceil(L / 2) least
template <typename T, int Q, int JTV = 0>
__global__ __launch_bounds__(logits_waves(Q) * 64)
void plm_logits_kernel(const T* __restrict__ W, const uint16_t* __restrict__ XL, T* __restrict__ S,
                       int N, int Npad, int L, int Cs, int numColTiles, int numNBlocks)
{
    constexpr int WAVES = logits_waves(Q);
    constexpr int NSEQ = logits_nseq(Q);
    constexpr int JT = JTV ? JTV : logits_jt(Q);
    constexpr int TROWS = JTV ? JTV * 2 * 5 : logits_tile_rows(Q);      // rows of W per tile (Q = 25: site pairs = 2 sites of 5 rows)
    static_assert(JTV == 0 || (Q == kPairQ && (JTV == 11 || JTV == 10)), "tile variants exist for the site-pair alphabet only");
    constexpr int CW = 512 / (int)sizeof(T);
    constexpr int TILE = 128 * 512;                 // bytes of one LDS buffer (TROWS <= 128 rows)
    static_assert(Q != kPairQ || sizeof(T) == 4, "the site-pair alphabet is a float32 formulation");
    constexpr int PIECES = TILE / 1024;             // 1 KiB (two rows) per LDS-DMA instruction
    constexpr int DMA_PER_WAVE = (PIECES + WAVES - 1) / WAVES;
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];

    // XCD-aware decode: all sequence blocks of one column strip run on one XCD (workgroup id % 8) so that its slice
    // of W is served by that XCD's L2 -- for the strips that come in full sets of eight.  The sequence blocks of the
    // numColTiles % 8 strips left over go round ALL XCDs (one strip at a time): handing those strips to XCDs 0 .. r-1
    // whole left the other XCDs idle for a round (D: 83 strips, 23 rounds on three XCDs against 21 on five).
    const int id = blockIdx.x;
    const int fullCT = (numColTiles / kNumXcd) * kNumXcd;
    int ct, nb;
    if (id < fullCT * numNBlocks) {
        const int xcd = id % kNumXcd, k = id / kNumXcd;
        ct = (k / numNBlocks) * kNumXcd + xcd;
        nb = k % numNBlocks;
    } else {
        const int r = id - fullCT * numNBlocks;
        ct = fullCT + r / numNBlocks;
        nb = r % numNBlocks;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n0 = nb * (WAVES * NSEQ) + wave * NSEQ;

    LogitsAcc<NSEQ / 8> acc;
#pragma unroll
    for (int i = 0; i < NSEQ / 8; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc.p[i][e] = 0.f;

    const unsigned char* Wbytes = reinterpret_cast<const unsigned char*>(W + (size_t)ct * CW);   // the strip, wave-uniform
    const size_t rowStrideBytes = (size_t)Cs * sizeof(T);
    // LDS-DMA piece p of a tile = rows 2p, 2p+1 (lanes 0-31 / 32-63, 16 bytes per lane); tile jt = rows
    // [jt*JT*Q, +128) of W (the allocation is padded so that the last tile can over-read)
    const uint32_t voff = (uint32_t)((lane >> 5) * rowStrideBytes + (lane & 31) * 16);
    const uint32_t ginc = (uint32_t)(WAVES * 2 * rowStrideBytes);
    auto stage = [&](int jt, int buf) {       // all pieces of this wave at once: only for tile 0
#pragma unroll
        for (int i = 0; i < DMA_PER_WAVE; ++i) {
            const int pairIdx = wave + i * WAVES;                     // wave-uniform
            if (PIECES % WAVES != 0 && pairIdx >= PIECES) break;
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(Wbytes + (size_t)(jt * TROWS + pairIdx * 2) * rowStrideBytes + voff),
                (__attribute__((address_space(3))) void*)(dca_smem + buf * TILE + pairIdx * 1024), 16, 0, 0);
        }
    };

    // The state words are a stream (N*L*2 bytes per strip, far beyond the L2), so the scalar loads
    // of the inner block, issued one site ahead, would wait for HBM at every site.  One vector
    // load per wave and tile touches every 64-byte line of the NEXT tile's state words (lane ->
    // (site, line)), a whole tile ahead; its data goes to a scratch corner of the LDS and is
    // never read -- the point is that the scalar loads then hit the L2 (D: 7.98 -> 7.55 ms, E: 0.79 ->
    // 0.72 ms).  The scatter kernel loads its state words a quarter tile ahead and gains nothing from this.
    constexpr int LPS = logits_lines_per_site(NSEQ);
    static_assert(JT * LPS <= 64, "one prefetch lane per (site, line)");
    const int pfSite = min(lane / LPS, JT - 1);
    const size_t pfLane = (size_t)pfSite * Npad * 2 + (size_t)n0 * 2 + min((lane % LPS) * 64, NSEQ * 2 - 4);
    auto prefetch_states = [&](int jt) {
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(reinterpret_cast<const unsigned char*>(XL) + (size_t)jt * JT * Npad * 2 + pfLane),
            (__attribute__((address_space(3))) void*)(dca_smem + 2 * TILE + wave * 256), 4, 0, 0);
    };

    const int numJT = (L + JT - 1) / JT;
    const uint32_t ldsBase = (uint32_t)(uintptr_t)dca_smem + lane * 8;
    stage(0, 0);
    for (int jt = 0; jt < numJT; ++jt) {
        const int buf = jt & 1;
        if (!(DCA_LOGITS_ABLATE & 4)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile jt have landed
        if (!(DCA_LOGITS_ABLATE & 1)) __syncthreads();                 // ... everyone's; and tile jt-1 is no longer read
        if (jt + 1 < numJT && !(DCA_LOGITS_ABLATE & 8)) prefetch_states(jt + 1);
        const uint16_t* sp = XL + (size_t)jt * JT * Npad + n0;     // wave-uniform
        const uint32_t vbase = ldsBase + buf * TILE;
        const uint32_t strideBytes = (uint32_t)Npad * 2u;
        // the block also issues this wave's LDS-DMA pieces of tile jt+1 (piece i = wave + i*WAVES), spread over its sites
        const uint32_t npc = __builtin_amdgcn_readfirstlane((jt + 1 < numJT && !(DCA_LOGITS_ABLATE & 2)) ? (uint32_t)((PIECES - wave + WAVES - 1) / WAVES) : 0u);
        const unsigned char* gbase = Wbytes + (size_t)((jt + 1) * TROWS + wave * 2) * rowStrideBytes;     // wave-uniform
        const uint32_t ldst = (uint32_t)(uintptr_t)dca_smem + (buf ^ 1) * TILE + wave * 1024;
        if constexpr (Q == kPairQ && JTV == 11) DCA_LOGITS_Q25J11_F32(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else if constexpr (Q == kPairQ && JTV == 10) DCA_LOGITS_Q25J10_F32(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else if constexpr (Q == kPairQ) DCA_LOGITS_Q25_F32(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else if constexpr (Q == 21 && sizeof(T) == 4) DCA_LOGITS_Q21_F32(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else if constexpr (Q == 21) DCA_LOGITS_Q21_F64(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else if constexpr (sizeof(T) == 4) DCA_LOGITS_Q5_F32(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
        else DCA_LOGITS_Q5_F64(vbase, sp, strideBytes, npc, gbase, ginc, voff, ldst, acc);
    }
    if (n0 < N)
        logits_store<NSEQ>(acc, reinterpret_cast<unsigned char*>(S + (size_t)n0 * Cs + (size_t)ct * CW) + lane * 8,
                     rowStrideBytes, N - n0);
}

// ------------------------------------------------------------------ softmax scan
// Lanes = sites, the q states of a site live in registers, so the softmax needs no
// cross-lane traffic.  Each wave owns one chunk of consecutive sequences and walks it
// serially carrying p_{n-1} (plmdca_numerics.cpp:492-530).  In chunked mode a chunk
// starts `warm` sequences early from a zero carry: the carry enters the logits with
// weight <= 1 and d softmax has 1-norm <= 1/2, so the start-up error shrinks by >= 2x
// per step (2^-40 after the default 40) -- far below float/double rounding.
// In: S (logit sums).  Out: R = w_n (p - delta) in a SEPARATE array, fxPart[2 wave], [2 wave + 1] = -sum w_n log p(x_ni) (hi, lo).
// (Not in place: a chunk's warm-up rows belong to its predecessors, which would be overwriting them with R at
// the same time -- chunk 0 has no warm-up and writes row t at its step t while chunk 1 reads it at its step t.)
//
// Memory access: the 64 sites of a wave are one contiguous 64*q*sizeof(T)-byte span of a row.
// It is fetched with 16-byte loads (prefetched DEPTH rows ahead into registers), transposed
// through a wave-private LDS buffer (lane l then reads its q values at stride q: conflict free
// for odd q) and written back the same way, instead of q strided 4-byte accesses per lane.
typedef uint4 __attribute__((may_alias)) dca_u4a;

template <typename T, int Q>
__global__ __launch_bounds__(256)
void plm_softmax_kernel(const T* __restrict__ SR, T* __restrict__ Rout, const T* __restrict__ x, const uint8_t* __restrict__ X,
                        const T* __restrict__ w, double* __restrict__ fxPart,
                        int N, int L, int Ls, int Cs, int halo, int chunk, int warm, int carry, int numChunks, double* __restrict__ colPart)
{
    constexpr int ROWB = 64 * Q * (int)sizeof(T);        // bytes of a wave's span of one row
    constexpr int NP = (ROWB + 1023) / 1024;             // 16-byte pieces per lane
#ifdef DCA_SOFTMAX_DEPTH
    constexpr int DEPTH = DCA_SOFTMAX_DEPTH;             // experiments
#else
    constexpr int DEPTH = NP > 6 ? 2 : 3;                // rows in flight
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int chunkId = blockIdx.y * 4 + wv;
    const int i0 = blockIdx.x * 64;
    const int i = i0 + lane;
    unsigned char* sIn = dca_smem + (size_t)wv * (2 * NP * 1024);
    unsigned char* sOut = sIn + NP * 1024;
    const int rowBytes = (min(64, L - i0) * Q * (int)sizeof(T) + 15) & ~15;
    double facc = 0.0, flo = 0.0;
    // float64, q = 5 (round 5): the double-double column sums of R (the field gradients, plm_colsum_*) are taken here, where
    // R is made, instead of in one more pass over it -- five more double-double accumulators per lane (for q = 21 the 42
    // registers do not fit beside the row buffers).  One partial per (chunk, site, state); colPart == nullptr: not wanted.
    constexpr bool COLSUM = sizeof(T) == 8 && Q == 5;
    [[maybe_unused]] double chi[COLSUM ? Q : 1], clo[COLSUM ? Q : 1];
    if constexpr (COLSUM) {
#pragma unroll
        for (int a = 0; a < Q; ++a) chi[a] = clo[a] = 0.0;
    }
    if (chunkId < numChunks) {
        const int s = halo + chunkId * chunk;
        const int e = min(s + chunk, N);
        const int ws = carry ? max(0, s - warm) : s;
        T h[Q], p[Q];
#pragma unroll
        for (int a = 0; a < Q; ++a) { h[a] = (i < L) ? x[(size_t)i * Q + a] : (T)0; p[a] = 0; }
        uint4 buf[DEPTH][NP];
        int xs[DEPTH];
        T wns[DEPTH];
        auto fetch = [&](int n, int d) {
            const unsigned char* row = reinterpret_cast<const unsigned char*>(SR + (size_t)n * Cs + (size_t)i0 * Q);
#pragma unroll
            for (int pc = 0; pc < NP; ++pc) {
                const int off = pc * 1024 + lane * 16;
                buf[d][pc] = (off < rowBytes) ? *reinterpret_cast<const dca_u4a*>(row + off) : make_uint4(0, 0, 0, 0);
            }
            xs[d] = (i < L) ? (int)X[(size_t)n * Ls + i] : 0;
            wns[d] = w[n];
        };
#pragma unroll
        for (int d = 0; d < DEPTH; ++d)
            if (ws + d < e) fetch(ws + d, d);
        for (int n0 = ws; n0 < e; n0 += DEPTH) {
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) {
                const int n = n0 + d;
                if (n < e) {
#pragma unroll
                    for (int pc = 0; pc < NP; ++pc) *reinterpret_cast<dca_u4a*>(sIn + pc * 1024 + lane * 16) = buf[d][pc];
                    __builtin_amdgcn_wave_barrier();
                    T z[Q];
#pragma unroll
                    for (int a = 0; a < Q; ++a) z[a] = reinterpret_cast<const T*>(sIn)[lane * Q + a] + h[a];
                    const int xi = xs[d];
                    const T wn = wns[d];
                    __builtin_amdgcn_wave_barrier();
                    if (n + DEPTH < e) fetch(n + DEPTH, d);
                    if (carry) {
#pragma unroll
                        for (int a = 0; a < Q; ++a) z[a] += p[a];
                    }
                    T m = z[0];
#pragma unroll
                    for (int a = 1; a < Q; ++a) m = z[a] > m ? z[a] : m;
                    T sum = 0;
#pragma unroll
                    for (int a = 0; a < Q; ++a) { p[a] = t_exp(z[a] - m); sum += p[a]; }
                    const T inv = (T)1 / sum;
#pragma unroll
                    for (int a = 0; a < Q; ++a) p[a] *= inv;
                    if (n >= s) {
                        T px = p[0];
#pragma unroll
                        for (int a = 1; a < Q; ++a) px = (a == xi) ? p[a] : px;
                        if (i < L) dd_add(facc, flo, -(double)(wn * t_log(px)));
#pragma unroll
                        for (int a = 0; a < Q; ++a) {
                            T r = wn * p[a];
                            if (a == xi) r -= wn;
                            reinterpret_cast<T*>(sOut)[lane * Q + a] = r;
                            if constexpr (COLSUM) dd_add(chi[a], clo[a], (double)r);
                        }
                        __builtin_amdgcn_wave_barrier();
                        unsigned char* row = reinterpret_cast<unsigned char*>(Rout + (size_t)n * Cs + (size_t)i0 * Q);
#pragma unroll
                        for (int pc = 0; pc < NP; ++pc) {
                            const int off = pc * 1024 + lane * 16;
                            if (off < rowBytes) *reinterpret_cast<dca_u4a*>(row + off) = *reinterpret_cast<const dca_u4a*>(sOut + off);
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
        }
    }
    if constexpr (COLSUM) {
        if (colPart && chunkId < numChunks && i < L) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const size_t o = 2 * ((size_t)chunkId * L * Q + (size_t)i * Q + a);
                colPart[o] = chi[a];
                colPart[o + 1] = clo[a];
            }
        }
    }
    // fixed-order wave reduction, one (hi, lo) partial per wave
    dd_wave_reduce(facc, flo);
    if (lane == 0) {
        const size_t slot = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4 + wv;
        fxPart[2 * slot] = facc;
        fxPart[2 * slot + 1] = flo;
    }
}

// ------------------------------------------------------------------ scatter (as a gather)
// G[(j,b)][c] = sum_{n : x_nj = b} R[n][c].  A workgroup owns 32 sites (two per wave) and one
// 512-byte column strip of R (lane = 8 bytes of a row) and walks the owned sequences in
// 128-row tiles that are double-buffered in LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per
// wave instruction, no staging registers): tile c+1 streams in while tile c is gathered, one
// barrier per tile.  The q accumulators of a site sit in fixed VGPRs and the one that a row adds
// to is selected with the gfx9 VGPR index mode (s_set_gpr_idx_on; M0 = 0x9000 | 2 x state), so the rows
// are visited in sequence order with immediate LDS offsets: one ds_read_b64 per row shared by the
// wave's two sites and one packed add per (row, site).  The M0 images of the states (XT2) reach SGPRs
// through scalar loads, one s_load_dwordx16 per site and quarter tile, issued a quarter ahead.  The inner block is generated assembly
// (tools/gen_scatter_asm.py -> scatter_gather_asm.inc): 84 accumulator + 16 data-ring registers
// are pinned, which is why the kernel is built for 128 VGPRs (16 waves = one workgroup per CU).
// The sums of a (site, state) run over n in ascending order: deterministic.

// XT2[j][k] = 0x9000 | 2 * x_{halo+k, j}: the M0 image that selects the accumulator of the state
// (index-enable bits for src0 and dst + register-pair offset); state 0 past N (zero rows); row stride NT
__global__ void plm_build_states_kernel(const uint8_t* __restrict__ X, uint16_t* __restrict__ XT2, int N, int L, int Ls,
                                        int halo, int NT)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (k >= NT) return;
    const int n = halo + k;
    XT2[(size_t)j * NT + k] = (uint16_t)(0x9000u | ((n < N) ? 2u * X[(size_t)n * Ls + j] : 0u));
}

#include "scatter_gather_asm.inc"

// accumulators of one site as the register tuples the generated assembly pins
template <int Q> struct SiteAcc;
template <> struct SiteAcc<21> {
    dca_v32f a; dca_v8f b; dca_v2f c;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 32; ++i) a[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = 0.f;
        c[0] = c[1] = 0.f;
    }
    template <int S> __device__ __forceinline__ dca_v2f get() const {
        if constexpr (S < 16) return dca_v2f{a[2 * S], a[2 * S + 1]};
        else if constexpr (S < 20) return dca_v2f{b[2 * (S - 16)], b[2 * (S - 16) + 1]};
        else return c;
    }
};
template <> struct SiteAcc<5> {
    dca_v8f a; dca_v2f b;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = 0.f;
        b[0] = b[1] = 0.f;
    }
    template <int S> __device__ __forceinline__ dca_v2f get() const {
        if constexpr (S < 4) return dca_v2f{a[2 * S], a[2 * S + 1]};
        else return b;
    }
};

template <> struct SiteAcc<kPairQ> {            // a site PAIR of q = 5: accumulator 5 b1 + b2
    dca_v32f a; dca_v16f b; dca_v2f c;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < 32; ++i) a[i] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = 0.f;
        c[0] = c[1] = 0.f;
    }
    template <int S> __device__ __forceinline__ dca_v2f get() const {
        if constexpr (S < 16) return dca_v2f{a[2 * S], a[2 * S + 1]};
        else if constexpr (S < 24) return dca_v2f{b[2 * (S - 16)], b[2 * (S - 16) + 1]};
        else return c;
    }
};

// site pair -> the 5 + 5 rows of its two sites: G[(2 jp, b1)] = sum_b2 A[5 b1 + b2], G[(2 jp + 1, b2)] = sum_b1 A[5 b1 + b2],
// each in ascending order of the summed state; rowBase = row (2 jp, 0) of the strip
template <int B = 0>
__device__ __forceinline__ void scatter_store_pair(const SiteAcc<kPairQ>& acc, unsigned char* rowBase, size_t rowStrideBytes)
{
    if constexpr (B < 5) {
        const dca_v2f first = (((acc.template get<5 * B>() + acc.template get<5 * B + 1>()) + acc.template get<5 * B + 2>()) +
                               acc.template get<5 * B + 3>()) + acc.template get<5 * B + 4>();
        const dca_v2f second = (((acc.template get<B>() + acc.template get<5 + B>()) + acc.template get<10 + B>()) +
                                acc.template get<15 + B>()) + acc.template get<20 + B>();
        *reinterpret_cast<dca_v2f*>(rowBase + (size_t)B * rowStrideBytes) = first;
        *reinterpret_cast<dca_v2f*>(rowBase + (size_t)(5 + B) * rowStrideBytes) = second;
        scatter_store_pair<B + 1>(acc, rowBase, rowStrideBytes);
    }
}

template <int Q, int S = 0>
__device__ __forceinline__ void scatter_store_site(const SiteAcc<Q>& acc, unsigned char* rowBase, size_t rowStrideBytes)
{
    if constexpr (S < Q) {
        *reinterpret_cast<dca_v2f*>(rowBase + (size_t)S * rowStrideBytes) = acc.template get<S>();
        scatter_store_site<Q, S + 1>(acc, rowBase, rowStrideBytes);
    }
}

// float64 mode, end of a canonical block that is not the workgroup's first: G = G + (the block's sums) -- the running sum
// of the finished blocks on the left, as the float64 oracle of the test suite adds them (its ORACLE_CANONICAL_BLOCK).  A lane's 8
// bytes are one double; every address is read and written by this lane only.
template <int Q, int S, int GROUP, int K = 0>
__device__ __forceinline__ void scatter_add_rows_f64(const SiteAcc<Q>& acc, const double (&v)[GROUP], unsigned char* rowBase, uint32_t laneOff,
                                                     size_t rowStrideBytes)
{
    if constexpr (K < GROUP && S + K < Q) {
        *reinterpret_cast<double*>(rowBase + (size_t)(S + K) * rowStrideBytes + laneOff) = v[K] + __builtin_bit_cast(double, acc.template get<S + K>());
        scatter_add_rows_f64<Q, S, GROUP, K + 1>(acc, v, rowBase, laneOff, rowStrideBytes);
    }
}

// rowBase: the wave-uniform address of row (site, 0) of the strip, laneOff = 8 * lane -- kept apart so that the row
// addresses are scalar base + 32-bit lane offset (no 64-bit address registers per row).
template <int Q, int S = 0>
__device__ __forceinline__ void scatter_add_site_f64(const SiteAcc<Q>& acc, unsigned char* rowBase, uint32_t laneOff, size_t rowStrideBytes)
{
    if constexpr (S < Q) {
        constexpr int GROUP = 7;          // rows in flight: the accumulators are pinned and the kernel has 128 registers
        double v[GROUP];
#pragma unroll
        for (int k = 0; k < GROUP; ++k)
            if (S + k < Q) v[k] = *reinterpret_cast<const double*>(rowBase + (size_t)(S + k) * rowStrideBytes + laneOff);
        scatter_add_rows_f64<Q, S, GROUP>(acc, v, rowBase, laneOff, rowStrideBytes);
        asm volatile("" ::: "memory");
        scatter_add_site_f64<Q, S + GROUP>(acc, rowBase, laneOff, rowStrideBytes);
    }
}

template <typename T, int Q, int JW, int WAVES_>
__global__ __launch_bounds__(WAVES_ * 64)
void plm_scatter_kernel(const T* __restrict__ R, const uint16_t* __restrict__ XT2,
                        T* __restrict__ G, int N, int L, int Cs, int halo, int numChunks, int NT, int ctBase, int numPairs, int splitX,
                        int numJG, int chunksPerSplit, size_t slabElems, int blockChunks,
                        int firstBlocksX, int ctBase2, int numPairs2, int splitX2, int chunksPerSplit2)
{
    constexpr int WAVES = WAVES_;                      // 16; 8 or 4 in the float64 mode on alignments with few column strips (configure)
    constexpr int JG = WAVES * JW;                     // sites (Q = 25: site pairs; L is then their number) per workgroup
    constexpr int QROWS = Q == kPairQ ? 10 : Q;        // rows of G per unit
    constexpr int CW = kRowBytes / (int)sizeof(T);     // columns per strip
    constexpr int DMA_PER_WAVE = kNC / 2 / WAVES;      // LDS-DMA instructions per wave and tile
    constexpr int TILE = kNC * kRowBytes;
    static_assert(kNC % (2 * WAVES) == 0, "tile rows must divide over the waves");
    static_assert(JW == 2 && (Q == 21 || Q == 5 || (Q == kPairQ && sizeof(T) == 4)), "no generated gather block for this shape");
    static_assert(WAVES == 16 || (sizeof(T) == 8 && (WAVES == 8 || WAVES == 4)), "no generated gather block for this workgroup size");
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];

    // workgroup id -> (XCD, (column strip, tile-range split) pair, site group): the numJG site groups of a pair run on
    // the same XCD (id % 8) so that their reads of the strip can meet in that XCD's L2.  The main launch has one pair
    // per strip and the splits in blockIdx.y; the launch for the strips left over after the full sets of eight
    // (launch_eval) carries a finer split in the pair index (splitX) so that it fills all XCDs for a fraction of a round.
    // A launch may carry a SECOND set of (strip, split) pairs behind the first firstBlocksX workgroups of every grid row -- the
    // left-over strips with their finer split (round 6: as a launch of their own they ran AFTER the main one, which at config C
    // leaves 32 CUs idle for its whole length: 269 + 48 us; merged they fill those CUs).  The second set has no blockIdx.y.
    int id = blockIdx.x;
    if (id >= firstBlocksX) {
        if (blockIdx.y != 0) return;
        id -= firstBlocksX; ctBase = ctBase2; numPairs = numPairs2; splitX = splitX2; chunksPerSplit = chunksPerSplit2; blockChunks = 0;
    }
    const int xcd = id % kNumXcd, k = id / kNumXcd;
    const int pr = (k / numJG) * kNumXcd + xcd;
    const int jg = k % numJG;
    if (pr >= numPairs) return;
    const int ct = ctBase + pr / splitX;
    const int split = blockIdx.y + pr % splitX;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j0 = jg * JG + wave * JW;

    // blockIdx.y splits the tile range; every split writes its own slab of G (summed by
    // the fold kernels in a fixed order), so small L*q shapes still fill the chip.
    const int cBegin = split * chunksPerSplit;
    const int cEnd = min(numChunks, cBegin + chunksPerSplit);

    SiteAcc<Q> acc[JW];
    const uint32_t* xs[JW];
#pragma unroll
    for (int jj = 0; jj < JW; ++jj) {
        acc[jj].zero();
        xs[jj] = reinterpret_cast<const uint32_t*>(XT2 + (size_t)min(j0 + jj, L - 1) * NT);
    }

    // LDS-DMA piece p of a tile = rows 2p, 2p+1 (lanes 0-31 / 32-63, 16 bytes per lane); a wave stages pieces
    // 4*wave .. 4*wave+3.  R has kNC zero rows behind row N-1, so the last tile needs no special case.
    const unsigned char* Rbytes = reinterpret_cast<const unsigned char*>(R + (size_t)ct * CW);    // the strip, wave-uniform
    const size_t rowStrideBytes = (size_t)Cs * sizeof(T);
    const uint32_t voff = (uint32_t)((lane >> 5) * rowStrideBytes + (lane & 31) * 16);
    const uint32_t ginc = (uint32_t)(2 * rowStrideBytes);
    auto tile_src = [&](int c) { return Rbytes + (size_t)(halo + c * kNC + wave * DMA_PER_WAVE * 2) * rowStrideBytes; };
    auto stage = [&](int c, int buf) {        // all four pieces at once: only for the first tile
#pragma unroll
        for (int i = 0; i < DMA_PER_WAVE && !(DCA_SCATTER_ABLATE & 8); ++i)
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(tile_src(c) + (size_t)i * ginc + voff),
                (__attribute__((address_space(3))) void*)(dca_smem + buf * TILE + (wave * DMA_PER_WAVE + i) * 1024), 16, 0, 0);
    };

    if (cBegin < cEnd) stage(cBegin, 0);
    const uint32_t ldsBase = (uint32_t)(uintptr_t)dca_smem + lane * 8;
    T* const Gslab = G + (size_t)split * slabElems;
    auto run_tiles = [&](int cFrom, int cTo) {
        for (int c = cFrom; c < cTo; ++c) {
            const int buf = (c - cBegin) & 1;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of tile c have landed
            if (!(DCA_SCATTER_ABLATE & 1)) __syncthreads();                 // ... everyone's; and tile c-1 is no longer read
            const uint32_t vbase = ldsBase + buf * TILE;
            // two sites per wave: the state words come through scalar loads inside the block, which also
            // issues the wave's four LDS-DMA pieces of tile c+1, one per quarter tile
            const uint32_t* sp0 = xs[0] + c * (kNC / 2);
            const uint32_t* sp1 = xs[1] + c * (kNC / 2);
            const uint32_t npc = __builtin_amdgcn_readfirstlane((c + 1 < cEnd && !(DCA_SCATTER_ABLATE & 8)) ? 1u : 0u);
            const unsigned char* gbase = tile_src(c + 1);
            const uint32_t ldst = (uint32_t)(uintptr_t)dca_smem + (buf ^ 1) * TILE + wave * DMA_PER_WAVE * 1024;
            uint32_t vtmp;
            [[maybe_unused]] uint32_t vw;       // LDS address / staging registers of the generator's register-staged variant
            [[maybe_unused]] dca_v4u stg;       // (DCA_GEN_SC_STAGE=vgpr; the shipped LDS-DMA blocks do not use them)
            if constexpr (Q == kPairQ)
                DCA_GATHER_Q25_F32_SMEM(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[0].c, acc[1].a, acc[1].b, acc[1].c);
            else if constexpr (Q == 21 && sizeof(T) == 4)
                DCA_GATHER_Q21_F32_SMEM(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[0].c, acc[1].a, acc[1].b, acc[1].c);
            else if constexpr (Q == 21 && WAVES == 16)
                DCA_GATHER_Q21_F64_SMEM(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[0].c, acc[1].a, acc[1].b, acc[1].c);
            else if constexpr (Q == 21 && WAVES == 8)
                DCA_GATHER_Q21_F64_SMEM_W8(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[0].c, acc[1].a, acc[1].b, acc[1].c);
            else if constexpr (Q == 21)
                DCA_GATHER_Q21_F64_SMEM_W4(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[0].c, acc[1].a, acc[1].b, acc[1].c);
            else if constexpr (sizeof(T) == 4)
                DCA_GATHER_Q5_F32_SMEM(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[1].a, acc[1].b);
            else if constexpr (WAVES == 16)
                DCA_GATHER_Q5_F64_SMEM(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[1].a, acc[1].b);
            else if constexpr (WAVES == 8)
                DCA_GATHER_Q5_F64_SMEM_W8(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[1].a, acc[1].b);
            else
                DCA_GATHER_Q5_F64_SMEM_W4(vbase, sp0, sp1, npc, gbase, ginc, voff, ldst, vtmp, stg, vw, acc[0].a, acc[0].b, acc[1].a, acc[1].b);
        }
    };
    auto row_base = [&](int jj, uint32_t laneOff) {
        return reinterpret_cast<unsigned char*>(Gslab + (size_t)(j0 + jj) * QROWS * Cs + (size_t)ct * CW) + laneOff;
    };
    auto row_base_uniform = [&](int jj) { return reinterpret_cast<unsigned char*>(Gslab + (size_t)(j0 + jj) * QROWS * Cs + (size_t)ct * CW); };

    if constexpr (sizeof(T) == 8) {
        // float64 (parity) mode: the chains run over canonical blocks of blockChunks tiles (kCanonBlock sequences), each
        // summed from zero; a workgroup with several blocks stores the first block's sums and adds every later block to the
        // running sum in G: ((B0 + B1) + B2) + ..., the oracle's order (blockChunks = 0: one chain over the whole range)
        const int blockLen = blockChunks > 0 ? blockChunks : max(1, cEnd - cBegin);
        for (int cb = cBegin; cb < cEnd || cb == cBegin; cb += blockLen) {
#pragma unroll
            for (int jj = 0; jj < JW; ++jj) acc[jj].zero();
            run_tiles(cb, min(cEnd, cb + blockLen));
            // the lane offset is re-made per block: as a loop invariant the 2 Q row addresses of the flush were hoisted out of
            // the block loop and spilled (142 registers of the 128 this kernel is built for)
            uint32_t laneOff = lane * 8;
            asm volatile("" : "+v"(laneOff));
#pragma unroll
            for (int jj = 0; jj < JW; ++jj)
                if (j0 + jj < L) {
                    if (cb == cBegin) scatter_store_site<Q>(acc[jj], row_base(jj, laneOff), rowStrideBytes);
                    else scatter_add_site_f64<Q>(acc[jj], row_base_uniform(jj), laneOff, rowStrideBytes);
                }
        }
    } else {
        run_tiles(cBegin, cEnd);
#pragma unroll
        for (int jj = 0; jj < JW; ++jj)
            if (j0 + jj < L) {
                if constexpr (Q == kPairQ) scatter_store_pair(acc[jj], row_base(jj, lane * 8), rowStrideBytes);
                else scatter_store_site<Q>(acc[jj], row_base(jj, lane * 8), rowStrideBytes);
            }
    }
}

// G[0] += G[1] + ... + G[nsplit-1], fixed order (deterministic).  Used when there are more than two slabs
// (deep, narrow alignments); with a few slabs the fold kernels add them on the fly.
template <typename T>
__global__ void plm_sum_slabs_kernel(T* __restrict__ G, size_t slabElems, int nsplit)
{
    // 16 bytes per lane and load, four slabs' loads in flight before their adds (round 6: config E sums 17 slabs of 2.9 MB --
    // 27 us with one 4-byte load per add, the adds of an element in the same ascending slab order as before)
    using V = typename V16<T>::type;
    constexpr int VEC = 16 / (int)sizeof(T);
    const size_t nv = slabElems / VEC, stride = (size_t)gridDim.x * blockDim.x, t0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    auto add = [](V& a, const V& v) {
        a.x += v.x; a.y += v.y;
        if constexpr (sizeof(T) == 4) { a.z += v.z; a.w += v.w; }
    };
    const bool aligned = (slabElems % VEC) == 0 && (reinterpret_cast<uintptr_t>(G) & 15) == 0;
    if (aligned) {
        for (size_t iv = t0; iv < nv; iv += stride) {
            V a = reinterpret_cast<const V*>(G)[iv];
            int sidx = 1;
            for (; sidx + 4 <= nsplit; sidx += 4) {
                const V b0 = reinterpret_cast<const V*>(G + (size_t)sidx * slabElems)[iv];
                const V b1 = reinterpret_cast<const V*>(G + (size_t)(sidx + 1) * slabElems)[iv];
                const V b2 = reinterpret_cast<const V*>(G + (size_t)(sidx + 2) * slabElems)[iv];
                const V b3 = reinterpret_cast<const V*>(G + (size_t)(sidx + 3) * slabElems)[iv];
                add(a, b0); add(a, b1); add(a, b2); add(a, b3);
            }
            for (; sidx < nsplit; ++sidx) add(a, reinterpret_cast<const V*>(G + (size_t)sidx * slabElems)[iv]);
            reinterpret_cast<V*>(G)[iv] = a;
        }
        return;
    }
    for (size_t i = t0; i < slabElems; i += stride) {
        T a = G[i];
        for (int sidx = 1; sidx < nsplit; ++sidx) a += G[(size_t)sidx * slabElems + i];
        G[i] = a;
    }
}

// The same for a column range whose slab count differs from the rest (the left-over strips of the scatter kernel):
// slab 0 receives the sum of slabs 0 .. nsplit-1, slabs 1 .. nzero-1 are cleared so that later sums over them add nothing.
template <typename T>
__global__ void plm_sum_slabs_cols_kernel(T* __restrict__ G, size_t slabElems, int Cs, int col0, int ncols, int rows, int nsplit, int nzero)
{
    const size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (idx >= (size_t)rows * ncols) return;
    const size_t off = (idx / ncols) * (size_t)Cs + col0 + idx % ncols;
    T a = G[off];
    for (int sidx = 1; sidx < nsplit; ++sidx) a += G[(size_t)sidx * slabElems + off];
    G[off] = a;
    for (int sidx = 1; sidx < nzero; ++sidx) G[(size_t)sidx * slabElems + off] = (T)0;
}

// ------------------------------------------------------------------ column sums of R (float64 mode)
// g[h_i(a)] needs sum_n R[n][(i,a)].  The float32 path reads it off G (sum over the states of site 0's rows); in float64
// mode -- the parity mode -- it is summed in double-double, i.e. independently of the order, like the objective: the
// oracle compensates the same sums (ORACLE_CANONICAL_F64), so both round the same exact value.  One more pass over R.
template <typename T>
__global__ __launch_bounds__(256)
void plm_colsum_parts_kernel(const T* __restrict__ R, int N, int Cs, int Lq, double* __restrict__ parts)
{
    __shared__ double redHi[4][64], redLo[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int rpb = (N + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rpb, r1 = min(N, r0 + rpb);
    double hi = 0.0, lo = 0.0;
    if (c < Lq)
        for (int n = r0 + wv; n < r1; n += 4) dd_add(hi, lo, (double)R[(size_t)n * Cs + c]);
    redHi[wv][lane] = hi; redLo[wv][lane] = lo;
    __syncthreads();
    if (wv == 0 && c < Lq) {
        for (int w = 1; w < 4; ++w) dd_add2(hi, lo, redHi[w][lane], redLo[w][lane]);
        parts[2 * ((size_t)blockIdx.y * Lq + c)] = hi;
        parts[2 * ((size_t)blockIdx.y * Lq + c) + 1] = lo;
    }
}
// the softmax kernel's per-chunk partials (q = 5): row block b of the output = the chunks b, b + gridDim.y, ... in that order
__global__ __launch_bounds__(256)
void plm_colsum_chunks_kernel(const double* __restrict__ chunkParts, int numChunks, int Lq, double* __restrict__ parts)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Lq) return;
    double hi = 0.0, lo = 0.0;
    for (int k = blockIdx.y; k < numChunks; k += gridDim.y) dd_add2(hi, lo, chunkParts[2 * ((size_t)k * Lq + c)], chunkParts[2 * ((size_t)k * Lq + c) + 1]);
    parts[2 * ((size_t)blockIdx.y * Lq + c)] = hi;
    parts[2 * ((size_t)blockIdx.y * Lq + c) + 1] = lo;
}
__global__ void plm_colsum_final_kernel(const double* __restrict__ parts, int nblocks, int Lq, double* __restrict__ colSum)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= Lq) return;
    double hi = 0.0, lo = 0.0;
    for (int b = 0; b < nblocks; ++b) dd_add2(hi, lo, parts[2 * ((size_t)b * Lq + c)], parts[2 * ((size_t)b * Lq + c) + 1]);
    colSum[c] = hi + lo;
}

// ------------------------------------------------------------------ column-strip decomposition: parameter pieces
// pairs (j, i), j in [j0, j1) (sender's sites), i in [i0, i1) (receiver's sites, i0 >= j1), between the packed vector and
// a dense [j][i][q*q] message
template <typename T, bool PACK>
__global__ void strip_pairs_copy_kernel(T* __restrict__ x, T* __restrict__ buf, int L, int q, int j0, int j1, int i0, int i1)
{
    const int ni = i1 - i0;
    const int j = j0 + blockIdx.x / ni, i = i0 + blockIdx.x % ni;
    const int q2 = q * q;
    T* px = x + (size_t)L * q + pair_index(L, j, i) * q2;
    T* pb = buf + (size_t)blockIdx.x * q2;
    for (int t = threadIdx.x; t < q2; t += blockDim.x) {
        if (PACK) pb[t] = px[t];
        else px[t] = pb[t];
    }
}

// ------------------------------------------------------------------ fold
// g[J_ij(a,b)] = 2 lambda_J J + G[(j,b)][(i,a)] + G[(i,a)][(j,b)]   (plmdca_numerics.cpp:541-602:
// the site-i and the site-j conditional both contribute), regulariser value per pair
// (:473-486) as a double partial.
// G arrives as `nsplit` slabs (one per tile-range split of the scatter grid); they are summed here in
// slab order, which is what a separate pass over the slabs would produce.
template <typename T>
__device__ __forceinline__ T slab_sum(const T* __restrict__ G, size_t off, size_t slabElems, int nsplit)
{
    T a = G[off];
    for (int sidx = 1; sidx < nsplit; ++sidx) a += G[(size_t)sidx * slabElems + off];
    return a;
}

// One WAVE per site pair (four pairs per workgroup): a pair is q*q = 441 elements, and with a workgroup per pair the
// small configurations were bound by workgroup dispatch and three dependent global round trips per workgroup
// (config C: 19 900 workgroups, 0.143 ms for 0.35 GB).
constexpr int kFoldWaves = 4;
// Column-strip decomposition: rank r holds the columns of sites [site0[r], site0[r+1]) and folds the pairs (i, j), i < j,
// whose FIRST site it holds.  Site i's conditional of such a pair lies in its own G; site j's lies in the G of the rank that
// holds j's columns, which has sent its rows of this rank's sites: recv[r'] = (this rank's L q rows) x recvCs[r'] columns.
struct StripMap {
    int rank = 0, world = 1, s0 = 0, s1 = 0;
    int site0[kMaxStripRanks + 1];
    const void* recv[kMaxStripRanks];
    int recvCs[kMaxStripRanks];
};
// g[h_i(a)] = 2 lambda_h h + sum_n R[n][(i,a)]; the column sum of R is the sum over b of
// any site's rows of G (site 0 here).  (:463-471, :538-539, :573-578)
// colSum (float64 mode): the column sums of R summed order-independently by plm_colsum_* below; else they are taken
// from G as described above.
template <typename T>
__device__ __forceinline__ void fold_fields_body(const T* __restrict__ x, const T* __restrict__ G, T* __restrict__ g,
                                                 double* __restrict__ regPart, int Lq, int q, int Cs, T lambdaH, int addReg,
                                                 size_t slabElems, int nsplit, const double* __restrict__ colSum, int blk)
{
    __shared__ double red[256];
    const int c = blk * blockDim.x + threadIdx.x;
    double reg = 0.0;
    if (c < Lq) {
        const T xv = x[c];
        T gv = addReg ? (T)2 * lambdaH * xv : (T)0;
        T s = 0;
        if (colSum) s = (T)colSum[c];
        else for (int b = 0; b < q; ++b) s += slab_sum(G, (size_t)b * Cs + c, slabElems, nsplit);
        g[c] = gv + s;
        if (addReg) reg = (double)lambdaH * (double)xv * (double)xv;
    }
    __shared__ double redLo[256];
    red[threadIdx.x] = reg;
    redLo[threadIdx.x] = 0.0;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) dd_add2(red[threadIdx.x], redLo[threadIdx.x], red[threadIdx.x + s], redLo[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { regPart[2 * (size_t)blk] = red[0]; regPart[2 * (size_t)blk + 1] = redLo[0]; }
}
template <typename T>
__global__ void plm_fold_fields_kernel(const T* __restrict__ x, const T* __restrict__ G, T* __restrict__ g,
                                       double* __restrict__ regPart, int Lq, int q, int Cs, T lambdaH, int addReg,
                                       size_t slabElems, int nsplit, const double* __restrict__ colSum)
{
    fold_fields_body<T>(x, G, g, regPart, Lq, q, Cs, lambdaH, addReg, slabElems, nsplit, colSum, (int)blockIdx.x);
}
// what the pair fold carries behind its own workgroups when the fields ride in its launch (one GPU: round 6)
template <typename T> struct FoldFieldsArgs { const T* x; T* g; double* regPart; int Lq; T lambdaH; const double* colSum; int pairBlocks; };
template <typename T>
__global__ __launch_bounds__(64 * kFoldWaves)
void plm_fold_pairs_kernel(const T* __restrict__ x, const T* __restrict__ G, T* __restrict__ g,
                           const PairIJ* __restrict__ pairs, double* __restrict__ regPart,
                           int L, int q, int Cs, T lambdaJ, int addReg, size_t slabElems, int nsplit, int pairBegin, int pairEnd,
                           const StripMap sm, const FoldFieldsArgs<T> ff)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dca_smem[];
    if (ff.pairBlocks >= 0 && (int)blockIdx.x >= ff.pairBlocks) {      // the field fold's workgroups, behind the pairs'
        fold_fields_body<T>(ff.x, G, ff.g, ff.regPart, ff.Lq, q, Cs, ff.lambdaH, addReg, slabElems, nsplit, ff.colSum, (int)blockIdx.x - ff.pairBlocks);
        return;
    }
    const int q2 = q * q;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    T* tile = reinterpret_cast<T*>(dca_smem) + (size_t)wave * ((q2 + 3) / 4 * 4);     // G[(j,b)][(i,a)] stored as tile[b*q+a]
    const int p = pairBegin + blockIdx.x * kFoldWaves + wave;
    if (p >= pairEnd) return;                                  // wave-uniform; no workgroup barriers below
    const int i = pairs[p].i, j = pairs[p].j;
    const int ic = (i - sm.s0) * q;                            // site i's first column in this rank's window
    for (int t = lane; t < q2; t += 64) {
        const int b = t / q, a = t % q;
        tile[t] = slab_sum(G, (size_t)(j * q + b) * Cs + ic + a, slabElems, nsplit);
    }
    // site j's conditional: this rank's G when it holds j's columns too, else the rows its holder has sent
    const T* Gj = G;
    size_t jRow = (size_t)i * q, jCs = (size_t)Cs;
    int jc = (j - sm.s0) * q, jSplit = nsplit;
    if (j >= sm.s1) {
        int r = sm.rank + 1;
        while (j >= sm.site0[r + 1]) ++r;
        Gj = static_cast<const T*>(sm.recv[r]);
        jRow = (size_t)(i - sm.s0) * q; jCs = (size_t)sm.recvCs[r]; jc = (j - sm.site0[r]) * q; jSplit = 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const size_t base = (size_t)L * q + (size_t)p * q2;
    double reg = 0.0, regLo = 0.0;
    for (int t = lane; t < q2; t += 64) {
        const int a = t / q, b = t % q;
        const T xv = x[base + t];
        // (2 lambda x + site i's conditional) + site j's conditional: the order of the reference's one-thread merge
        // (plmdca_numerics.cpp:570-602 in ascending site order) and of the oracle
        T gv = addReg ? (T)2 * lambdaJ * xv : (T)0;
        gv += tile[b * q + a];                                                            // G[(j,b)][(i,a)]: column of site i
        gv += slab_sum(Gj, (jRow + a) * jCs + jc + b, slabElems, jSplit);                 // G[(i,a)][(j,b)]: column of site j
        g[base + t] = gv;
        if (addReg) dd_add(reg, regLo, (double)lambdaJ * (double)xv * (double)xv);
    }
    dd_wave_reduce(reg, regLo);                                               // fixed tree
    if (lane == 0) { regPart[2 * (size_t)p] = reg; regPart[2 * (size_t)p + 1] = regLo; }
}

}  // namespace
